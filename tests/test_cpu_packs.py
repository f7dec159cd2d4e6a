"""The pack cache that the seven network heads share (packs.PackedWeights), the view cutter and the size-query table, without a GPU:
what drops a pack, what moves the key, and where check() raises -- per class exactly where the class raised before it joined the
mixin: train mode for Backbone, ResnetEncoder, FAN and Encoder4Editing; a trainable parameter for every class but Encoder4Editing
(its own forward trains) and FLAME (which never had a check)."""
import copy
import os
import pickle
import re

import pytest
import torch

from util import ROOT

# name -> (module path, constructor, check() raises in train mode, check() raises on a trainable parameter)
HEADS = {
    'Backbone': ('id_loss', lambda m: m.Backbone(), 'eval mode only', 'no gradient for the facenet weights'),
    'ResnetEncoder': ('deca', lambda m: m.ResnetEncoder(), 'eval mode only', 'no gradient for the encoder weights'),
    'FAN': ('landmarks', lambda m: m.FAN(4), 'eval mode only', 'no gradient for the weights'),
    'S3FD': ('face_detector', lambda m: m.S3FD(), None, 'no gradient for the weights'),
    'FLAME': ('flame', lambda m: m.FLAME(), None, None),
    'LPIPS': ('lpips', lambda m: m.LPIPS(), None, 'no gradient for the LPIPS weights'),
    'Encoder4Editing': ('encoder', lambda m: m.Encoder4Editing(50, 'ir_se', 32), r'train\(\) mode', None),
}
PLANTED = ('key', torch.zeros(1), [])


@pytest.fixture(scope='module', params=list(HEADS))
def head(request):
    import importlib
    path, make, train_words, grad_words = HEADS[request.param]
    m = make(importlib.import_module('stylegan_directions_face_reenactment_amd.' + path)).eval()
    return m, train_words, grad_words


def test_every_head_is_on_the_mixin(head):
    from stylegan_directions_face_reenactment_amd.packs import PackedWeights
    m = head[0]
    assert isinstance(m, PackedWeights) and m._pack is None
    for name in ('_key', 'packed', '_apply', '__getstate__', 'check'):           # one definition: nobody overrides these
        assert getattr(type(m), name) is getattr(PackedWeights, name), name


def test_a_planted_pack_is_dropped_by_every_copy_move_and_load(head):
    m = head[0]
    try:
        m._pack = PLANTED
        twin = copy.deepcopy(m)
        assert twin._pack is None and m._pack is PLANTED and not twin.training
        assert pickle.loads(pickle.dumps(m))._pack is None and m._pack is PLANTED
        assert '_pack' not in m.state_dict()
        m.float()
        assert m._pack is None
        m._pack = PLANTED
        m._apply(lambda t: t)
        assert m._pack is None
        m._pack = PLANTED
        m.load_state_dict(m.state_dict())
        assert m._pack is None
        m._pack = PLANTED
        m.invalidate_packs()
        assert m._pack is None
    finally:
        m._pack = None


def test_key_moves_with_an_in_place_write_and_with_nothing_else(head):
    m = head[0]
    entries = list(m.state_dict(keep_vars=True).items())
    k0 = m._key()
    assert len(k0) == len(entries) and all(e == (t.data_ptr(), t._version, t.device) for e, (_, t) in zip(k0, entries))
    m.train()
    m.eval()
    m.state_dict()
    assert m._key() == k0
    picks = {entries[0][0]: entries[0][1], entries[-1][0]: entries[-1][1]}
    picks.update((n, b) for n, b in list(m.named_buffers())[:1])                 # a buffer too, where the class has one
    for name, t in picks.items():
        before = m._key()
        with torch.no_grad():
            t.add_(0)
        after = m._key()
        assert after != before and m._key() == after, name
        assert sum(a != b for a, b in zip(after, before)) == 1, name


def test_check_raises_where_it_did(head):
    m, train_words, grad_words = head
    m.check()                                                                    # eval mode, as constructed
    m.train()
    try:
        if train_words is None:
            m.check()
        else:
            with pytest.raises(RuntimeError, match=train_words):
                m.check()
    finally:
        m.eval()
    p = next(p for p in m.parameters() if p.is_floating_point())
    was = p.requires_grad
    p.requires_grad_(True)
    try:
        if grad_words is None:
            m.check()
        else:
            with pytest.raises(RuntimeError, match=grad_words):
                m.check()
    finally:
        p.requires_grad_(was)
    m.check()


# ---------------------------------------------------------------------------------------------------------------- the view cutter
@pytest.mark.parametrize('align', [1, 64])
def test_views_cut_consecutive_aligned_views(align):
    from stylegan_directions_face_reenactment_amd.packs import views
    rows, shapes = 3, ((5, 7), (11,), (2, 3, 4), (64,))
    offsets, o = [], 0
    for s in shapes:
        offsets.append(o)
        o = -(-(o + rows * int(torch.Size(s).numel())) // align) * align
    buf = torch.arange(o, dtype=torch.float32)
    cut = views(buf, rows, align=align)
    for s, want in zip(shapes, offsets):
        v = cut(s)
        assert tuple(v.shape) == (rows,) + s and v.storage_offset() == want and v.is_contiguous()
        assert v.data_ptr() == buf.data_ptr() + 4 * want and float(v.flatten()[0]) == want
    cut.done()
    assert (align == 1) == (offsets == [0, 105, 138, 210]) and (align == 64) == (offsets == [0, 128, 192, 320])


@pytest.mark.parametrize('align', [1, 64])
def test_views_done_fires_on_a_buffer_one_element_too_long(align):
    from stylegan_directions_face_reenactment_amd.packs import views
    n = 2 * 64
    cut = views(torch.zeros(n + 1), 2, align=align)
    cut((64,))
    with pytest.raises(AssertionError, match=r'\(%d, %d\)' % (n, n + 1)):
        cut.done()


# ---------------------------------------------------------------------------------------------------------------- the size queries
def test_size_queries_are_declared_in_the_header_with_their_argument_counts():
    from stylegan_directions_face_reenactment_amd import _native
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    declared = dict(re.findall(r'^int64_t\s+(sgdfr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', header, re.M))
    assert set(_native.SIZE_QUERIES) == set(declared)                # every int64_t function of the header is a size query
    for name, nargs in _native.SIZE_QUERIES.items():
        args = [a.strip() for a in declared[name].split(',') if a.strip() not in ('', 'void')]
        assert len(args) == nargs and all(re.fullmatch(r'int\s+\w+', a) for a in args), (name, declared[name])
    counts = set(re.findall(r'^int\s+(sgdfr_[a-z0-9_]+_count)\s*\(\s*int\s+\w+\s*\)\s*;', header, re.M))
    assert set(_native.COUNT_QUERIES) <= counts
    assert not set(_native.SIZE_QUERIES) & set(_native.SIGNATURES)

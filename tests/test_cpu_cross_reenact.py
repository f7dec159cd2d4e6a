"""CPU: the parts of cross-reenactment that are plain tensors or host checks: the TargetAnalysis container, the hold policy
for S sources against S separate calls, the byte map of a uint8 panel against images_to_uint8's arithmetic restated in numpy, and what
video_frames_px and reenact_many refuse before anything is launched.  The pipeline itself runs in tests/test_gpu_cross_reenact.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cross_reenact_restatement as X
from util import ROOT, golden


def bits(a, b):
    if a.dtype in (torch.uint8, torch.bool):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def analysis(n, seed, batch=2, keys=('pose', 'alpha_exp', 'alpha_shp', 'cam'), S=8):
    from stylegan_directions_face_reenactment_amd.reenact import TargetAnalysis
    g = torch.Generator().manual_seed(seed)
    widths = {'pose': 6, 'alpha_exp': 50, 'alpha_shp': 100, 'cam': 3, 'other': 2}
    params = {k: torch.randn(n, widths[k], generator=g) for k in keys}
    params[keys[0]][::2, 0] = -0.0                                        # a bit pattern a float comparison would not tell apart
    return TargetAnalysis(torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8), params, torch.randn(n, 3, generator=g),
                          torch.rand(n, generator=g) < 0.6, torch.rand(n, generator=g) < 0.8, batch)


def same(a, b):
    return (len(a) == len(b) and a.batch == b.batch and list(a.params) == list(b.params) and bits(a.crops, b.crops)
            and bits(a.angles, b.angles) and bits(a.ok, b.ok) and bits(a.valid, b.valid)
            and all(bits(a.params[k], b.params[k]) for k in a.params))


def test_target_analysis_slices_joins_saves_and_moves_every_field_bit_for_bit(tmp_path):
    from stylegan_directions_face_reenactment_amd.reenact import TargetAnalysis
    a = analysis(7, 1)
    assert len(a) == 7 and a.batch == 2 and a.device.type == 'cpu'
    # slices are views of the same rows
    lo, hi = a[:4], a[4:]
    assert len(lo) == 4 and len(hi) == 3 and lo.crops.data_ptr() == a.crops.data_ptr() and bits(hi.params['cam'], a.params['cam'][4:])
    assert bits(a[2:5].ok, a.ok[2:5]) and bits(a[2:5].valid, a.valid[2:5]) and bits(a[2:5].angles, a.angles[2:5])
    assert same(TargetAnalysis.cat([lo, hi]), a) and same(TargetAnalysis.cat([a[:2], a[2:4], a[4:6], a[6:]]), a)
    assert len(a[3:3]) == 0 and same(TargetAnalysis.cat([a[:0], a]), a)
    with pytest.raises(RuntimeError, match='slice'):
        a[3]
    with pytest.raises(RuntimeError, match='slice'):
        a[::2]
    # a cache across processes: plain tensors and ints through torch.save / torch.load
    d = a.as_dict()
    assert all(torch.is_tensor(v) or isinstance(v, int) for v in d.values()) and d['batch'] == 2
    path = os.path.join(str(tmp_path), 'analysis.pt')
    torch.save(d, path)
    assert same(TargetAnalysis.from_dict(torch.load(path)), a)
    with pytest.raises(RuntimeError, match='lacks'):
        TargetAnalysis.from_dict({k: v for k, v in d.items() if k != 'ok'})
    moved = a.to('cpu')
    assert same(moved, a) and moved.device.type == 'cpu'
    # cat refuses what does not belong together
    with pytest.raises(RuntimeError, match='batch'):
        TargetAnalysis.cat([a, analysis(3, 2, batch=4)])
    with pytest.raises(RuntimeError, match='param keys'):
        TargetAnalysis.cat([a, analysis(3, 2, keys=('pose', 'alpha_exp', 'other'))])
    with pytest.raises(RuntimeError, match='non-empty'):
        TargetAnalysis.cat([])
    # the constructor refuses fields that do not fit
    with pytest.raises(RuntimeError, match='uint8'):
        TargetAnalysis(a.crops.float(), a.params, a.angles, a.ok, a.valid, 2)
    with pytest.raises(RuntimeError, match='ok must be'):
        TargetAnalysis(a.crops, a.params, a.angles, a.ok[:5], a.valid, 2)
    with pytest.raises(RuntimeError, match='valid must be'):
        TargetAnalysis(a.crops, a.params, a.angles, a.ok, a.valid.int(), 2)
    with pytest.raises(RuntimeError, match='params'):
        TargetAnalysis(a.crops, {'pose': a.params['pose'][:3]}, a.angles, a.ok, a.valid, 2)
    with pytest.raises(RuntimeError, match='batch'):
        TargetAnalysis(a.crops, a.params, a.angles, a.ok, a.valid, 0)


OK_PATTERNS = {'all true': [True] * 7, 'all false': [False] * 7, 'first row false': [False] + [True] * 6,
               'alternating': [True, False] * 3 + [True], 'alternating from false': [False, True] * 3 + [False]}


@pytest.mark.parametrize('pattern', sorted(OK_PATTERNS))
def test_hold_over_three_sources_equals_three_separate_calls(pattern):
    """N = 7 rows, S = 3 sources, NaNs in the failed rows: one pass with the rows found once equals S hold_failed_rows calls from an
    empty carry, and ok rows pass through bit for bit."""
    from stylegan_directions_face_reenactment_amd.reenact import hold_failed_rows_many
    ok = torch.tensor(OK_PATTERNS[pattern])
    sv = torch.randn(3, 7, 15, generator=torch.Generator().manual_seed(11))
    sv[:, ::3, 0] = -0.0
    poisoned = sv.clone()
    poisoned[:, ~ok] = float('nan')
    got = hold_failed_rows_many(poisoned, ok)
    want = X.hold_per_source(poisoned, ok)
    assert got.shape == (3, 7, 15) and bits(got, want), pattern
    assert bits(got[:, ok], sv[:, ok]) and bool(torch.isfinite(got).all())
    if not ok[0]:                                                         # before the first ok row: zeros, every source from an empty carry
        first = OK_PATTERNS[pattern].index(True) if any(OK_PATTERNS[pattern]) else 7
        assert (got[:, :first] == 0).all() and not torch.signbit(got[:, :first]).any()
    assert hold_failed_rows_many(sv[:, :0], ok[:0]).shape == (3, 0, 15)


def test_byte_map_of_a_uint8_panel_is_the_two_float_maps_and_not_the_identity():
    """All 256 values: reenact.uint8_panel_map (torch float32) equals images_to_uint8's arithmetic restated in numpy applied to the crop
    kernel's byte -> float map.  The truncation sends u to u - 1; the fixed points are printed."""
    from stylegan_directions_face_reenactment_amd.reenact import BLANK_BYTE, uint8_panel_map
    table = uint8_panel_map()
    want = X.panel_byte_map()
    assert table.dtype == torch.uint8 and table.shape == (256,) and np.array_equal(table.numpy(), want)
    v = X.crop_byte_to_float(np.arange(256))
    assert v.dtype == np.float32 and v[0] == -1.0 and v[255] == 1.0 and np.all(np.diff(v) > 0)
    fixed = [u for u in range(256) if int(want[u]) == u]
    down = [u for u in range(256) if int(want[u]) == u - 1]
    print('uint8 panel map: fixed points %s, %d values map to u - 1, table[:4] = %s, table[252:] = %s'
          % (fixed, len(down), want[:4].tolist(), want[252:].tolist()))
    assert len(fixed) + len(down) == 256 and 0 in fixed and len(down) >= 200           # never more than one count, mostly one down
    assert np.all(np.diff(want.astype(np.int32)) >= 0)
    # the byte of an invalid row's float crop (0.0 in every pixel)
    assert int(X.image_to_u8(np.zeros(1, np.float32))[0]) == BLANK_BYTE == 127


def cpu_reenactor():
    from stylegan_directions_face_reenactment_amd import reenact
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.model import Generator
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    G = Generator(32, 512, 8, channel_multiplier=1)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    shifts = ShiftVectors('voxceleb', 15, 6.0, ranges=golden('kat8_shift.npz')['ranges_voxceleb'])
    return reenact.Reenactor(G, A, None, None, None, None, shifts, truncation=1.0)


def test_video_frames_px_refuses_before_any_launch():
    from stylegan_directions_face_reenactment_amd.reenact import video_frames_px
    x = torch.zeros(2, 3, 8, 8)
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    out = torch.zeros(2, 8, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        video_frames_px(x, [], 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        video_frames_px(None, [u8], 8, out=out)
    with pytest.raises(RuntimeError, match='no CPU path'):
        video_frames_px(None, [x], 8, out=out)
    with pytest.raises(RuntimeError, match='float32'):
        video_frames_px(x.double(), [], 8)
    with pytest.raises(RuntimeError, match=r'float32 \[rows,3,P,P\] or uint8'):
        video_frames_px(None, [x.half()], 8, out=out)
    with pytest.raises(RuntimeError, match=r'float32 \[rows,3,P,P\] or uint8'):
        video_frames_px(None, [u8.to(torch.int8)], 8, out=out)
    with pytest.raises(RuntimeError, match='int32'):
        video_frames_px(None, [u8], 8, out=out, index=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='int32'):
        video_frames_px(None, [u8], 8, out=out, index=[torch.zeros(2)])
    with pytest.raises(RuntimeError, match='index entries'):
        video_frames_px(None, [u8], 8, out=out, index=[None, None])
    with pytest.raises(RuntimeError, match='up to 3'):
        video_frames_px(None, [u8, u8, u8, u8], 8, out=out)
    with pytest.raises(RuntimeError, match='skipped panel'):
        video_frames_px(None, [u8], 8)                                    # x=None skips the last panel: `out` has to hold it


def test_video_frames_px_c_entry_refuses_bad_arguments_and_is_declared():
    from stylegan_directions_face_reenactment_amd import _native as N
    lib = N.load()
    fake = ctypes.c_void_p(64)                                            # never dereferenced: every case is refused first
    def panels(*rows):
        arr = (N.VideoPanel * 3)()
        for k, (data, index, kind, n) in enumerate(rows):
            arr[k].data, arr[k].index, arr[k].kind, arr[k].rows = data, index, kind, n
        return arr
    good = panels((64, None, N.PANEL_F32, 1), (None, None, 0, 0), (64, 64, N.PANEL_U8, 9))
    call = lib.sgdfr_video_frames_px
    assert call(fake, 2, 8, 3, good, 3, fake, 0, None) != 0 and b'1, 2 or 4' in lib.sgdfr_last_error()
    assert call(fake, 2, 8, 1, good, 4, fake, 0, None) != 0 and b'left panels' in lib.sgdfr_last_error()
    assert call(fake, 2, 8, 1, None, 1, fake, 0, None) != 0 and b'descriptor' in lib.sgdfr_last_error()
    assert call(fake, 2, 8, 1, panels((64, None, 2, 1)), 1, fake, 0, None) != 0 and b'kind' in lib.sgdfr_last_error()
    assert call(fake, 2, 8, 1, panels((64, None, N.PANEL_U8, 0)), 1, fake, 0, None) != 0 and b'rows' in lib.sgdfr_last_error()
    assert call(fake, 2, 8, 1, panels((64, None, N.PANEL_U8, 3)), 1, fake, 0, None) != 0 and b'without an index' in lib.sgdfr_last_error()
    assert call(fake, 2, 8, 1, good, 3, None, 0, None) != 0 and b'null' in lib.sgdfr_last_error()
    assert call(None, 0, 8, 1, good, 3, None, 0, None) == 0                                       # no rows: nothing to do
    assert call(None, 2, 8, 1, panels((None, None, 0, 0)), 1, None, 0, None) == 0                 # no x, no panel: nothing to do
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    assert 'sgdfr_video_frames_px' in set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header)) and 'sgdfr_video_frames_px' in N.SIGNATURES
    assert 'struct sgdfr_video_panel' in header and [f[0] for f in N.VideoPanel._fields_] == ['data', 'index', 'kind', 'rows']
    assert N.ABI_VERSION == 23 and lib.sgdfr_abi_version() == 23          # one symbol added, nothing moved


def test_reenact_many_and_its_kin_refuse_before_any_launch():
    from stylegan_directions_face_reenactment_amd.reenact import Source, TargetAnalysis
    r = cpu_reenactor()
    a = analysis(4, 3, S=256)
    src = Source(torch.zeros(1, 8, 512), r.G, torch.zeros(1, 3, 256, 256), torch.zeros(1, 256, 256, 3, dtype=torch.uint8),
                 {k: v[:1] for k, v in a.params.items()}, a.angles[:1], None, None)
    with pytest.raises(RuntimeError, match='no CPU path'):
        r.reenact_many([src], a)
    with pytest.raises(RuntimeError, match='no CPU path'):
        r.reenact_analysed(a)
    with pytest.raises(RuntimeError, match='no CPU path'):
        r.analyse(torch.zeros(2, 96, 128, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='Sources'):
        r.reenact_many([], a)
    with pytest.raises(RuntimeError, match='Sources'):
        r.reenact_many([{'code': None}], a)
    with pytest.raises(RuntimeError, match='TargetAnalysis'):
        r.reenact_many([src], a.as_dict())
    with pytest.raises(RuntimeError, match='valid must be a bool'):
        r.reenact_many([src], a, valid=torch.ones(4))
    with pytest.raises(RuntimeError, match='valid must be a bool'):
        r.reenact_analysed(a, valid=torch.ones(3, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='on_fail'):
        r.reenact_many([src], a, on_fail='skip')
    with pytest.raises(RuntimeError, match='output'):
        r.reenact_analysed(a, output='grid')
    with pytest.raises(RuntimeError, match='Source'):
        r.use_source({'code': None})
    with pytest.raises(RuntimeError, match=r'\[1,4,15\]'):
        r.cross_metrics([src], a, torch.zeros(4, 15), None)
    with pytest.raises(RuntimeError, match='no CPU path'):
        r.cross_metrics([src], a, torch.zeros(1, 4, 15), None)
    # use_source selects without a launch and resets the hold carry
    r.use_source(src)
    assert r.G_source is r.G and r.session is not None and r.source_x is src.x and not bool(r._carry_valid) and (r._carry == 0).all()

"""CPU: the e4e encoder with the head count apart from the input side.  The restatement (tests/e4e_restatement.py) against the
fixture written from the reference's own Encoder4Editing(50, 'ir_se', 512 / 1024) on small inputs (tests/golden/kat24_e4e_styles.npz,
scripts/make_golden_e4e_styles.py), the `_n` entries of the C ABI against the entries they generalise, and what `encode` refuses."""
import os
import re

import pytest
import torch

from util import ROOT, S, golden
import e4e_restatement as R
import e4e_styles_cases as C

BAR = 8.0


@pytest.fixture(scope='module')
def kat():
    return golden(C.KAT)


@pytest.mark.parametrize('name', ['d', 'e'])
def test_restatement_against_the_reference_fixture(kat, name):
    """fp64 within 1e-10 max|w| of the reference's fp64 codes; fp32 within 8 x the reference's own max |fp32 - fp64|: the bars of
    test_cpu_e4e_taps."""
    enc, state = C.make_encoder(S, name)
    x = C.fixture_inputs(S, name)
    want = torch.from_numpy(kat['w_' + name])
    top = float(want.abs().max())
    assert abs(top - float(kat['max_w_' + name])) == 0.0
    with torch.no_grad():
        t64 = R.forward(state, x.double())
        t32 = R.forward(state, x)
    e64 = float((t64['w'] - want).abs().max())
    e32 = float((t32['w'].double() - want).abs().max())
    dev = float(kat['dev_w_' + name])
    print('case %s: fp64 restatement %.3e (bar %.3e), fp32 restatement %.3e = %.2f x dev_w %.3e (bar %.0f x)' % (
        name, e64, 1e-10 * top, e32, e32 / dev, dev, BAR))
    B, side = C.CASES[name][:2]
    assert enc.style_count == C.heads(name) == len(enc.styles) and enc.input_size == side
    assert tuple(t64['w'].shape) == tuple(want.shape) == (B, C.heads(name), 512)
    assert tuple(t64['h_fine'].shape) == (B, C.heads(name) - 7, 512) and tuple(t64['p1'].shape) == (B, 512, side // 4, side // 4)
    assert e64 <= 1e-10 * top and e32 <= BAR * dev
    assert all(('dev_%s_%s' % (k, name)) in kat.files for k in R.TAPS)


def test_fixture_holds_the_three_cases_below_the_size_limit(kat):
    assert [C.heads(n) for n in 'def'] == [18, 16, 18]
    for name in 'def':
        B = C.CASES[name][0]
        assert tuple(kat['w_' + name].shape) == (B, C.heads(name), 512) and kat['w_' + name].dtype.name == 'float64'
        assert float(kat['dev_w_' + name]) > 0 and float(kat['max_w_' + name]) > 0
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', C.KAT)) < 1 << 20


def test_c_abi_declares_the_n_entries():
    from stylegan_directions_face_reenactment_amd import _native
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    declared = set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header))
    names = {'sgdfr_e4e_param_count_n', 'sgdfr_e4e_pack_elems_n', 'sgdfr_e4e_debug_elems_n', 'sgdfr_e4e_workspace_bytes_n',
             'sgdfr_e4e_prepack_n_f32', 'sgdfr_e4e_forward_n_f32'}
    assert names <= declared
    assert {'sgdfr_e4e_prepack_n_f32', 'sgdfr_e4e_forward_n_f32'} <= set(_native.SIGNATURES)
    assert _native.SIZE_QUERIES['sgdfr_e4e_pack_elems_n'] == 2 and _native.SIZE_QUERIES['sgdfr_e4e_debug_elems_n'] == 3
    assert _native.SIZE_QUERIES['sgdfr_e4e_workspace_bytes_n'] == 3 and _native.COUNT_QUERIES_N == {'sgdfr_e4e_param_count_n': 2}
    lib = _native.load()
    assert all(hasattr(lib, n) for n in names)


def test_n_queries_equal_the_old_ones_at_the_input_sides_own_head_count():
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    for res in range(32, 257, 16):
        n = lib.sgdfr_e4e_style_count(res)
        assert lib.sgdfr_e4e_param_count_n(res, n) == lib.sgdfr_e4e_param_count(res) > 0, res
        assert lib.sgdfr_e4e_pack_elems_n(res, n) == lib.sgdfr_e4e_pack_elems(res) > 0, res
        for rows in (1, 3):
            assert lib.sgdfr_e4e_debug_elems_n(rows, res, n) == lib.sgdfr_e4e_debug_elems(rows, res) > 0, res
            assert lib.sgdfr_e4e_workspace_bytes_n(rows, res, n) == lib.sgdfr_e4e_workspace_bytes(rows, res) > 0, res


def test_n_queries_count_the_heads_and_refuse_what_is_out_of_range():
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    assert lib.sgdfr_e4e_param_count_n(256, 18) == 423 + 4 * 14            # four more fine heads: 6 convs and a linear, two tensors each
    assert lib.sgdfr_e4e_param_count_n(256, 16) == 423 + 2 * 14
    for res in (32, 80, 256):
        for n in range(8, 19):
            convs = sum(4 if j < 3 else 5 if j < 7 else 6 for j in range(n))
            assert lib.sgdfr_e4e_param_count_n(res, n) == 3 + 10 * 24 + 4 + 2 * convs + 2 * n
    for n in (7, 19, 0, -1):
        assert lib.sgdfr_e4e_param_count_n(256, n) == -1 and lib.sgdfr_e4e_pack_elems_n(256, n) == -1
        assert lib.sgdfr_e4e_debug_elems_n(1, 256, n) == -1 and lib.sgdfr_e4e_workspace_bytes_n(1, 256, n) == -1
        assert lib.sgdfr_e4e_forward_n_f32(None, 1, 256, n, None, None, None, None, 0, None) != 0 and b'style heads' in lib.sgdfr_last_error()
        assert lib.sgdfr_e4e_prepack_n_f32(None, 256, n, None, None) != 0 and b'style heads' in lib.sgdfr_last_error()
    for bad in (16, 272, 512):
        assert lib.sgdfr_e4e_param_count_n(bad, 18) == -1 and lib.sgdfr_e4e_pack_elems_n(bad, 18) == -1
        assert lib.sgdfr_e4e_debug_elems_n(1, bad, 18) == -1 and lib.sgdfr_e4e_workspace_bytes_n(1, bad, 18) == -1
        assert lib.sgdfr_e4e_forward_n_f32(None, 1, bad, 18, None, None, None, None, 0, None) != 0 and b'resolution' in lib.sgdfr_last_error()
    assert lib.sgdfr_e4e_workspace_bytes_n(0, 64, 18) == -1 and lib.sgdfr_e4e_workspace_bytes_n(257, 64, 18) == -1
    assert lib.sgdfr_e4e_prepack_n_f32(None, 64, 18, None, None) != 0 and b'null' in lib.sgdfr_last_error()


def test_workspace_grows_only_where_the_fine_maps_pass_the_unit_buffer():
    """The two parked head-map buffers hold max(64, 8 G_fine) R^2 floats per row: up to 15 heads (G_fine = 8: 64 R^2) the layout
    is the old one, 16 and 18 heads add 2 x (72 - 64) and 2 x (88 - 64) R^2 per row and the head vectors past the 14th."""
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()

    def align(n):
        return (n + 63) // 64 * 64

    for rows, res in ((1, 32), (3, 80), (2, 256)):
        base = lib.sgdfr_e4e_workspace_bytes(rows, res)
        r2 = rows * res * res
        for n in range(8, 19):
            parked = max(64, 8 * (n - 7)) * r2
            vecs = rows * max(n, 14) * 512
            want = base + 4 * (2 * (align(parked) - align(64 * r2)) + 2 * (align(vecs) - align(rows * 14 * 512)))
            assert lib.sgdfr_e4e_workspace_bytes_n(rows, res, n) == want, (rows, res, n)


def test_encode_refuses_bad_input_sizes_and_head_counts():
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _ = C.make_encoder(S, 'd')
    assert (enc.image_resolution, enc.input_size, enc.style_count) == (1024, 32, 18)
    assert E.Encoder4Editing(50, 'ir_se', 64).input_size == 64 and E.Encoder4Editing(50, 'ir_se', 1024).input_size == 256
    with pytest.raises(RuntimeError, match='no CPU path'):
        E.encode(enc, torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match='built for 32x32'):
        E.encode(enc, torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match=r'\[B,3,32,32\]'):
        E.encode(enc, torch.zeros(3, 32, 32))
    # the 512 generator's encoder reads the 256 x 256 crop: a 512 x 512 image is still refused, in the old words
    enc512 = E.Encoder4Editing(50, 'ir_se', 512).eval()
    assert (enc512.input_size, enc512.style_count) == (256, 16)
    with pytest.raises(ValueError, match='multiple of 16'):
        E.encode(enc512, torch.zeros(1, 3, 512, 512))
    with pytest.raises(ValueError, match='built for 256x256'):
        E.encode(enc512, torch.zeros(1, 3, 512, 512))
    for bad in (512, 40, 16, 272, 64.0, True):
        with pytest.raises(ValueError, match='multiple of 16'):
            E.encode(E.Encoder4Editing(50, 'ir_se', 64, input_size=bad).eval(), torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match='style heads'):                 # image_resolution 2048: 20 heads
        E.encode(E.Encoder4Editing(50, 'ir_se', 2048, input_size=32).eval(), torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match='style heads'):                 # image_resolution 16: 6 heads
        E.encode(E.Encoder4Editing(50, 'ir_se', 16, input_size=32).eval(), torch.zeros(1, 3, 32, 32))


def test_prepack_plan_and_debug_views_follow_the_head_count():
    from stylegan_directions_face_reenactment_amd import _native, encoder as E
    lib = _native.load()
    enc, _ = C.make_encoder(S, 'd')
    ps = E.folded(enc)
    assert len(ps) == lib.sgdfr_e4e_param_count_n(32, 18)
    assert enc._prepack_plan(ps) == (len(ps), (32, 18), (32, 18))
    with pytest.raises(RuntimeError, match='folded tensors'):
        enc._prepack_plan(ps[:-2])
    total = sum(p.numel() for p in ps if p is not None)
    assert total <= lib.sgdfr_e4e_pack_elems_n(32, 18) <= total + 64 * len(ps)
    n = lib.sgdfr_e4e_debug_elems_n(2, 32, 18)
    v = E.debug_views(torch.zeros(n), 2, 32, 18)
    assert tuple(v['h_fine'].shape) == (2, 11, 512) and tuple(v['p1'].shape) == (2, 512, 8, 8)

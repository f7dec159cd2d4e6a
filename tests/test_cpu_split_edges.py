"""Self-checks of the reference machinery of tests/test_gpu_split_edges.py (tests/split_refs.py), on the CPU: the references it reuses
are torch's fp64 convolutions at odd and non-square sizes, the Winograd restatements are the convolution, the decoders invert an encoder
written from include/sgdfr.h, the exact weights map to the intended dyadics, the restated host rules are the library's own (swept through
its host queries), every accept / refuse boundary is found from both sides, and the case lists reach every plan, geometry class, staging
slot count, slice count and launch form they claim to.  The run prints which case reaches which."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import conv_refs as R
import split_refs as Q
from util import O, S  # noqa: F401  (puts the repository root on sys.path)

P3, U3, D3 = Q.PLAIN3, Q.UP3, Q.DOWN3


def _lib():
    from stylegan_directions_face_reenactment_amd import _native
    return _native.load()


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def _w_oihw(wp):
    return wp.permute(2, 0, 1).reshape(wp.shape[2], wp.shape[0], 3, 3).double()


# ------------------------------------------------------------------ references

@pytest.mark.parametrize('B,cin,cout,H,W', [(2, 16, 32, 5, 7), (3, 16, 64, 1, 1), (1, 16, 32, 3, 250), (2, 64, 32, 2, 2)])
def test_references_of_the_split_cases_are_torchs_fp64_convolutions(B, cin, cout, H, W):
    """conv_reference at H != W and odd sizes, on the inputs the GPU module uses (raw weight, scale in fp64): conv2d / conv_transpose2d
    / the stride-2 conv of the interleaved planes; the bound dominates the fp32 one and is zero exactly where the reference reads no
    product (the plane entries outside the transposed-conv result)."""
    for kind, arith in (('int', 'fp16x3'), ('real', 'bf16x3'), ('real', 'fp16f8')):
        c = Q.C(P3, B, cin, cout, H, W, noise='per', bias=True, act=True)
        i = Q.case_inputs(kind, c, arith)
        wc = i['w'][0].double() / (9 * cin) ** 0.5
        assert _close(_w_oihw(i['wp64']), wc)
        want = TF.conv2d(i['x'].double() * i['s'].double()[:, :, None, None], wc, padding=1) * i['d'].double()[:, :, None, None]
        want = want + float(i['noise_w']) * i['noise'].double() + i['bias'].double()[None, :, None, None]
        want = torch.where(want > 0, want, want * Q.SLOPE) * Q.GAIN
        ref, bound = Q.conv_reference(c, i, arith)
        assert _close(ref, want)
        fp32 = R.plain3_ref(i['x'], i['wp64'], i['s'], i['d'], i['noise'], i['noise_w'], i['bias'], act=True, slope=Q.SLOPE, gain=Q.GAIN)[1]
        assert bool((bound >= fp32).all()) and bool((bound > 0).all())
        c = Q.C(U3, B, cin, cout, H, W)
        i = Q.case_inputs(kind, c, arith)
        planes, bound = Q.conv_reference(c, i, arith)
        T = R.planes_to_full(planes)
        want = TF.conv_transpose2d(i['x'].double() * i['s'].double()[:, :, None, None], (i['w'][0].double() / (9 * cin) ** 0.5).transpose(0, 1),
                                   stride=2) * i['d'].double()[:, :, None, None]
        assert _close(T[:, :, :2 * H + 1, :2 * W + 1], want)
        out = R.planes_outside(H, W)
        assert bool((planes[:, :, out] == 0).all()) and bool((bound[:, :, out] == 0).all()) and bool((bound[:, :, ~out] > 0).all())
    # DOWN3: forward layer cdx -> C planes; the conv takes the C-channel planes (times d) to cdx channels
    C_, cdx = 16, 256
    for kind, arith in (('int', 'fp16x3'), ('real', 'bf16x3')):
        c = Q.C(D3, B, C_, cdx, H, W)
        i = Q.case_inputs(kind, c, arith)
        assert i['w'].shape == (1, C_, cdx, 3, 3)
        full = R.planes_to_full(i['x'].double() * i['s'].double()[:, :, None, None, None])[:, :, :2 * H + 1, :2 * W + 1]
        wc = i['w'][0].double() / (9 * cdx) ** 0.5                                      # [C, cdx, 3, 3]
        want = TF.conv2d(full, wc.transpose(0, 1).contiguous(), stride=2)
        ref, bound = Q.conv_reference(c, i, arith)
        assert ref.shape == (B, cdx, H, W) and _close(ref, want) and bool((bound > 0).all())
        # ... which is the input gradient of the transposed conv (autograd)
        u = torch.zeros(B, cdx, H, W, dtype=torch.float64, requires_grad=True)
        Tt = TF.conv_transpose2d(u, wc.transpose(0, 1).contiguous(), stride=2)       # weight [in = cdx, out = C, 3, 3]
        Tt.backward(full)
        assert _close(ref, u.grad)


@pytest.mark.parametrize('f', [2, 4])
def test_winograd_row_forms_are_the_convolution(f):
    """A^T ((B^T d) (.) (G g)) with the matrices of csrc/common.h and csrc/wsplit.hip is the plain conv; its absolute-value form bounds
    it; |B^T d| <= 2 / 10 max|d| (WSPLIT_GROWTH_LOG2); even integer weights (f = 2) give an integral G w."""
    B, cin, cout, H, W = 2, 16, 8, 5, 16
    x = S.counter_tensor(5, 'wsx', (B, cin, H, W))
    s = S.counter_tensor(5, 'wss', (B, cin), 1.0, 0.3)
    w = S.counter_tensor(5, 'wsw', (cout, cin, 3, 3)).double()
    xs = x.double() * s.double()[:, :, None, None]
    V = Q.ws_input_ref(xs, f)
    assert V.shape == (B, cin, f + 2, H, W // f)
    ref, _ = R.plain3_ref(x, R.wp_of(w), s)
    assert _close(Q.ws_conv(V, w, f), ref)
    assert bool((Q.ws_conv(V, w, f, absolute=True) >= ref.abs() * (1 - 1e-12)).all())
    assert float(Q.WS_BT[f].abs().sum(1).max()) == (2.0 if f == 2 else 10.0) and 2 ** Q.WSPLIT_GROWTH_LOG2[f] >= float(Q.WS_BT[f].abs().sum(1).max())
    assert float(V.abs().max()) <= float(Q.WS_BT[f].abs().sum(1).max()) * float(xs.abs().max())
    # the row border: the first tile's d_0 and the last tile's d_{f+1} are zero, not the neighbour row's values
    d = R._pad(xs, 0, 0, 1, 1).unfold(3, f + 2, f)
    assert bool((d[:, :, :, 0, 0] == 0).all()) and bool((d[:, :, :, -1, -1] == 0).all()) and bool((d[:, :, :, 0, 1] == xs[:, :, :, 0]).all())
    k = torch.tensor(Q.exact_weight_values(16, 'fp16x3', even=True), dtype=torch.float64)
    Gk = torch.einsum('tk,abk->abt', Q.WS_G[2], torch.stack(torch.meshgrid(k, k, k, indexing='ij'), -1).reshape(-1, 1, 3))
    assert torch.equal(Gk, Gk.round())


def _encode(v, arith):
    """hi = round16(v), lo = round16(v - hi) as split_pair forms them (include/sgdfr.h), v already range-shifted."""
    dt = torch.bfloat16 if arith == 'bf16x3' else torch.float16
    hi = v.float().to(dt)
    lo = (v.float() - hi.float()).to(dt)
    return hi, lo


@pytest.mark.parametrize('arith', Q.ARITHS)
def test_decoders_invert_the_documented_forms(arith):
    """An encoder written from the layouts include/sgdfr.h documents, decoded again: xs, the WS form, the phase-major DOWN3 input and the
    interleaved padded planes; hi + lo is within split_step of the value and equal to it where split_fits says so."""
    B, C, H, W = 2, 16, 3, 8
    sh = 1.0 if arith == 'bf16x3' else 16.0
    v = S.counter_tensor(3, 'dec.v', (B, C, H, W)).double()
    hi, lo = _encode(v / sh, arith)

    def chunks(t):      # [B,C,N] -> [B,C/8,N,8]
        return t.reshape(B, C // 8, 8, -1).permute(0, 1, 3, 2)
    xs = torch.stack([chunks(hi.reshape(B, C, -1)), chunks(lo.reshape(B, C, -1))], 2).contiguous().view(torch.int16)
    got = Q.decode_xs(xs, B, C, H, W, arith)
    assert bool(((got - v).abs() <= Q.split_step(v, arith)).all())
    vi = R.int_tensor(3, 'dec.i', (B * C, H * W), -8, 8).view(B, C, H, W).double() * 0.5
    hi, lo = _encode(vi / sh, arith)
    assert Q.split_fits(vi, arith) and bool((lo.float() == 0).all())
    xs = torch.stack([chunks(hi.reshape(B, C, -1)), chunks(lo.reshape(B, C, -1))], 2).contiguous().view(torch.int16)
    assert torch.equal(Q.decode_xs(xs, B, C, H, W, arith), vi)
    for f in (2, 4):    # WS: [B][C/8][t][hi,lo][H W/f][8]
        V = Q.ws_input_ref(v, f)                                          # [B,C,f+2,H,TW]
        hi, lo = _encode(V / sh, arith)

        def wchunks(t):     # [B,C,T,H,TW] -> [B,C/8,T,HT,8]
            return t.reshape(B, C // 8, 8, f + 2, -1).permute(0, 1, 3, 4, 2)
        vs = torch.stack([wchunks(hi), wchunks(lo)], 3).contiguous().view(torch.int16)
        got = Q.decode_ws(vs, B, C, H, W, f, arith)
        assert got.shape == V.shape and bool(((got - V).abs() <= Q.split_step(V, arith)).all())
    # phase-major planes: chunk index ph C/8 + c/8
    P = S.counter_tensor(3, 'dec.p', (B, C, 4, H + 1, W + 1)).double()
    hi, lo = _encode(P / sh, arith)

    def pchunks(t):     # [B,C,4,R,P] -> [B,4 C/8,RP,8]
        return t.reshape(B, C // 8, 8, 4, -1).permute(0, 3, 1, 4, 2).reshape(B, 4 * C // 8, -1, 8)
    ps = torch.stack([pchunks(hi), pchunks(lo)], 2).contiguous().view(torch.int16)
    got = Q.decode_split_planes(ps, B, C, H, W, arith)
    assert bool(((got - P).abs() <= Q.split_step(P, arith)).all())
    # interleaved padded planes [B][Cout][stride][px][py]
    RP, stride = (H + 1) * (W + 1), 64
    y = torch.full((B, C, stride, 2, 2), -7.0, dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            y[:, :, :RP, px, py] = P[:, :, 2 * py + px].reshape(B, C, RP)
    planes, pad = Q.decode_planes_il(y.reshape(B, C, 4, stride), B, C, H, W, stride)
    assert torch.equal(planes, P) and pad.shape == (B, C, stride - RP, 4) and bool((pad == -7).all())


def test_exact_weights_map_to_the_intended_dyadics():
    """numpy float32, as sgdfr_modconv_prepack_split_f32 forms the value: w * fl32(64 / sqrtf(9 Cin)) (bf16: fl32(1 / sqrtf)) is 64 k
    (k) for every weight k sqrt(9 Cin) of the exact sets; no other Cin below 1024 has an integral sqrt(9 Cin) that is a multiple of 16's."""
    for cs, root in ((16, 12), (64, 24), (256, 48)):
        for arith in ('fp16x3', 'bf16x3', 'fp16f8'):
            good = Q.exact_weight_values(cs, arith)
            assert good == list(range(-8, 9)), (cs, arith, good)              # none had to be dropped
            assert Q.exact_weight_values(cs, arith, even=True) == list(range(-8, 9, 2))
            scale = (np.float32(1.0) if arith == 'bf16x3' else np.float32(64.0)) / np.sqrt(np.float32(cs) * np.float32(9))
            for k in good:
                got = np.float32(np.float32(k * root) * scale)
                assert float(got) == (k if arith == 'bf16x3' else 64 * k)
                assert Q.split_fits(torch.tensor([float(got)]) * (1.0 if arith == 'bf16x3' else 16.0), 'bf16x3' if arith == 'bf16x3' else 'fp16x3')
    assert [c for c in range(16, 1025, 16) if (9 * c) ** 0.5 % 1 == 0] == [16, 64, 144, 256, 400, 576, 784, 1024]
    for c in Q.all_direct_cases():
        cs = c['cout'] if c['mode'] == D3 else c['cin']
        if cs in (16, 64, 256):
            for arith in ('fp16x3', 'bf16x3'):
                assert Q.exact_condition(c['cin'] * (4 if c['mode'] == D3 else 1), arith=arith), Q.case_id(c)
    i = Q.case_inputs('int', Q.C(P3, 3, 16, 64, 5, 7, noise='per', bias=True), 'fp16x3')
    assert float(i['x'].abs().max()) <= 8 and float(i['wp64'].abs().max()) <= 8 and torch.equal(i['wp64'], i['wp64'].round())
    assert torch.equal(i['w'][0].double(), Q._w_from_wp(i['wp64'])[0] * 12) and set(i['s'].unique().tolist()) <= {0.5, 1.0, 2.0}
    assert float(i['wp64'].view(-1)[0]) != 0 and float(i['wp64'].view(-1)[-1]) != 0
    assert all(Q.exact_condition(c['cin'], taps=3, growth=2) for c in Q.WSPLIT_CASES if c['f'] == 2 and c['cin'] in (16, 64))


# ------------------------------------------------------------------ the restated host rules against the library

def _sweep_shapes():
    sizes = [(1, 1), (2, 2), (4, 4), (5, 7), (8, 4), (4, 8), (6, 6), (8, 8), (12, 12), (15, 15), (16, 16), (16, 32), (32, 16), (24, 24), (32, 32),
             (48, 48), (64, 64), (3, 250), (2, 300), (2, 381), (2, 382), (2, 500), (2, 512), (2, 637), (2, 638), (2, 700), (2, 701), (2, 702),
             (2, 765), (8, 96), (4, 128), (8, 128), (8, 192), (16, 128), (7, 128), (128, 128), (255, 255), (256, 256), (8, 512), (16, 1024)]
    batches = (1, 2, 3, 5, 16, 17, 31, 32, 33, 64, 255, 256, 257, 260)
    chans = ((16, 64), (16, 32), (16, 96), (16, 128), (32, 256), (64, 64), (112, 64), (512, 512), (8, 64), (24, 64), (16, 48), (16, 16), (64, 192),
             (128, 160), (1024, 128))
    return itertools.product(batches, chans, sizes, (P3, U3, D3))


def test_restated_split_rules_are_the_librarys():
    lib = _lib()
    n = 0
    for B, (cin, cout), (H, W), mode in _sweep_shapes():
        a = (B, cin, cout, H, W, mode)
        assert Q.split_supported(*a) == lib.sgdfr_modconv2d_split_supported(*a), a
        assert Q.split_f8_ok(*a) == lib.sgdfr_modconv2d_split_f8_ok(*a), a
        assert Q.ksplit_hint(*a) == lib.sgdfr_modconv2d_split_ksplit_hint(*a), a
        assert Q.xin_supported(*a) == lib.sgdfr_modconv2d_split_xin_supported(*a), a
        assert Q.cout_tiles(*a) == lib.sgdfr_modconv2d_split_cout_tiles(*a), a
        assert Q.cout_tiles(*a, xin_whole=True) == lib.sgdfr_modconv2d_split_cout_tiles_xin(*a), a
        for xin in (0, 1):      # cfg, NEX, simgs, the half tile: what the other queries cannot tell apart (cfg 6 from cfg 0)
            assert Q.plan_info(*a, xin_whole=bool(xin)) == lib.sgdfr_modconv2d_split_plan_info(*a, xin), (a, xin)
        n += 1
    assert n > 10000, n
    # every width of the flat space at H = 2, both channel widths: the boundaries below are not between two sweep points
    for W in range(1, 800):
        for cout in (64, 128):
            for mode in (U3, D3):
                a = (2, 16, cout, 2, W, mode)
                assert Q.split_supported(*a) == lib.sgdfr_modconv2d_split_supported(*a), a
                assert Q.xin_supported(*a) == lib.sgdfr_modconv2d_split_xin_supported(*a), a
                assert Q.plan_info(*a) == lib.sgdfr_modconv2d_split_plan_info(*a, 0), a


def test_restated_winograd_rules_are_the_librarys():
    lib = _lib()
    n = 0
    for B, cin, cout, H, W, f in itertools.product((1, 2, 3, 32, 64, 260), (16, 32, 48, 64, 96, 8, 24), (128, 256, 64, 192),
                                                   (1, 4, 8, 15, 16, 32, 64, 128), (8, 12, 14, 16, 18, 20, 24, 32, 48, 64, 96, 128, 256), (2, 4)):
        assert Q.wsplit_supported(B, cin, cout, H, W, f) == lib.sgdfr_modconv2d_wsplit_supported(B, cin, cout, H, W, f), (B, cin, cout, H, W, f)
        if f == 4:
            assert Q.wsplit_wide(B, cin, cout, H, W) == lib.sgdfr_modconv2d_wsplit_wide(B, cin, cout, H, W), (B, cin, cout, H, W)
        n += 1
    assert n > 10000, n
    assert any(Q.wsplit_wide(B, 64, 128, 64, 64) for B in (32, 64, 260)) and not Q.wsplit_wide(1, 64, 128, 16, 32)


# ------------------------------------------------------------------ boundaries, from both sides

def _last_first(fn, values):
    ok = [v for v in values if fn(v)]
    return max(ok), min(v for v in values if v > max(ok) and not fn(v))


def test_support_boundaries_from_both_sides():
    lib = _lib()
    sup, xin, wsp = lib.sgdfr_modconv2d_split_supported, lib.sgdfr_modconv2d_split_xin_supported, lib.sgdfr_modconv2d_wsplit_supported
    widths = range(1, 1200)
    found = {}
    # UP3 / DOWN3 widths at H = 2, with and without a pre-split input (fp32 input: supported; pre-split: xin_supported)
    found['UP3 Cin 16'] = _last_first(lambda W: sup(1, 16, 64, 2, W, U3), widths)
    found['UP3 Cin 16, Cout 128'] = _last_first(lambda W: sup(1, 16, 128, 2, W, U3), widths)
    found['UP3 Cin 512'] = _last_first(lambda W: sup(1, 512, 64, 2, W, U3), widths)
    found['UP3 pre-split Cin 16'] = _last_first(lambda W: xin(1, 16, 64, 2, W, U3), widths)
    found['UP3 pre-split Cin 512'] = _last_first(lambda W: xin(1, 512, 64, 2, W, U3), widths)
    found['DOWN3 C 16'] = _last_first(lambda W: sup(2, 16, 128, 2, W, D3), widths)
    found['DOWN3 pre-split C 16'] = _last_first(lambda W: xin(2, 16, 128, 2, W, D3), widths)
    found['DOWN3 C 512'] = _last_first(lambda W: sup(2, 512, 128, 2, W, D3), widths)
    for k, v in found.items():
        print('boundary %-24s last accepted W = %d, first refused W = %d' % (k, *v))
    assert found['UP3 Cin 16'] == (701, 702) and found['UP3 Cin 16, Cout 128'] == (701, 702) and found['UP3 pre-split Cin 16'] == (637, 638)
    assert found['DOWN3 C 16'] == (381, 382) and found['DOWN3 pre-split C 16'] == (381, 382)
    assert found['UP3 Cin 512'] == (701, 702) and found['UP3 pre-split Cin 512'] == (573, 574) and found['DOWN3 C 512'] == (381, 382)
    for k, v in found.items():
        assert v[1] == v[0] + 1, k                                  # no hole below the boundary
    # ... and every one of them is where the restatement puts it, and in the GPU lists
    assert Q.split_supported(1, 16, 64, 2, 701, U3) and not Q.split_supported(1, 16, 64, 2, 702, U3)
    ids = {(c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W']) for c in Q.all_direct_cases()}
    for want in ((U3, 1, 16, 64, 2, 701), (U3, 1, 16, 64, 2, 637), (U3, 1, 16, 64, 2, 700), (D3, 2, 16, 128, 2, 381), (D3, 2, 16, 128, 2, 300)):
        assert want in ids, want
    assert (1, 16, 64, 2, 702) in Q.UP_REFUSED and (2, 16, 128, 2, 382) in Q.DOWN_REFUSED and (1, 16, 64, 2, 638) in Q.UP_XIN_REFUSED
    # PLAIN3: the widths and heights of the patch rule, the whole-rows / whole-images rule, channel divisibility
    for ok, bad in Q.PLAIN_LAST:
        assert sup(*ok, P3) == 1 and sup(*bad, P3) == 0, (ok, bad)
        assert ok in {(c['B'], c['cin'], c['cout'], c['H'], c['W']) for c in Q.PLAIN_CASES}, ok
    for a in Q.PLAIN_REFUSED:
        assert sup(*a, P3) == 0 and Q.split_supported(*a, P3) == 0, a
    for a in Q.UP_REFUSED:
        assert sup(*a, U3) == 0, a
    for a in Q.UP_XIN_REFUSED:
        assert sup(*a, U3) == 1 and xin(*a, U3) == 0, a
    for a in Q.DOWN_REFUSED:
        assert sup(*a, D3) == 0, a
    assert [n for n in (4, 6, 8, 12, 16, 24, 32, 48, 64) if sup(1, 16, 64, n, n, P3)] == [4, 8, 16, 32, 64]
    assert [W for W in range(64, 400, 32) if sup(1, 16, 64, 8, W, P3)] == [64, 128, 192, 256, 320, 384]
    assert [H for H in range(1, 33) if sup(1, 16, 64, H, 128, P3)] == [8, 16, 24, 32] and [H for H in range(1, 17) if sup(1, 16, 128, H, 128, P3)] == [4, 8, 12, 16]
    assert [c for c in range(16, 257, 16) if sup(1, 16, c, 4, 4, P3)] == [32, 64, 96, 128, 160, 192, 224, 256]
    assert [c for c in range(16, 513, 16) if sup(1, 16, c, 4, 4, D3)] == [128, 256, 384, 512]
    assert [c for c in range(4, 65, 4) if sup(1, c, 64, 4, 4, P3)] == [16, 32, 48, 64]
    # the Winograd forms: W >= 16, W / f a multiple of the patch width, H a multiple of the patch height
    for ok, bad in Q.WSPLIT_LAST:
        assert wsp(*ok) == 1 and wsp(*bad) == 0, (ok, bad)
    for a in Q.WSPLIT_REFUSED:
        assert wsp(*a) == 0 and Q.wsplit_supported(*a) == 0, a
    assert [W for W in range(2, 70, 2) if wsp(1, 16, 128, 16, W, 2)] == [16, 32, 64] and [W for W in range(4, 70, 4) if wsp(1, 16, 128, 16, W, 4)] == [16, 32, 64]
    assert [H for H in range(1, 33) if wsp(1, 16, 128, H, 32, 2)] == [8, 16, 24, 32] and [H for H in range(1, 33) if wsp(1, 16, 128, H, 16, 4)] == [16, 32]
    assert [c for c in range(32, 300, 32) if wsp(1, 16, c, 16, 16, 2)] == [128, 256] and [c for c in range(8, 50, 8) if wsp(1, c, 128, 16, 16, 2)] == [16, 32, 48]


# ------------------------------------------------------------------ the case lists reach what they claim

def _facts(c, xin, ksplit=None, up_tail=None):
    ks = Q.ksplit_hint(c['B'], c['cin'], c['cout'], c['H'], c['W'], c['mode']) if ksplit is None else ksplit
    if c['mode'] == D3:
        ks = 1
    return Q.launch_facts(c['B'], c['cin'], c['cout'], c['H'], c['W'], c['mode'], xin=xin, ksplit=ks, up_tail=up_tail)


def launches_of(c):
    """The launches the GPU module makes of a direct case: [(label, facts)] -- fp32 input with the hinted K slices, and a pre-split
    input without slices where the library allows it (DOWN3: only that)."""
    a = (c['B'], c['cin'], c['cout'], c['H'], c['W'], c['mode'])
    out = []
    if c['mode'] != D3:
        out.append(('fp32', _facts(c, False)))
    if Q.xin_supported(*a) and not c['bcast']:
        out.append(('xin', _facts(c, True, ksplit=1)))
    return out


def test_the_case_lists_reach_every_plan_geometry_slot_count_and_slice_class():
    reach = {}

    def note(key, c, label):
        reach.setdefault(key, '%s [%s]' % (Q.case_id(c), label))
    for c in Q.all_direct_cases():
        a = (c['B'], c['cin'], c['cout'], c['H'], c['W'], c['mode'])
        assert Q.split_supported(*a), Q.case_id(c)
        for label, g in launches_of(c):
            p = g['plan']
            note(('plan', p.cfg, label), c, label)
            note(('geometry', g['kind'] + ('/TC%d' % g['TC'] if g['kind'] == 'patch' else '') + ('/ragged' if g['ragged'] else '')), c, label)
            note(('NEX', c['mode'], g['NEX']), c, label)
            note(('simgs', '<= 2' if g['simgs'] <= 2 else '> 2', c['mode']), c, label)
            if g['half']:
                note(('half cout tile', c['mode'], g['n_cout_tiles'] > 1), c, label)
            ks = g['ksplit']
            note(('ksplit', 1 if ks == 1 else 2 if ks == 2 else 16 if ks == 16 else 'odd', c['mode'] if ks > 1 else None), c, label)
            if ks > 1 and ks == (c['cin'] // 16) // 2:
                note(('ksplit cap Cin/16/2 binds', ks), c, label)
            note(('persistent' if g['persistent'] else 'one block per tile', c['mode']), c, label)
            if p.cfg in (4, 5):
                t = g['tail_round']
                key = 'taken' if t else ('n_full = 0' if g['n_full'] == 0 else 'tail = 0' if g['tail'] == 0 else 'tail > 128' if g['tail'] > 128 else 'other')
                note(('tail round', p.cfg, key, g['tail'] if t or g['tail'] > 128 else None), c, label)
    for k in sorted(reach, key=str):
        print('reached %-60s by %s' % (' '.join(str(v) for v in k if v is not None), reach[k]))
    plans = {(k[1], k[2]) for k in reach if k[0] == 'plan'}
    assert plans >= {(0, 'fp32'), (0, 'xin'), (1, 'fp32'), (1, 'xin'), (2, 'fp32'), (3, 'fp32'), (3, 'xin'), (4, 'fp32'), (4, 'xin'), (5, 'xin'),
                     (6, 'xin'), (8, 'xin')}, plans
    assert not any(k[0] == 'plan' and (k[1], k[2]) in ((2, 'xin'), (6, 'fp32'), (8, 'fp32'), (5, 'fp32')) for k in reach)       # launch_plan has no such form
    geo = {k[1] for k in reach if k[0] == 'geometry'}
    assert geo >= {'rows', 'images', 'images/ragged', 'patch/TC64', 'patch/TC32', 'flat', 'flat/ragged'}, geo
    nex = {(k[1], k[2]) for k in reach if k[0] == 'NEX'}
    # every slot count a supported shape can reach, per mode: swept over the shapes of the restatement test
    reachable = set()
    for B, (cin, cout), (H, W), mode in _sweep_shapes():
        for xin in (False, True):
            g = Q.split_plan(B, cin, cout, H, W, mode, xin)
            if g is not None:
                reachable.add((mode, g['NEX']))
    print('reachable (mode, NEX):', sorted(reachable))
    assert nex == reachable == {(P3, 2), (P3, 3), (P3, 4), (U3, 2), (U3, 3), (U3, 4), (D3, 2), (D3, 3)}, (nex, reachable)
    assert {k[1:] for k in reach if k[0] == 'simgs'} >= {('<= 2', P3), ('> 2', P3), ('<= 2', U3), ('> 2', U3), ('<= 2', D3), ('> 2', D3)}
    assert {k[1:] for k in reach if k[0] == 'half cout tile'} >= {(P3, False), (P3, True), (U3, False), (U3, True)}
    ks = {k[1] for k in reach if k[0] == 'ksplit'}
    assert ks == {1, 2, 'odd', 16}, ks
    assert {k[1] for k in reach if k[0] == 'ksplit cap Cin/16/2 binds'} >= {2, 3, 16}
    assert ('persistent', P3) in reach and ('one block per tile', P3) in reach and ('one block per tile', U3) in reach
    tails = {k[1:] for k in reach if k[0] == 'tail round'}
    assert tails >= {(4, 'taken', 1), (4, 'taken', 128), (4, 'tail > 128', 129), (4, 'tail = 0', None), (5, 'n_full = 0', None), (5, 'taken', 2)}, tails
    # the transposed conv's deep plan always has a whole round: big means >= 256 tiles (n_full = 0 is reached by DOWN3 only)
    for B, (cin, cout), (H, W), mode in _sweep_shapes():
        if mode == U3:
            g = Q.split_plan(B, cin, cout, H, W, mode)
            assert g is None or g['plan'].cfg != 4 or g['n_pix_tiles'] * g['n_cout_tiles'] >= 256
    # the uneven slices: 7 channel blocks over 3 slices
    assert Q.ksplit_hint(1, 112, 64, 4, 4, P3) == 3 and [7 * k // 3 for k in range(4)] == [0, 2, 4, 7]
    assert Q.ksplit_hint(1, 512, 512, 4, 4, P3) == 16 and Q.ksplit_hint(1, 64, 64, 4, 4, P3) == 2
    # the tail round's own geometry (128-wide tiles) stays inside the staging the kernel has: NI = 1 launches take NEX from xs
    for c in Q.UP_CASES + Q.DOWN_CASES:
        for label, g in launches_of(c):
            if g['tail_round']:
                t = g['tail_round']
                assert t['count'] > 0 and t['lid0'] >= 0 and (2 * t['xs'] + 511) // 512 <= (3 if c['mode'] == D3 else 4), Q.case_id(c)
                if c['mode'] == D3 and g['n_cout_tiles'] == 1:      # the tail tiles store something: not the padding row of the grid alone
                    first = t['n_full'] * 256
                    assert any((q % g['rps']) // g['P'] < c['H'] and (q % g['rps']) % g['P'] < c['W'] for q in range(first, g['total_pix'])), Q.case_id(c)


def test_the_winograd_case_list_reaches_every_tile_form():
    seen = set()
    for c in Q.WSPLIT_CASES:
        g = Q.wsplit_geometry(c['B'], c['cin'], c['cout'], c['H'], c['W'], c['f'])
        assert g is not None, Q.case_id(c)
        wide = c['wide']
        if wide:
            assert c['f'] == 4 and Q.wswide_plan(g, 2) is not None and c['cin'] % 32 == 0       # reached with SGDFR_WSPLIT_WIDE_NOW = 2
        else:
            assert Q.wswide_plan(g, 1) is None                                                   # by tile count: the 64-tile kernel
        seen.add((c['f'], 'wide' if wide else 'TCT %d' % g['TCT'], 'odd' if (c['cin'] // 16) % 2 else 'even'))
        print('reached F(%d,3) %-7s %s channel blocks by %s' % (c['f'], 'wide' if wide else 'TCT %d' % g['TCT'], 'odd' if (c['cin'] // 16) % 2 else 'even', Q.case_id(c)))
    assert {(f, t) for f, t, _ in seen} == {(2, 'TCT 8'), (2, 'TCT 16'), (4, 'TCT 4'), (4, 'TCT 8'), (4, 'wide')}
    for f in (2, 4):
        assert {par for ff, t, par in seen if ff == f and t != 'wide'} == {'odd', 'even'}
    assert Q.wswide_plan(Q.wsplit_geometry(1, 64, 128, 16, 32, 4), 2)['total_blocks'] == 1          # the wide kernel's smallest legal shape
    assert Q.wswide_plan(Q.wsplit_geometry(1, 48, 128, 16, 32, 4), 2) is None and Q.wswide_plan(Q.wsplit_geometry(1, 64, 128, 16, 16, 4), 2) is None

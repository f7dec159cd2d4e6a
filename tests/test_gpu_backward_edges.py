"""The bandwidth-bound backward helpers (csrc/backward.hip, blur_adjoint_split_kernel of csrc/upfirdn2d.hip) at their chunk, tile,
path and grid-stride edges, each kernel against its own plain fp64 reference (tests/backward_refs.py, itself checked on the CPU by
tests/test_cpu_backward_edges.py, which also proves that the case lists cross every edge from both sides).

Two kinds of check (backward_refs.py): EXACT on small integers with gain 2, slope 1/4, power-of-two scales and integer FIRs (every
partial sum below 2^24 of its unit: torch.equal with fp32(fp64 reference), every word of every output, whatever the order of the
atomics) and BOUNDED on synthetic.counter_tensor inputs with the production gain and slope, error / bound <= 1 and no error under a
zero bound.  Every test prints its worst ratio on a line starting with "backward-edges" (pytest -s); the bars are derived, never
fitted.

group                 bar
F.act_grad_reduce     exact; g_pre (K 1, c 2: slope, gain); sums (K = wave depth: ceil(min(HW, 2048) / 64) + 6 + chunks - 1; c = 3, the
                      third 10: + 1/gain, out * that, noise_w * noise, two subtractions); absmax words == bits of g_pre.abs().amax((2, 3))
                      with no word, the adjacent word and a word of its own (second memset)
F.grad_join           exact; g_pre (K = 1 + 3 + 1 added terms, c 4: rgb_scale, s_rgb, slope, gain); sums as above with c = K + 4 (+ 7);
                      r_next, r_rgb (K = wave depth, c 0); absmax words; untouched: r_next / r_rgb without their term, sums[..., 2]
                      without want_y in a caller's workspace; a view one float into its storage == the aligned call's g_pre
F.scale_reduce        exact; dx (K 1, c 0), r (K = wave depth)
F.torgb_bwd           exact at Cin 1, 4, 64; dx (K 3, c 2: scale, s), r (K = wave depth)
F.prepack_t           == fp32(w * fp32(1 / sqrtf(Cin k k))) in the transposed layout bit for bit; exact against fp64 for k = 1, Cin 4, 16, 64
F.blur_adjoint        exact with both integer FIRs (padding row and column 0); gT (K 16, c 0); asum (K = 16 + 24 + 6 + strips of a plane:
                      one atomic per strip, the per-lane path)
F.blur_adjoint_split  exact: hi + lo == fp64 gT d; bounded: the blur bound |d| + 2^-24 |v| + the form's step (bf16x3 2^-16 |v|, fp16x3
                      2^-22 |v| + 2^-20); asum as above; the saturation word stays 0; C % 8 != 0 and a misaligned xs raise

Measured on an MI355X (worst error / bound over the cases of each group; the exact checks are bit for bit and have no figure):
F.act_grad_reduce     0.547
F.grad_join           scalar kernel 0.463, float4 kernel 0.462, rgb kernel 0.523
F.scale_reduce        0.997 (dx is one rounding against a bound of one half-ulp: the bar is met with nothing to spare, by construction)
F.torgb_bwd           0.577
F.blur_adjoint        0.182
F.blur_adjoint_split  QC 32 0.466, QC 32 with column W 0.463, QC 64 0.468, QC 64 with column W 0.467
No kernel failed a check.  The whole file (181 cases) runs in 4.5 s; the slowest case takes 0.8 s (the first launch), the
grid-stride cases 0.2 s each.

Where the bars differ from a bare K: the sums carry their terms' own roundings as c (3, or K + 4 after grad_join, and 7 more for the
y sum); the exact grad_join inputs lie in [-2, 2] (with [-8, 8] the y sum of a 4100-element plane would pass 2^24); the blur_adjoint
grid-stride case is 4065 planes at (H, W) = (1, 519), so that the last wave of the second pass keeps 8 lanes whose other 56 took the
wave-sum path in the first pass (at 4352 planes of (1, 512) that wave straddles two planes in the first pass).

Bite check (scratch builds, nothing committed; each fails the named tests and no other group): the last float4 row of a chunk dropped
in grad_join_rgb_kernel (p + 4 >= hi) fails 35 (test_grad_join_paths 31: every rgb-path case; test_grad_join_term_subsets 4: the rgb
and gu+rgb subsets at HW 2052); its channel break one early (c + 1 >= C) the same 35; hi one short in act_grad_reduce_kernel fails
test_act_grad_reduce 17 (every case with HW >= 2048); the padding rule 2 bb + px > 2 W turned >= fails test_blur_adjoint 6 and
test_blur_adjoint_grid_stride; the full-wave guard of blur_adjoint_kernel's asum removed fails test_blur_adjoint[4, 5, 8] and
test_blur_adjoint_grid_stride; the `two` branch of blur_adjoint_split_kernel disabled fails test_blur_adjoint_split[32, 64, 128] and
both test_blur_adjoint_split_grid_stride cases.  grad_join_kernel<4> forced on a one-float-offset view was judged by reading and not
run: its float4 loads stay inside the buffers, and the hardware serves unaligned global loads, so it would return the same words; the
alignment clause of grad_join_path is therefore shown only by the restatement, the other clauses (HW % 4, HW >= 1024, g_rgb, g_add)
by the two rgb mutations, which fail exactly the cases that join_path() sends to the rgb kernel and the two offset-view cases whose
aligned comparison call runs on it.
"""
import numpy as np
import pytest
import torch

import backward_refs as R
from util import O, S  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EX = dict(slope=R.SLOPE, gain=R.GAIN)


def _F():
    from stylegan_directions_face_reenactment_amd import functional as F_
    return F_


def _N():
    from stylegan_directions_face_reenactment_amd import _native as N
    return N


def _say(what, **figures):
    print('backward-edges %-52s %s' % (what, '  '.join('%s %.3g' % kv for kv in figures.items())))


def _dev(i):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in i.items()}


def _eq(y, ref64):
    return y.dtype == torch.float32 and y.shape == ref64.shape and torch.equal(y, ref64.float().to(y.device))


def _ratio(y, ref, bound):
    err = (y.double() - ref).abs()
    assert y.shape == ref.shape and bool((err[bound == 0] == 0).all()), 'error under a zero bound'
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


def _off(t):
    """The same values as a contiguous view that starts one float into its storage."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _words(g_pre):
    return g_pre.abs().amax((2, 3)).view(torch.int32)


# ------------------------------------------------------------------ act_grad_reduce

def _act_raw(i, want_y, slope, gain):
    """sgdfr_act_grad_reduce_f32 itself with a word per plane that does NOT follow the sums (gap of 8 floats): the second memset."""
    N = _N()
    B, C, _, HW = i['out'].shape
    n = B * C
    buf = torch.full((n * 4 + 8,), 99.0, device=DEV)
    sums, gmax = buf[:n * 3].view(B, C, 3), buf[n * 3 + 8:].view(torch.int32).view(B, C)
    g_pre = torch.empty_like(i['out'])
    nz = i['noise']
    N.call('sgdfr_act_grad_reduce_f32', N.ptr(i['g']), N.ptr(i['out']), N.ptr(nz), 0 if nz is None or nz.shape[0] == 1 else HW,
           N.ptr(i['noise_w']) if nz is not None else None, N.ptr(i['bias']), N.ptr(g_pre), N.ptr(sums), B, C, HW, float(slope), float(gain),
           int(want_y), N.ptr(gmax), N.stream())
    assert bool((buf[n * 3:n * 3 + 8] == 99.0).all()), 'the gap between the sums and the words was written'
    return g_pre, sums, gmax


@pytest.mark.parametrize('B,C,HW,noise,bias,want_y', R.ACT_CASES)
def test_act_grad_reduce(B, C, HW, noise, bias, want_y):
    F_ = _F()
    worst = 0.0
    for kind, kw in (('exact', EX), ('real', dict(slope=0.2, gain=2 ** 0.5))):
        i = _dev(R.act_inputs(kind, B, C, HW, noise, bias))
        ref = R.act_grad_ref(i['g'], i['out'], i['noise'], i['noise_w'], i['bias'], want_y=want_y, **kw)
        runs = [F_.act_grad_reduce(i['g'], i['out'], i['noise'], i['noise_w'], i['bias'], want_y, **kw) + (None,),
                F_.act_grad_reduce(i['g'], i['out'], i['noise'], i['noise_w'], i['bias'], want_y, want_absmax=True, **kw),
                _act_raw(i, want_y, **kw)]
        for g_pre, sums, gmax in runs:
            assert g_pre.shape == i['out'].shape and sums.shape == (B, C, 3)
            if gmax is not None:
                assert torch.equal(gmax, _words(g_pre)), (kind, 'absmax words')
            if kind == 'exact':
                assert R.act_exact_condition(HW) and _eq(g_pre, ref['g_pre']) and _eq(sums, ref['sums']), (kind, B, C, HW)
            else:
                worst = max(worst, _ratio(g_pre, ref['g_pre'], ref['b_pre']), _ratio(sums, ref['sums'], ref['b_sums']))
    _say('act_grad_reduce B%d C%d HW%d %s' % (B, C, HW, noise), ratio=worst)
    assert worst <= 1.0


# ------------------------------------------------------------------ grad_join

SENTINEL = 7.0


def _join_call(F_, c, i, kw, off=None):
    """F.grad_join of a case; with c['work'] the buffers are carved from a zeroed workspace five floats into its storage, and what
    the kernel must not touch carries a sentinel.  Returns (the wrapper's tuple, the workspace or None)."""
    B, C, HW = c['B'], c['C'], c['HW']
    n = B * C
    a = dict(i)
    if off:
        a[off] = _off(a[off])
    work = None
    if c['work']:
        work = torch.zeros(n * 8 + 5, device=DEV)[5:]
        if 'gu' not in c['terms']:
            work[n * 4:n * 5] = SENTINEL
        if 'rgb' not in c['terms']:
            work[n * 5:] = SENTINEL
        if not c['want_y']:
            work[2:n * 3:3] = SENTINEL
    got = F_.grad_join(a['out'], a['gu'], a['s_next'], a['g_rgb'], a['w_rgb'], a['s_rgb'], a['g_add'], a['noise'], a['noise_w'], a['bias'],
                       want_y=c['want_y'], work=work, **kw)
    return got, work


def _join_check(c, kind, got, work, ref, tag):
    """Every output of one grad_join call; returns the worst ratio (0 for the exact kind)."""
    g_pre, sums, gmax, r_next, r_rgb = got
    B, C, n = c['B'], c['C'], c['B'] * c['C']
    assert g_pre.shape == (B, C, 1, c['HW']) and sums.shape == (B, C, 3) and gmax.shape == (B, C) and gmax.dtype == torch.int32
    assert torch.equal(gmax, _words(g_pre)), (tag, 'absmax words')
    assert (r_next is None) == ('gu' not in c['terms']) and (r_rgb is None) == ('rgb' not in c['terms'])
    third = sums[..., 2]
    if not c['want_y']:
        assert bool((third == (SENTINEL if work is not None else 0.0)).all()), (tag, 'sums[..., 2] without want_y')
    if work is not None:
        assert r_next is not None or bool((work[n * 4:n * 5] == SENTINEL).all()), (tag, 'r_next without gu')
        assert r_rgb is not None or bool((work[n * 5:] == SENTINEL).all()), (tag, 'r_rgb without g_rgb')
    k3 = 3 if c['want_y'] else 2
    if kind == 'exact':
        assert _eq(g_pre, ref['g_pre']), (tag, 'g_pre', float((g_pre.double() - ref['g_pre']).abs().max()))
        assert _eq(sums[..., :k3], ref['sums'][..., :k3]), (tag, 'sums')
        assert r_next is None or _eq(r_next, ref['r_next']), (tag, 'r_next')
        assert r_rgb is None or _eq(r_rgb, ref['r_rgb']), (tag, 'r_rgb')
        return 0.0
    worst = max(_ratio(g_pre, ref['g_pre'], ref['b_pre']), _ratio(sums[..., :k3], ref['sums'][..., :k3], ref['b_sums'][..., :k3]))
    if r_next is not None:
        worst = max(worst, _ratio(r_next, ref['r_next'], ref['b_next']))
    if r_rgb is not None:
        worst = max(worst, _ratio(r_rgb, ref['r_rgb'], ref['b_rgb']))
    return worst


def _join_case(c):
    F_ = _F()
    worst = 0.0
    for kind, kw in (('exact', EX), ('real', dict(slope=0.2, gain=2 ** 0.5))):
        if not c[kind]:
            continue
        assert kind != 'exact' or R.join_exact_condition(c['C'], c['HW'])
        i = _dev(R.join_inputs(kind, c['B'], c['C'], c['HW'], c['terms'], c['noise'], c['bias']))
        ref = R.grad_join_ref(want_y=c['want_y'], **i, **kw)
        tag = '%s %s %s' % (R.join_id(c), kind, R.join_path(c))
        got, work = _join_call(F_, c, i, kw, c['off'])
        worst = max(worst, _join_check(c, kind, got, work, ref, tag))
        if c['off']:                  # the scalar kernel forms g_pre by the float4 kernels' expressions: the same words
            aligned, _ = _join_call(F_, c, i, kw)
            assert torch.equal(got[0], aligned[0]) and torch.equal(got[2], aligned[2]), (tag, 'g_pre of the offset view')
    _say('grad_join %s %s' % (R.join_id(c), R.join_path(c)), ratio=worst)
    assert worst <= 1.0, (R.join_id(c), worst)


@pytest.mark.parametrize('c', R.JOIN_SUBSET_CASES, ids=R.join_id)
def test_grad_join_term_subsets(c):
    """All seven non-empty subsets of {gu, g_rgb, g_add} on the scalar and on a float4 kernel, buffers allocated by the wrapper and
    carved from a caller's zeroed workspace (zero_outputs = 0)."""
    _join_case(c)


@pytest.mark.parametrize('c', R.JOIN_CHUNK_CASES, ids=R.join_id)
def test_grad_join_chunk_edges(c):
    _join_case(c)


@pytest.mark.parametrize('c', R.JOIN_PATH_CASES, ids=R.join_id)
def test_grad_join_paths(c):
    """The rgb kernel on both sides of HW >= 1024, at channel counts that are no multiple of its four channels per wave and at
    last chunks that end inside a float4 row; what must leave it (g_add, an offset view, HW % 4 != 0) and still be right."""
    _join_case(c)


# ------------------------------------------------------------------ scale_reduce, torgb_bwd

@pytest.mark.parametrize('B,C,HW,bcast', R.SCALE_CASES)
def test_scale_reduce(B, C, HW, bcast):
    F_ = _F()
    worst = 0.0
    for kind in ('exact', 'real'):
        i = _dev(R.reduce_inputs(kind, 'scale', B, C, HW, bcast=bcast))
        ref = R.scale_reduce_ref(i['gu'], i['x'], i['s'])
        gu = i['gu'].clone()
        dx, r = F_.scale_reduce(gu, i['x'], i['s'])                      # dx aliases gu, as in the per-layer backward
        assert dx.data_ptr() == gu.data_ptr() and r.shape == (B, C) and (not bcast or i['x'].shape[0] == 1)
        if kind == 'exact':
            assert R.reduce_exact_condition(HW) and _eq(dx, ref['dx']) and _eq(r, ref['r']), (B, C, HW)
        else:
            worst = max(worst, _ratio(dx, ref['dx'], ref['b_dx']), _ratio(r, ref['r'], ref['b_r']))
    _say('scale_reduce B%d C%d HW%d%s' % (B, C, HW, ' bcast' if bcast else ''), ratio=worst)
    assert worst <= 1.0


@pytest.mark.parametrize('B,cin,HW', R.TORGB_BWD_CASES)
def test_torgb_bwd(B, cin, HW):
    F_ = _F()
    worst = 0.0
    for kind in ('exact', 'real'):
        if kind == 'exact' and not R.reduce_exact_condition(HW, cin):
            continue
        i = _dev(R.reduce_inputs(kind, 'torgb', B, cin, HW))
        ref = R.torgb_bwd_ref(i['x'], i['g'], i['w_rgb'], i['s'])
        dx, r = F_.torgb_bwd(i['x'], i['g'], i['w_rgb'], i['s'])
        assert r.shape == (B, 3, cin)
        if kind == 'exact':
            assert _eq(dx, ref['dx']) and _eq(r, ref['r']), (B, cin, HW)
        else:
            worst = max(worst, _ratio(dx, ref['dx'], ref['b_dx']), _ratio(r, ref['r'], ref['b_r']))
    _say('torgb_bwd B%d Cin%d HW%d' % (B, cin, HW), ratio=worst)
    assert worst <= 1.0


def test_an_empty_batch_returns_without_a_launch():
    """B = 0 through every wave-per-chunk entry with live, pre-filled output buffers: no memset, no kernel, no word changes."""
    N = _N()
    C, HW = 4, 65
    x = torch.full((2, C, 1, HW), 3.0, device=DEV)
    g3 = torch.full((2, 3, 1, HW), 3.0, device=DEV)
    s = torch.full((2, C), 2.0, device=DEV)
    w = torch.full((3, C), 2.0, device=DEV)
    outs = [torch.full((2 * C * 8 + 2 * C * HW,), 99.0, device=DEV) for _ in range(5)]
    o = [(b[:2 * C * HW], b[2 * C * HW:]) for b in outs]
    p, st = N.ptr, N.stream()
    N.call('sgdfr_act_grad_reduce_f32', p(x), p(x), None, 0, None, None, p(o[0][0]), p(o[0][1]), 0, C, HW, 0.2, 1.4, 1, p(o[0][1][3 * C:]), st)
    N.call('sgdfr_grad_join_f32', p(x), p(x), p(s), p(g3), p(w), p(s), p(x), None, 0, None, None, p(o[1][0]), p(o[1][1]), p(o[1][1][24:]),
           p(o[1][1][32:]), p(o[1][1][40:]), 0, C, HW, 0.2, 1.4, 1, 1, st)
    N.call('sgdfr_scale_reduce_f32', p(x), p(x), C * HW, p(s), p(o[2][0]), p(o[2][1]), 0, C, HW, st)
    N.call('sgdfr_torgb_bwd_f32', p(x), p(g3), p(w), p(s), p(o[3][0]), p(o[3][1]), 0, C, 1, HW, st)
    N.call('sgdfr_blur_adjoint_f32', p(x), p(w), p(x), p(o[4][0]), p(o[4][1]), 0, C, 1, 1, st)
    torch.cuda.synchronize()
    assert all(bool((b == 99.0).all()) for b in outs)


# ------------------------------------------------------------------ prepack_t

@pytest.mark.parametrize('cout,cin,k', R.PREPACK_T_CASES)
def test_prepack_t_bit_for_bit(cout, cin, k):
    F_ = _F()
    sc = np.float32(R.wscale32(cin * k * k))
    w = S.counter_tensor(19, 'pt.%d.%d.%d' % (cout, cin, k), (1, cout, cin, k, k))
    wi = R.ints(19, 'pti.%d.%d.%d' % (cout, cin, k), (1, cout, cin, k, k), -8, 8)
    for flip in (0, 1):
        wt = F_.prepack_t(w.to(DEV), flip).cpu()
        want = (R.prepack_t_ref(w[0], flip).float().numpy() * sc).astype(np.float32)           # fp32(w * fp32 scale), one rounding
        assert wt.shape == (cout, k * k, cin) and np.array_equal(wt.numpy(), want), (cout, cin, k, flip)
        if k == 1 and cin in (4, 16, 64):                                                       # a power-of-two scale: exact against fp64
            assert float(sc) * float(sc) * cin == 1.0
            assert _eq(F_.prepack_t(wi.to(DEV), flip).cpu(), R.prepack_t_ref(wi[0], flip) * float(sc))


# ------------------------------------------------------------------ blur_adjoint

def _blur_check(F_, i, fir, kind, with_planes):
    planes = i['planes'] if with_planes else None
    ref = R.blur_adjoint_ref(i['g'], fir, planes)
    gt, asum = F_.blur_adjoint(i['g'], fir, planes)
    assert (asum is None) == (planes is None)
    if kind == 'exact':
        assert _eq(gt, ref['gt']), ('gT', tuple(i['g'].shape), float((gt.double() - ref['gt']).abs().max()))
        assert asum is None or _eq(asum, ref['asum']), ('asum', tuple(i['g'].shape))
        return 0.0
    worst = _ratio(gt, ref['gt'], ref['b_gt'])
    return worst if asum is None else max(worst, _ratio(asum, ref['asum'], ref['b_asum']))


@pytest.mark.parametrize('H', R.BLUR_ADJ_H)
def test_blur_adjoint(H):
    """F.blur_adjoint over H != W, the strip tails (H + 1 over 4), tail waves (strips % 64 != 0) and waves across planes."""
    F_ = _F()
    worst = 0.0
    for n, W in enumerate(R.BLUR_ADJ_W):
        B, C = R.BLUR_ADJ_PLANES[(n + H) % 3]
        assert (H, W) != (2, 2) or B * C == 3
        for k, (fx, fr) in enumerate(zip(R.exact_firs(), R.real_firs())):
            for with_planes in (True, False):
                assert R.blur_exact_condition(H, W, fx)
                _blur_check(F_, _dev(R.blur_inputs('exact', B, C, H, W)), fx.to(DEV), 'exact', with_planes)
                worst = max(worst, _blur_check(F_, _dev(R.blur_inputs('real', B, C, H, W)), fr.to(DEV), 'real', with_planes))
    _say('blur_adjoint H=%d' % H, ratio=worst)
    assert worst <= 1.0


def test_blur_adjoint_grid_stride():
    """More strips than the 8192 x 256 threads of the capped grid (the 512 -> 1024 layer at B >= 2 does that): the kernel strides,
    and the second pass ends in a wave of 8 lanes whose other 56 took the wave-sum path in the first pass; exact, asum included.
    Inputs and reference stay on the device."""
    F_ = _F()
    B, C, H, W = R.BLUR_ADJ_STRIDE
    assert R.adjoint_strides(B * C, H, W) and R.adjoint_tail(B * C, H, W) == (8, True)
    fir = R.exact_firs()[1].to(DEV)
    assert R.blur_exact_condition(H, W, fir.cpu())
    _blur_check(F_, R.blur_inputs('exact', B, C, H, W, device=DEV), fir, 'exact', True)


# ------------------------------------------------------------------ blur_adjoint_split

def _split_check(F_, i, fir, kind, arith, with_d, with_planes, word):
    B, C, H2, W2 = i['g'].shape
    H, W = H2 // 2, W2 // 2
    planes, d = (i['planes'] if with_planes else None), (i['d'] if with_d else None)
    ref = i.get('ref') or R.blur_adjoint_ref(i['g'], fir, i['planes'])
    with F_.saturation_sink(word):
        xs, asum = F_.blur_adjoint_split(i['g'], fir, planes, d, arith)
    assert (asum is None) == (planes is None)
    dec = R.decode_split_planes(xs, B, C, H, W, arith)
    dd = d.double()[:, :, None, None, None] if d is not None else 1.0
    want = ref['gt'] * dd
    if kind == 'exact':
        assert torch.equal(dec, want), ('hi + lo', arith, (B, C, H, W), float((dec - want).abs().max()))
        assert asum is None or _eq(asum, ref['asum']), ('asum', arith, (B, C, H, W))
        return 0.0
    base = ref['b_gt'] * (dd.abs() if d is not None else 1.0)          # (the step is taken at the device's fp32 value: base (1 + 2^-15))
    worst = _ratio(dec, want, base * (1 + 2.0 ** -15) + R.split_step(want, arith) * (base > 0))
    return worst if asum is None else max(worst, _ratio(asum, ref['asum'], ref['b_asum']))


@pytest.mark.parametrize('W', R.SPLIT_W)
def test_blur_adjoint_split(W):
    """The fused adjoint against its OWN fp64 reference, through the decoded hi + lo: both column-tile widths, column W riding on the
    thread of column W - 1 or not, a second tile of two columns, one and two row tiles, both arithmetics, d and the planes given or not."""
    F_ = _F()
    worst = 0.0
    word = F_.new_saturation_word(DEV)
    for H in R.SPLIT_H:
        for C in (8, 24):
            B = 3 if C == 8 else 2
            for fx, fr in zip(R.exact_firs(), R.real_firs()):
                ix, ir = _dev(R.blur_inputs('exact', B, C, H, W)), _dev(R.blur_inputs('real', B, C, H, W))
                ix['ref'], ir['ref'] = R.blur_adjoint_ref(ix['g'], fx.to(DEV), ix['planes']), R.blur_adjoint_ref(ir['g'], fr.to(DEV), ir['planes'])
                assert R.blur_exact_condition(H, W, fx)
                for arith in ('bf16x3', 'fp16x3'):
                    for with_d, with_planes in ((True, True), (False, False), (True, False)):
                        _split_check(F_, ix, fx.to(DEV), 'exact', arith, with_d, with_planes, word)
                        worst = max(worst, _split_check(F_, ir, fr.to(DEV), 'real', arith, with_d, with_planes, word))
    assert int(word) == 0, 'saturation word'
    p = R.split_plan(2, 8, 4, W)
    _say('blur_adjoint_split W=%d QC%d%s' % (W, p['QC'], ' +column W' if p['extra'] else ''), ratio=worst)
    assert worst <= 1.0


@pytest.mark.parametrize('B,C,H,W', R.SPLIT_STRIDE)
def test_blur_adjoint_split_grid_stride(B, C, H, W):
    """More than 8192 tiles at each column-tile width: the tile loop strides; exact, asum included, on the device."""
    F_ = _F()
    assert R.split_plan(B, C, H, W)['strides']
    fir = R.exact_firs()[1].to(DEV)
    i = R.blur_inputs('exact', B, C, H, W, device=DEV)
    i['ref'] = R.blur_adjoint_ref(i['g'], fir, i['planes'])
    word = F_.new_saturation_word(DEV)
    for arith in ('bf16x3', 'fp16x3'):
        _split_check(F_, i, fir, 'exact', arith, True, True, word)
    assert int(word) == 0


def test_blur_adjoint_split_refusals():
    F_, N = _F(), _N()
    fir = R.real_firs()[0].to(DEV)
    with pytest.raises(RuntimeError, match='blur_adjoint_split'):
        F_.blur_adjoint_split(torch.zeros(2, 12, 4, 4, device=DEV), fir, None, None, 'bf16x3')
    B, C, H, W = 1, 8, 2, 2
    g = torch.zeros(B, C, 2 * H, 2 * W, device=DEV)
    buf = torch.zeros(B * 4 * C // 8 * 2 * (H + 1) * (W + 1) * 8 + 4, device=DEV, dtype=torch.int16)
    xs = buf[4:]
    assert xs.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError, match='misaligned'):
        N.call('sgdfr_blur_adjoint_split_f32', N.ptr(g), N.ptr(fir), None, None, N.ptr(xs), None, B, C, H, W, N.SPLIT_BF16, None, N.stream())
    assert bool((buf == 0).all())

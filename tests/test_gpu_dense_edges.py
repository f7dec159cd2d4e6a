"""The dense, style and pointwise kernels (csrc/linear.hip, csrc/elementwise.hip) at their dispatch edges, each against a plain fp64
reference (tests/dense_refs.py, itself checked on the CPU by tests/test_cpu_dense_edges.py).

Two kinds of check (dense_refs.py): EXACT on small integers (sums < 2^24: bit for bit whatever the summation order) and BOUNDED on
synthetic.counter_tensor inputs with the a-priori per-element bound (K + 8) * 2^-24 * (|x| @ |w|^T |wscale| + |bias| |bscale|).
Every test prints its worst error / bound ratio (or ulp distance) on a line starting with "dense-edges" (pytest -s); the bars are
derived, never fitted.

group                     bar
F.linear                  exact on integers; ratio <= 1 (after leaky-ReLU: bound * gain + 2^-23 |ref|); 51 shapes, 19 skinny, 32 tiled
F.style_demod             s: exact (D = 64, 256) / ratio <= 1; d: 4 ulp on integer arguments (one rounding of the argument, the
                          hardware rsqrt, one rounding of the result), relative 0.5 bound(acc)/acc + 4 * 2^-23 on real ones
F.styles_batched          as style_demod; every row == the same row alone at B = 1, bit for bit; views disjoint;
                          range plans: s_n, d_n == ldexp(s, e), ldexp(d, -e) by the host rule == F.split_range, bit for bit
F.demod_grad              exact on integers; ratio <= 1 (K = Cout)
F.styles_batched_bwd      exact on integers (D = 64, 256; rows without the 1/sqrt(516) ToRGB layer); ratio <= 1 with the ds bound
                          carried through the latent stage; the unread latent row == 0
F.demod_dq / param_grads  exact on integers; ratio <= 1 (B, resp. B*HW terms)
pixel_norm (+ gradient)   (D/64 + 16) * 2^-23 of max |ref| per row
F.affine                  exact on integers; ratio <= 1 for y, dx, dW, db
uint8 packing             == the numpy float32 evaluation, every byte, on the 1788 boundary probes
FusedAdam                 rtol 2e-6, atol 1e-7 against the fp64 restatement (4 steps, default lr)
F.absmax                  == the bit pattern of x.abs().amax()

Measured on an MI355X (worst over the cases of each group; error / bound unless said otherwise):
F.linear                  skinny 0.195, tiled 0.183 (host emulation of both accumulation orders, tests/test_cpu_dense_edges.py: 0.198)
F.style_demod             s 0.0135; d 0.0985 on real inputs; d on integer arguments 0.764 ulp of the 4 ulp bar
F.styles_batched          s 0.0191; d 0.147; d on integer arguments 0.801 ulp of the 4 ulp bar; range exponents from -4 to the +120 clamp
F.demod_grad              0.0405
F.styles_batched_bwd      latent gradient 0.00236; mod_w / mod_b gradients 0.288
F.demod_dq / param_grads  0.475
pixel_norm (+ gradient)   forward 0.0467 of its bar, gradient 0.0277 (host emulation of the gradient: 0.03)
F.affine                  0.193
FusedAdam                 0.10 of rtol 2e-6 / atol 1e-7 at the tensor limit, 0.097 with the alternating parameter (a per-parameter step
                          count would lie 3.9e3 bars away)
The exact checks, uint8 packing and F.absmax are bit for bit: they have no figure.
"""
import numpy as np
import pytest
import torch

import dense_refs as R
from util import S

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23


def _F():
    from stylegan_directions_face_reenactment_amd import functional as F_
    return F_


def _say(what, **figures):
    print('dense-edges %-34s %s' % (what, '  '.join('%s %.3g' % kv for kv in figures.items())))


def _exact(y, ref64):
    return torch.equal(y.detach().cpu(), ref64.float().cpu())


# ------------------------------------------------------------------ F.linear

LINEAR_CASES = [pytest.param(M, K, N, 'skinny' if (M <= 128 and K <= 512 and N >= 64) else 'tiled',
                             id='%dx%dx%d-%s' % (M, K, N, 'skinny' if (M <= 128 and K <= 512 and N >= 64) else 'tiled'))
                for M, K, N in R.linear_cases()]


def test_the_sweeps_cross_every_dispatch_edge():
    """Readable from the parametrisation: both linear kernels at >= 12 shapes, the chunk rule of sgdfr_styles_batched_f32 (4, 16, 64),
    SG_BU = 8 images per block and SG_MAXC = 512 channels per pass of the latent gradient, the 16384-element block split of the ToRGB
    bias gradient, the 1024-element chunks of the Adam launch."""
    sides = [p.values[3] for p in LINEAR_CASES]
    assert sides.count('skinny') >= 12 and sides.count('tiled') >= 12
    Bs = {c[0] for c in STYLES_CASES}
    for edge in (4, 16, 64):
        assert edge - 1 in Bs and edge in Bs and edge + 1 in Bs
    assert {7, 8, 9} <= set(BWD_B) and any(cin > 512 and cin % 512 % 4 == 0 for _, _, cin, _ in BWD_LAYERS)
    assert any(B * HW > 16384 for B in PG_B for HW in PG_HW) and any(B * HW <= 16384 for B in PG_B for HW in PG_HW)
    assert {1023, 1024, 1025} <= set(R.ADAM_SIZES)


@pytest.mark.parametrize('M,K,N,side', LINEAR_CASES)
def test_linear_exact_and_bounded(M, K, N, side):
    F_ = _F()
    assert (M <= 128 and K <= 512 and N >= 64) == (side == 'skinny')
    worst = 0.0
    # exact: integers in [-8, 8], wscale a power of two (64 * 515 < 2^24)
    x, w, b = R.linear_inputs('int', M, K, N)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    assert _exact(F_.linear(xg, wg, bg, wscale=0.5, bscale=2.0), R.linear_ref(x, w, b, 0.5, 2.0)[0])
    assert _exact(F_.linear(xg, wg), R.linear_ref(x, w)[0])
    lat = R.int_tensor(7, 'lin.lat%d.%d.%d' % (M, K, N), (M, 3 * K)).view(M, 3, K)
    assert _exact(F_.linear(lat.cuda()[:, 1], wg, bg, wscale=2.0), R.linear_ref(lat[:, 1], w, b, 2.0)[0])      # ldx = 3 K
    assert _exact(F_.linear(xg[-1:].expand(M, K), wg, bg), R.linear_ref(x[-1:].expand(M, K), w, b)[0])         # stride 0: copied
    # bounded: real inputs
    x, w, b = R.linear_inputs('real', M, K, N)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    for kw in (dict(wscale=0.3, bscale=2.0), dict(), dict(lrelu=True), dict(wscale=0.3, bscale=2.0, lrelu=True)):
        for bias in (b, None):
            y = F_.linear(xg, wg, bias.cuda() if bias is not None else None, **kw)
            assert y.shape == (M, N)
            worst = max(worst, R.ratio(y, *R.linear_ref(x, w, bias, **kw)))
    lat = S.counter_tensor(7, 'lin.rlat%d.%d.%d' % (M, K, N), (M, 3, K))
    worst = max(worst, R.ratio(F_.linear(lat.cuda()[:, 2], wg, bg, lrelu=True), *R.linear_ref(lat[:, 2], w, b, lrelu=True)))
    worst = max(worst, R.ratio(F_.linear(xg[:1].expand(M, K), wg, bg), *R.linear_ref(x[:1].expand(M, K), w, b)))
    _say('linear %dx%dx%d %s' % (M, K, N, side), ratio=worst)
    assert worst <= 1.0


def test_linear_refuses_a_wrong_feature_count():
    F_ = _F()
    with pytest.raises(RuntimeError):
        F_.linear(torch.zeros(3, 65).cuda(), torch.zeros(4, 64).cuda())
    with pytest.raises(RuntimeError):
        F_.linear(torch.zeros(3, 64), torch.zeros(4, 64).cuda())


# ------------------------------------------------------------------ F.style_demod

def _real_layer(key, D, cin, cout, seed=11):
    mw = S.counter_tensor(seed, key + '.mw', (cin, D))
    mb = S.counter_tensor(seed, key + '.mb', (cin,), 1.0, 0.1)
    q = (S.counter_tensor(seed, key + '.q', (cout, cin)).abs() + 0.1) if cout else None
    return mw, mb, q


def _int_layer(key, D, cin, cout, seed=11):
    return (R.int_tensor(seed, key + '.mw', (cin, D)), R.int_tensor(seed, key + '.mb', (cin, 1)).view(cin),
            R.int_tensor(seed, key + '.q', (cout, cin), 1, 4) if cout else None)


def _check_s_d(tag, mode, D, style, layer, s, d):
    """One layer's (s, d) from the device against fp64; returns (ratio of s, ratio of d, ulps of d)."""
    mw, mb, q = layer
    sref, sbound = R.style_ref(style, mw, mb, D)
    rs = rd = ul = 0.0
    if mode == 'real' or (mode == 'int' and not R.pow4(D)):       # 'struct' is exact at every D: one power-of-four entry or none
        rs = R.ratio(s, sref, sbound)
        assert rs <= 1.0, (tag, 's', rs)
    else:
        assert _exact(s, sref), (tag, 's')
    if q is not None:
        dref, drel = R.demod_ref(s, q)
        if mode == 'struct':                # integer argument >= 1: 4 ulp
            ul = R.ulps(d, dref)
            assert ul <= 4.0, (tag, 'd ulps', ul)
        else:
            rd = R.ratio(d, dref, dref * drel)
            assert rd <= 1.0, (tag, 'd', rd)
    else:
        assert d is None
    return rs, rd, ul


def _layer_inputs(mode, key, B, D, cin, cout):
    """(style [B,D], (mod_w, mod_b, q)) on the CPU for one layer: 'real' | 'int' (exact s where 1/sqrt(D) is a power of two) | 'struct'
    (integer s in [-4,4], integer q: exact argument of the rsqrt)."""
    if mode == 'real':
        return S.counter_tensor(11, key + '.st', (B, D)), _real_layer(key, D, cin, cout)
    if mode == 'int':
        return R.int_tensor(11, key + '.st', (B, D)), _int_layer(key, D, cin, cout)
    return R.int_tensor(11, key + '.st', (B, D), -2, 2), R.structured_style_layer(11, key, D, cin, cout)


@pytest.mark.parametrize('B,D,cin,cout', [(1, 512, 64, 64), (3, 512, 63, 130), (128, 256, 64, 48), (129, 256, 64, 48), (5, 200, 96, 70),
                                          (4, 64, 512, 512), (2, 512, 6, 3)])
def test_style_demod_edges(B, D, cin, cout):
    F_ = _F()
    fig = dict(s=0.0, d=0.0, ulps=0.0)
    for mode in ('real', 'int', 'struct'):
        key = 'sd.%s.%d.%d.%d.%d' % (mode, B, D, cin, cout)
        style, layer = _layer_inputs(mode, key, B, D, cin, cout)
        g = [t.cuda() for t in layer]
        s, d = F_.style_demod(style.cuda(), g[0], g[1], g[2], cout)
        assert s.shape == (B, cin) and d.shape == (B, cout)
        rs, rd, ul = _check_s_d(key, mode, D, style, layer, s, d)
        fig = dict(s=max(fig['s'], rs), d=max(fig['d'], rd), ulps=max(fig['ulps'], ul))
        s0, d0 = F_.style_demod(style.cuda(), g[0], g[1])                 # without q: the same s, no d
        assert d0 is None and torch.equal(s0, s)
        lat = torch.zeros(B, 3, D)
        lat[:, 1] = style
        lat[:, 0], lat[:, 2] = 77.0, -55.0
        s1, d1 = F_.style_demod(lat.cuda()[:, 1], g[0], g[1], g[2], cout)   # a strided row of a [B, L, D] latent
        assert torch.equal(s1, s) and torch.equal(d1, d)
    _say('style_demod B%d D%d %d->%d' % (B, D, cin, cout), **fig)


# ------------------------------------------------------------------ F.styles_batched

WIDTHS_FULL = [(6, 16), (10, 3), (64, 130), (130, 512), (512, 16), (512, 3), (64, 512), (130, 130)]      # cout 3: ToRGB, q = None
WIDTHS_SMALL = [(10, 16), (130, 3), (64, 130), (6, 512)]
# (B, D, L): every B on both sides of the chunk thresholds 4 / 16 / 64, every D, every L; the long list at the small batches
STYLES_CASES = [(1, 64, 1), (3, 256, 4), (4, 193, 18), (5, 512, 18), (15, 64, 4), (16, 512, 4), (17, 193, 1), (63, 256, 18), (64, 512, 4),
                (65, 64, 18)]


def _latent_rows(L, n):
    """Latent row per layer: repeated, out of order, the last row included."""
    order = [L - 1, 0, L // 2, L - 1, 1 % L, 0, L - 1, L // 2]
    return [order[i % len(order)] for i in range(n)]


def _styles_setup(mode, B, D, L):
    widths = WIDTHS_FULL if B <= 5 else WIDTHS_SMALL
    key = 'sb.%s.%d.%d.%d' % (mode, B, D, L)
    if mode == 'real':
        latent = S.counter_tensor(13, key + '.lat', (B, L, D))
    else:
        latent = R.int_tensor(13, key + '.lat', (B, L * D), *((-8, 8) if mode == 'int' else (-2, 2))).view(B, L, D)
    layers = []
    for i, ((cin, cout), li) in enumerate(zip(widths, _latent_rows(L, len(widths)))):
        rgb = cout == 3
        lk = '%s.%d' % (key, i)
        layer = {'real': _real_layer, 'int': _int_layer}[mode](lk, D, cin, 0 if rgb else cout) if mode != 'struct' else \
            R.structured_style_layer(13, lk, D, cin, 0 if rgb else cout)
        layers.append((li, layer, cout))
    return latent, layers


def _specs(layers):
    return [(li, mw.cuda(), mb.cuda(), q.cuda() if q is not None else None, cout) for li, (mw, mb, q), cout in layers]


@pytest.mark.parametrize('B,D,L', STYLES_CASES)
def test_styles_batched_values_views_and_chunk_independence(B, D, L):
    F_ = _F()
    fig = dict(s=0.0, d=0.0, ulps=0.0)
    for mode in ('real', 'int', 'struct'):
        latent, layers = _styles_setup(mode, B, D, L)
        specs = _specs(layers)
        lg = latent.cuda()
        outs = F_.styles_batched(lg, specs)
        assert len(outs) == len(layers)
        spans = []
        for i, ((li, layer, cout), (s, d)) in enumerate(zip(layers, outs)):
            assert s.shape == (B, layer[0].shape[0]) and (d is None) == (layer[2] is None)
            rs, rd, ul = _check_s_d('%s layer %d' % (mode, i), mode, D, latent[:, li], layer, s, d)
            fig = dict(s=max(fig['s'], rs), d=max(fig['d'], rd), ulps=max(fig['ulps'], ul))
            spans += [(t.data_ptr(), t.data_ptr() + 4 * t.numel()) for t in (s, d) if t is not None]
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))          # every returned view is disjoint from the others
        if mode == 'real':          # each row equals the same row computed alone (B = 1: one chunk, one image per iteration)
            for b in range(B):
                alone = F_.styles_batched(lg[b:b + 1], specs)
                for (s, d), (s1, d1) in zip(outs, alone):
                    assert torch.equal(s[b:b + 1], s1) and (d is None or torch.equal(d[b:b + 1], d1)), b
    _say('styles_batched B%d D%d L%d' % (B, D, L), **fig)


def _word(v):
    return int(np.float32(v).view(np.uint32))


@pytest.mark.parametrize('B,D,L', [(1, 64, 1), (5, 512, 18), (17, 193, 4), (64, 256, 4)])
def test_styles_batched_range_plans(B, D, L):
    """s_n == s * 2^e and d_n == d * 2^-e bit for bit, e recomputed on the host from the device's own s by the rule of include/sgdfr.h,
    and the pair equals F.split_range of the same s, d and plan."""
    F_ = _F()
    latent = S.counter_tensor(17, 'rp.lat%d.%d' % (B, D), (B, L, D))
    latent = latent * (2.0 ** ((torch.arange(B) % 7) - 3).float()).view(B, 1, 1)         # the rows' max |s| sit in different binades
    widths = [(6, 16), (10, 3), (64, 130), (130, 16), (512, 16), (64, 48), (10, 16), (6, 130), (130, 130), (64, 16), (10, 130)]
    layers = []
    for i, ((cin, cout), li) in enumerate(zip(widths, _latent_rows(L, len(widths)))):
        layers.append((li, _real_layer('rp.%d.%d.%d' % (B, D, i), D, cin, 0 if cout == 3 else cout, seed=17), cout))
    zero = (torch.zeros(64, D), torch.zeros(64), layers[5][1][2])                         # an all-zero style row: e = 0
    layers[5] = (layers[5][0], zero, 48)
    sub = torch.zeros(10)
    sub[3], sub[7] = 2.0 ** -130, -2.0 ** -128                                           # a subnormal max |s|
    layers[6] = (layers[6][0], (torch.zeros(10, D), sub, layers[6][1][2]), 16)
    words = {k: torch.tensor([v], dtype=torch.int64).to(torch.int32).cuda() for k, v in
             (('w37', _word(37.0)), ('w0', 0), ('winf', 0x7f800000), ('wsmall', _word(3e-5)))}
    plans = [(10, 0), None, (-5, 6), None, (words['w37'], 12), (0, 6), (10, 0), (words['w0'], 0), (words['winf'], 6),
             (words['wsmall'], 0), (-100, 12)]
    specs = _specs(layers)
    lg = latent.cuda()
    plain = F_.styles_batched(lg, specs)
    ranged = F_.styles_batched(lg, specs, plans=plans)
    es = []
    for i, (plan, (s, d), (s_n, d_n)) in enumerate(zip(plans, plain, ranged)):
        if plan is None or d is None:
            assert torch.equal(s_n, s) and (d is None or torch.equal(d_n, d)), i        # unplanned layers of the same call
            continue
        bound, headroom = plan
        kw = dict(word=int(bound.cpu()) & 0xffffffff) if isinstance(bound, torch.Tensor) else dict(x_log2=bound)
        want_s, want_d, e = R.apply_range(s, d, headroom, **kw)
        es.append(e)
        assert torch.equal(s_n.cpu(), want_s) and torch.equal(d_n.cpu(), want_d), (i, e)
        if isinstance(bound, torch.Tensor):
            a, b = F_.split_range(s, d, bound, headroom=headroom)
        else:
            a, b = F_.split_range(s, d, None, x_log2=bound, headroom=headroom)
        assert torch.equal(a, s_n) and torch.equal(b, d_n), i
    assert torch.equal(plain[6][0].cpu(), sub.expand(B, 10))                # the subnormal styles arrive as they are
    assert (es[3] == 0).all() and (es[5] == 0).all() and (es[6] == 0).all()                # zero row, zero word, non-finite word
    assert (es[4] == 120).all() and (es[8] > 60).all()                                     # subnormal styles clamp at +120; x_log2 = -100
    if B > 1:
        assert len(set(es[0].tolist())) > 1                                                # one exponent per image
    _say('range plans B%d D%d' % (B, D), e_min=min(int(e.min()) for e in es), e_max=max(int(e.max()) for e in es))


def test_styles_batched_refusals():
    F_ = _F()
    mw, mb, q = (t.cuda() for t in _real_layer('rf', 64, 10, 16))
    lat = torch.zeros(2, 2, 64).cuda()
    F_.styles_batched(lat, [(1, mw, mb, q, 16)], plans=[(100, 12)])
    for plan in ((10, 13), (10, -1), (101, 0), (-101, 0)):
        with pytest.raises(RuntimeError):
            F_.styles_batched(lat, [(1, mw, mb, q, 16)], plans=[plan])
    with pytest.raises(RuntimeError):
        F_.styles_batched(lat, [(2, mw, mb, q, 16)])                        # latent row out of range
    with pytest.raises(RuntimeError):
        F_.styles_batched(torch.zeros(2, 2, 513).cuda(), [(0, torch.zeros(10, 513).cuda(), mb, q, 16)])      # style dimension > 512


# ------------------------------------------------------------------ F.demod_grad

@pytest.mark.parametrize('B,cin,cout', [(1, 64, 64), (5, 63, 48), (128, 64, 512), (129, 64, 512), (3, 96, 513), (7, 130, 70)])
def test_demod_grad_edges(B, cin, cout):
    """ds = gs + s * ((-gd * d^3) @ Q): linear_skinny_kernel<2,2> (B <= 128, Cout <= 512, Cin >= 64) or launch_linear<2,2>."""
    F_ = _F()
    key = 'dg.%d.%d.%d' % (B, cin, cout)

    def ref(gd, d, qt, s, gs):
        v = -gd.double() * d.double() ** 3
        acc = v @ qt.double().t()
        mag = gs.double().abs() + s.double().abs() * (v.abs() @ qt.double().abs().t())
        return gs.double() + s.double() * acc, (cout + 8) * R.U * mag
    ins = (R.int_tensor(19, key + 'gd', (B, cout), -4, 4), R.choice_tensor(19, key + 'd', (B, cout), (0.5, 1.0, 2.0)),
           R.int_tensor(19, key + 'qt', (cin, cout), 0, 2), R.int_tensor(19, key + 's', (B, cin), -4, 4), R.int_tensor(19, key + 'gs', (B, cin)))
    assert _exact(F_.demod_grad(*[t.cuda() for t in ins]), ref(*ins)[0])
    ins = (S.counter_tensor(19, key + 'gd', (B, cout)), S.counter_tensor(19, key + 'd', (B, cout)).abs() * 0.3 + 0.6,
           S.counter_tensor(19, key + 'qt', (cin, cout)).abs(), S.counter_tensor(19, key + 's', (B, cin), 1.0, 0.3),
           S.counter_tensor(19, key + 'gs', (B, cin)))
    r = R.ratio(F_.demod_grad(*[t.cuda() for t in ins]), *ref(*ins))
    _say('demod_grad B%d %d<-%d' % (B, cin, cout), ratio=r)
    assert r <= 1.0


# ------------------------------------------------------------------ F.styles_batched_bwd, F.demod_dq, F.param_grads

BWD_B = (1, 7, 8, 9, 17)
BWD_D = (64, 200, 256)
# (kind, latent row, cin, cout): two layers share row 0; cin = 516 takes a second pass of the SG_MAXC loop with a 4-channel remainder;
# row 3 of the L = 4 latent is read by nobody
BWD_LAYERS = [('demod', 0, 6, 48), ('demod', 0, 64, 512), ('plain', 1, 516, 0), ('demod', 1, 130, 48), ('rgb', 2, 516, 3), ('rgb', 2, 64, 3)]


def _bwd_layers(mode, B, D):
    key = 'bw.%s.%d.%d' % (mode, B, D)
    out = []
    for i, (kind, li, cin, cout) in enumerate(BWD_LAYERS):
        k = '%s.%d' % (key, i)
        if mode == 'int':
            gen = lambda n, shape, lo=-2, hi=2: R.int_tensor(23, k + n, shape, lo, hi)
            e = {'latent_index': li, 'mod_w': gen('mw', (cin, D), -1, 1)}
            if kind == 'rgb':
                e['rgb_r'], e['rgb_w'] = gen('r', (B, 3 * cin)).view(B, 3, cin), gen('w', (3, cin))
            else:
                e['gs'] = gen('gs', (B, cin), -4, 4)
                if kind == 'demod':
                    e['a'], e['d'] = gen('a', (B, cout)), R.choice_tensor(23, k + 'd', (B, cout), (0.5, 1.0, 2.0))
                    e['s'], e['qt'] = gen('s', (B, cin)), gen('qt', (cin, cout), 0, 1)
        else:
            gen = lambda n, shape: S.counter_tensor(23, k + n, shape)
            e = {'latent_index': li, 'mod_w': gen('mw', (cin, D))}
            if kind == 'rgb':
                e['rgb_r'], e['rgb_w'] = gen('r', (B, 3, cin)), gen('w', (3, cin))
            else:
                e['gs'] = gen('gs', (B, cin))
                if kind == 'demod':
                    e['a'], e['d'] = gen('a', (B, cout)), gen('d', (B, cout)).abs() + 0.5
                    e['s'], e['qt'] = gen('s', (B, cin)), gen('qt', (cin, cout)).abs()
        out.append((kind, e))
    return out


def _dyadic_ds(kind, e):
    """Is dL/ds of this layer a dyadic fraction on the integer inputs?  Always, but for a ToRGB layer, whose 1/sqrt(cin) is a power
    of two only at cin = 64 (of the widths here)."""
    return kind != 'rgb' or e['mod_w'].shape[0] == 64


def _to_device(layers, wants):
    dev = []
    for (kind, e), (ww, wb) in zip(layers, wants):
        g = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in e.items()}
        if kind == 'demod':             # a = d * dL/dd arrives as a strided view of the [B, cout, 3] sums
            sums = torch.zeros(g['a'].shape + (3,), device='cuda')
            sums[:, :, 2] = g['a']
            g['a'] = sums[:, :, 2]
        g['want_w'], g['want_b'] = ww, wb
        dev.append(g)
    return dev


@pytest.mark.parametrize('D', BWD_D)
@pytest.mark.parametrize('B', BWD_B)
def test_styles_batched_bwd_edges(B, D):
    F_ = _F()
    L = 4
    wants = [(True, True), (False, True), (True, False), (False, False), (True, True), (False, False)]
    fig = dict(glat=0.0, gmod=0.0)
    for mode in ('int', 'real'):
        layers = _bwd_layers(mode, B, D)
        latent = (R.int_tensor(23, 'bw.lat%s%d.%d' % (mode, B, D), (B, L * D), -2, 2) if mode == 'int' else
                  S.counter_tensor(23, 'bw.lat%d.%d' % (B, D), (B, L * D))).view(B, L, D)
        want, per = R.style_bwd_reference(layers, latent, B, L, D)
        dev = _to_device(layers, wants)
        glat = F_.styles_batched_bwd(dev, B, L, D, latent=latent.cuda())
        assert glat.shape == (B, L, D)
        assert torch.equal(glat[:, 3], torch.zeros(B, D, device='cuda'))                 # the row nobody reads: exactly zero
        ws = R.wscale32(D)
        exact = mode == 'int' and R.pow4(D)
        bound = torch.zeros(B, L, D, dtype=torch.float64)
        terms = {l: sum(e['mod_w'].shape[0] for _, e in layers if e['latent_index'] == l) for l in range(L)}
        for (kind, e), (ds, gmw, gmb), g in zip(layers, per, dev):
            dsb = R.style_bwd_ds_bound(kind, e)
            mw, li = e['mod_w'].double().abs(), e['latent_index']
            bound[:, li] += ws * ((terms[li] + 8) * R.U * (ds.abs() @ mw) + dsb @ mw)
            dyadic = _dyadic_ds(kind, e)
            if exact and dyadic:
                assert float((ds.abs() @ mw).max()) * 4 < 2 ** 24                       # quarter-integers below 2^24: exact
            lat = latent[:, li].double()
            assert ('gmod_w' in g) == g['want_w'] and ('gmod_b' in g) == g['want_b']
            if g['want_w']:
                if exact and dyadic:
                    assert _exact(g['gmod_w'], gmw), (kind, 'gmod_w')
                else:
                    r = R.ratio(g['gmod_w'], gmw, ws * ((B + 8) * R.U * (ds.abs().t() @ lat.abs()) + dsb.t() @ lat.abs()))
                    fig['gmod'] = max(fig['gmod'], r)
            if g['want_b']:
                if mode == 'int' and dyadic:
                    assert _exact(g['gmod_b'], gmb), (kind, 'gmod_b')
                else:
                    fig['gmod'] = max(fig['gmod'], R.ratio(g['gmod_b'], gmb, (B + 8) * R.U * ds.abs().sum(0) + dsb.sum(0)))
        if exact:
            assert _exact(glat[:, :2], want[:, :2])                                     # rows 0, 1: dyadic sums, bit for bit
            fig['glat'] = max(fig['glat'], R.ratio(glat[:, 2], want[:, 2], bound[:, 2]))  # (1/sqrt(516) of the ToRGB layer is not)
        else:
            fig['glat'] = max(fig['glat'], R.ratio(glat, want, bound))
        # want_latent=False: no latent gradient, the parameter gradients are the same
        dev2 = _to_device(layers, wants)
        assert F_.styles_batched_bwd(dev2, B, L, D, latent=latent.cuda(), want_latent=False) is None
        for g, g2 in zip(dev, dev2):
            for k in ('gmod_w', 'gmod_b'):
                assert (k not in g) or torch.equal(g[k], g2[k])
    _say('styles_batched_bwd B%d D%d' % (B, D), **fig)
    assert fig['glat'] <= 1.0 and fig['gmod'] <= 1.0


PG_B = (1, 9)
PG_C = (1, 255, 256, 257)
PG_HW = (1, 255, 16385)


@pytest.mark.parametrize('B', PG_B)
def test_demod_dq_and_param_grads_edges(B):
    from stylegan_directions_face_reenactment_amd import _native as N
    F_ = _F()
    worst = 0.0
    for C in PG_C:
        for cout, cin in ((C, 7), (5, C)):
            key = 'dq.%d.%d.%d' % (B, cout, cin)
            for mode in ('int', 'real'):
                if mode == 'int':
                    a, d, s = R.int_tensor(29, key + 'a', (B, cout), -4, 4), R.choice_tensor(29, key + 'd', (B, cout), (0.5, 1.0, 2.0)), \
                        R.int_tensor(29, key + 's', (B, cin), -4, 4)
                else:
                    a, d, s = S.counter_tensor(29, key + 'a', (B, cout)), S.counter_tensor(29, key + 'd', (B, cout)).abs() + 0.5, \
                        S.counter_tensor(29, key + 's', (B, cin))
                sums = torch.zeros(B, cout, 3)
                sums[:, :, 2] = a
                dq = F_.demod_dq(sums.cuda()[:, :, 2], d.cuda(), s.cuda())
                ref = R.demod_dq_reference(a, d, s)
                if mode == 'int':
                    assert _exact(dq, ref), key
                else:
                    mag = ((a.double() / d.double()) * d.double() ** 3 * 0.5).abs().t() @ (s.double() ** 2)
                    worst = max(worst, R.ratio(dq, ref, (B + 8) * R.U * mag))
        for HW in PG_HW:
            key = 'pg.%d.%d.%d' % (B, C, HW)
            sums = R.int_tensor(29, key + 'sums', (B, C * 3)).view(B, C, 3)
            r_rgb, s_rgb = R.int_tensor(29, key + 'r', (B, 3 * C)).view(B, 3, C), R.int_tensor(29, key + 's', (B, C))
            g_rgb = R.int_tensor(29, key + 'g', (B * 3, HW)).view(B, 3, HW)
            entries = [(N.PGRAD_RGB_B, g_rgb.cuda(), None, 3, HW), (N.PGRAD_BIAS, sums.cuda(), None, C, 0), (N.PGRAD_NOISE, sums.cuda(), None, C, 0),
                       (N.PGRAD_RGB_W, r_rgb.cuda(), s_rgb.cuda(), C, 0), (N.PGRAD_RGB_B, g_rgb.cuda(), None, 3, HW)]
            for call in range(2):       # the ToRGB bias accumulates with atomics into a zeroed output: also on a second call
                gbr0, gb, gn, gw, gbr = F_.param_grads(entries, B)
                assert _exact(gb, sums[:, :, 0].double().sum(0)) and _exact(gn, sums[:, :, 1].double().sum().view(1)), (key, call)
                rs = r_rgb.double() * s_rgb.double().unsqueeze(1)
                if C in (1, 256):           # 1/sqrt(C) a power of two: bit for bit
                    assert _exact(gw, rs.sum(0) / C ** 0.5), (key, call)
                else:                       # B products, B - 1 additions, the scale (and its own rounding)
                    worst = max(worst, R.ratio(gw, rs.sum(0) / C ** 0.5, (B + 8) * R.U * rs.abs().sum(0) / C ** 0.5))
                assert _exact(gbr, g_rgb.double().sum((0, 2))) and torch.equal(gbr0, gbr), (key, call)
            g_real = S.counter_tensor(29, key + 'gr', (B, 3, HW))
            out, = F_.param_grads([(N.PGRAD_RGB_B, g_real.cuda(), None, 3, HW)], B)
            worst = max(worst, R.ratio(out, g_real.double().sum((0, 2)), (B * HW + 8) * R.U * g_real.double().abs().sum((0, 2))))
    _say('demod_dq / param_grads B%d' % B, ratio=worst)
    assert worst <= 1.0


# ------------------------------------------------------------------ pixel norm

@pytest.mark.parametrize('D', [1, 63, 64, 65, 512, 515])
@pytest.mark.parametrize('B', [1, 4, 5])
def test_pixel_norm_forward_and_gradient(B, D):
    """x * rsqrt(mean(x^2) + 1e-8) and its gradient against fp64 autograd, relative to max |ref| per row: D/64 serial adds per lane,
    the 6-step butterfly, the rsqrt and the final products -- (D/64 + 16) * 2^-23.  The last row is all zero.  At D = 1 the gradient
    is the eps * r^2 remainder of two cancelling terms: an fp32 difference of the two misses the bar there by six orders of magnitude
    (tests/test_cpu_dense_edges.py), the kernel keeps the eps term apart."""
    from stylegan_directions_face_reenactment_amd.autograd import PixelNormFn
    F_ = _F()
    x = S.counter_tensor(31, 'pn.x%d.%d' % (B, D), (B, D))
    x[-1] = 0.0
    g = S.counter_tensor(31, 'pn.g%d.%d' % (B, D), (B, D))
    ref, gref = R.pixelnorm_ref(x, g)
    bar = R.pixelnorm_bar(D)
    xg = x.cuda().requires_grad_(True)
    y = PixelNormFn.apply(xg)
    y.backward(g.cuda())
    assert torch.equal(F_.pixel_norm(x.cuda()), y.detach())
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xg.grad).all())
    assert torch.equal(y[-1].detach().cpu(), torch.zeros(D))
    assert torch.allclose(gref[-1], g[-1].double() * R.PIXELNORM_EPS ** -0.5, rtol=1e-12, atol=0)       # the zero row: g * rsqrt(eps)

    def rel(a, r):
        scale = r.detach().abs().amax(1, keepdim=True).clamp_min(1e-300)
        return float(((a.detach().double().cpu() - r.detach()).abs() / scale).max())
    ef, eb = rel(y, ref), rel(xg.grad, gref)
    _say('pixel_norm B%d D%d' % (B, D), fwd=ef / bar, bwd=eb / bar)
    assert ef <= bar and eb <= bar


# ------------------------------------------------------------------ F.affine

@pytest.mark.parametrize('M,K,N', [(1, 15, 64), (4, 512, 64), (130, 70, 64), (5, 513, 3), (3, 64, 515)])
def test_affine_gradients(M, K, N):
    """dX = g @ W, dW = g^T @ x, db = 1^T g through the linear kernels (three GEMMs on different sides of the dispatch)."""
    F_ = _F()
    worst = 0.0
    for mode in ('int', 'real'):
        key = 'af.%s.%d.%d.%d' % (mode, M, K, N)
        if mode == 'int':
            x, w, b = R.linear_inputs('int', M, K, N, seed=37)
            g = R.int_tensor(37, key + 'g', (M, N))
        else:
            x, w, b = R.linear_inputs('real', M, K, N, seed=37)
            g = S.counter_tensor(37, key + 'g', (M, N))
        xd, wd, bd, gd = x.double(), w.double(), b.double(), g.double()
        refs = dict(y=xd @ wd.t() + bd, y0=xd @ wd.t(), x=gd @ wd, w=gd.t() @ xd, b=gd.sum(0))        # y0: the bias absent
        bounds = dict(y=(K + 8) * R.U * (xd.abs() @ wd.abs().t() + bd.abs()), y0=(K + 8) * R.U * (xd.abs() @ wd.abs().t()),
                      x=(N + 8) * R.U * (gd.abs() @ wd.abs()), w=(M + 8) * R.U * (gd.abs().t() @ xd.abs()), b=(M + 8) * R.U * gd.abs().sum(0))
        gT = g.t().contiguous().cuda().t()                        # non-contiguous upstream gradients: transposed, and sliced
        gS = torch.cat([g, g + 1.0], 1).cuda()[:, :N]
        for upstream, need, bias in ((gT, 'xwb', True), (gS, 'xwb', True), (gT, 'xw', False), (gS, 'x', True), (gT, 'w', True),
                                     (gS, 'wb', True)):
            assert not upstream.is_contiguous() or M == 1 or N == 1
            xg, wg, bg = x.cuda().requires_grad_('x' in need), w.cuda().requires_grad_('w' in need), b.cuda().requires_grad_('b' in need)
            if need == 'x':
                wg = wg.detach()
            y = F_.affine(xg, wg, bg if bias else None)
            y.backward(upstream)
            got = {'y' if bias else 'y0': y, 'x': xg.grad, 'w': wg.grad, 'b': bg.grad if bias else None}
            for k in 'xwb':
                assert (got[k] is not None) == (k in need and (bias or k != 'b')), (need, k)
            for k, v in got.items():
                if v is None:
                    continue
                if mode == 'int':
                    assert _exact(v, refs[k]), (key, need, k)
                else:
                    worst = max(worst, R.ratio(v, refs[k], bounds[k]))
    _say('affine %dx%dx%d' % (M, K, N), ratio=worst)
    assert worst <= 1.0


# ------------------------------------------------------------------ uint8 packing

@pytest.mark.parametrize('B,H,W', [(1, 1, 1), (3, 5, 7), (2, 17, 35), (1, 725, 725)])
def test_images_to_uint8_is_the_float32_evaluation(B, H, W):
    """Every byte equals uint8((clamp(v) + 1) / (2 + 1e-5) * 255) evaluated in IEEE float32 on the probe set (the values next to all 254
    integer boundaries); 725 x 725 pixels are more than the 2048 blocks of the grid cap take in one pass."""
    from stylegan_directions_face_reenactment_amd.reenact import images_to_uint8, grid_frames_uint8
    img = R.u8_image(B, H, W, offset=5 * H)
    want = R.u8_np32(img).transpose(0, 2, 3, 1)
    got = images_to_uint8(torch.from_numpy(img).cuda())
    assert got.dtype == torch.uint8 and got.shape == (B, H, W, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(grid_frames_uint8([torch.from_numpy(img).cuda()]).cpu().numpy(), want)
    if B * H * W * 3 >= 1788:
        assert (want != R.u8_f64(img).transpose(0, 2, 3, 1)).any()         # the fp64 evaluation would not pass


@pytest.mark.parametrize('B,H,W', [(3, 5, 7), (2, 17, 35)])
def test_grid_frames_uint8_panels(B, H, W):
    from stylegan_directions_face_reenactment_amd.reenact import grid_frames_uint8
    full = [R.u8_image(B, H, W, offset=311 * k) for k in range(4)]
    one = R.u8_image(1, H, W, offset=977)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for swap in (False, True):
        for K in (1, 2, 3, 4):
            panels = list(full[:K])
            if K >= 2:
                panels[1] = one                                             # a [1,3,H,W] panel shown in every frame
            want, _ = R.u8_grid_host(panels, B, swap)
            got = grid_frames_uint8([dev(p) for p in panels], swap_rb=swap)
            assert got.shape == (B, H, K * W, 3) and np.array_equal(got.cpu().numpy(), want), (K, swap)
        # a skipped panel: its columns of `out` keep their pattern, the others are written
        panels = [full[0], None, one, full[3]]
        want, mask = R.u8_grid_host(panels, B, swap)
        pattern = (np.arange(B * H * 4 * W * 3) % 251).astype(np.uint8).reshape(B, H, 4 * W, 3)
        out = torch.from_numpy(pattern.copy()).cuda()
        got = grid_frames_uint8([dev(p) for p in panels], swap_rb=swap, out=out)
        assert got is out and np.array_equal(out.cpu().numpy(), np.where(mask, want, pattern)), swap


def test_uint8_wrappers_refuse():
    from stylegan_directions_face_reenactment_amd.reenact import images_to_uint8, grid_frames_uint8
    x = torch.zeros(2, 3, 4, 6).cuda()
    for bad in (lambda: grid_frames_uint8([x] * 5), lambda: grid_frames_uint8([x, None]),
                lambda: grid_frames_uint8([x, None], out=torch.zeros(2, 4, 11, 3, dtype=torch.uint8).cuda()),
                lambda: grid_frames_uint8([x, None], out=torch.zeros(2, 4, 12, 3).cuda()),
                lambda: images_to_uint8(torch.zeros(2, 4, 4, 6).cuda()), lambda: images_to_uint8(torch.zeros(2, 3, 4, 6))):
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------------------ FusedAdam

def test_fused_adam_at_the_tensor_limit_and_chunk_edges():
    """N.MAX_ADAM_TENSORS tensors whose sizes straddle the 1024-element chunks of the block -> (tensor, chunk) search, four steps
    against the fp64 restatement of _single_tensor_adam fed the same fp32 gradients (bars of test_fused_adam_equals_torch_adam)."""
    from stylegan_directions_face_reenactment_amd import _native as N
    from stylegan_directions_face_reenactment_amd.finetune import FusedAdam
    n = N.MAX_ADAM_TENSORS
    sizes = [R.ADAM_SIZES[i % len(R.ADAM_SIZES)] for i in range(n)]
    p0 = [S.counter_tensor(41, 'ad.p%d' % i, (sz,)) for i, sz in enumerate(sizes)]
    ps = [p.cuda().requires_grad_(True) for p in p0]
    opt, ref = FusedAdam(ps), R.Adam64(p0)
    worst = 0.0
    for step in range(4):
        grads = [S.counter_tensor(41, 'ad.g%d.%d' % (step, i), (sz,), 0.0, 10.0 ** (step - 2)) for i, sz in enumerate(sizes)]
        for p, g in zip(ps, grads):
            p.grad = g.cuda()
        opt.step()
        ref.step(grads)
        for i, (p, r) in enumerate(zip(ps, ref.p)):
            got = p.detach().cpu()
            for j in (0, -1):           # the first and the last element of every tensor
                assert abs(float(got[j]) - float(r[j])) <= 1e-7 + 2e-6 * abs(float(r[j])), (step, i, j)
            assert torch.allclose(got.double(), r, rtol=2e-6, atol=1e-7), (step, i, sizes[i])
            worst = max(worst, float(((got.double() - r).abs() / (1e-7 + 2e-6 * r.abs())).max()))
    assert float(opt.step_count) == 4.0
    _say('FusedAdam %d tensors' % n, err_over_bar=worst)
    with pytest.raises(ValueError):
        FusedAdam([torch.zeros(1).cuda() for _ in range(n + 1)])


def test_fused_adam_skips_parameters_without_a_gradient():
    """FusedAdam.step updates the parameters that have a gradient (one launch over those) and leaves the others, their moments
    included, untouched; the one device step count moves once per step that updates anything, not at all otherwise."""
    from stylegan_directions_face_reenactment_amd.finetune import FusedAdam
    sizes = (1025, 7, 2049)
    p0 = [S.counter_tensor(43, 'as.p%d' % i, (sz,)) for i, sz in enumerate(sizes)]
    ps = [p.cuda().requires_grad_(True) for p in p0]
    opt, ref = FusedAdam(ps), R.Adam64(p0)
    opt.step()                                                              # nothing has a gradient: not a step
    assert float(opt.step_count) == 0.0 and all(torch.equal(p.detach().cpu(), q) for p, q in zip(ps, p0))
    for step in range(3):
        grads = [S.counter_tensor(43, 'as.g%d.%d' % (step, i), (sz,)) for i, sz in enumerate(sizes)]
        grads[1] = None
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.cuda()
        v1 = ps[1]._version
        opt.step()
        ref.step(grads)
        assert torch.equal(ps[1].detach().cpu(), p0[1]) and ps[1]._version == v1
        assert float(opt.state[ps[1]]['exp_avg'].abs().max()) == 0.0 and float(opt.state[ps[1]]['exp_avg_sq'].abs().max()) == 0.0
        for i in (0, 2):
            assert torch.allclose(ps[i].detach().cpu().double(), ref.p[i], rtol=2e-6, atol=1e-7), (step, i)
    assert float(opt.step_count) == 3.0


def test_fused_adam_shares_one_step_count_between_live_and_skipped_steps():
    """A parameter that has a gradient at some steps and none at others: at a skipped step it and its moments stay bit for bit; at a
    live step its moments advance once and the bias correction is that of the ONE device step count (the number of steps in which
    anything was updated), not of the number of its own updates.  That is where FusedAdam departs from torch.optim.Adam, whose count
    is per parameter: the expectation is Adam64(shared_count=True), and the per-parameter count is checked to lie far outside the
    bars, so the case tells the two apart."""
    from stylegan_directions_face_reenactment_amd.finetune import FusedAdam
    sizes = (1025, 300, 7)
    p0 = [S.counter_tensor(45, 'aa.p%d' % i, (sz,)) for i, sz in enumerate(sizes)]
    ps = [p.cuda().requires_grad_(True) for p in p0]
    opt, ref, torch_like = FusedAdam(ps), R.Adam64(p0, shared_count=True), R.Adam64(p0)
    worst = apart = 0.0
    for step in range(5):
        grads = [S.counter_tensor(45, 'aa.g%d.%d' % (step, i), (sz,)) for i, sz in enumerate(sizes)]
        if step in (0, 2, 3):
            grads[1] = None                                                 # parameter 1 is live at steps 1 and 4 only
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.cuda()
        before = [t.clone() for t in (ps[1].detach(), opt.state[ps[1]]['exp_avg'], opt.state[ps[1]]['exp_avg_sq'])]
        opt.step()
        ref.step(grads)
        torch_like.step(grads)
        after = (ps[1].detach(), opt.state[ps[1]]['exp_avg'], opt.state[ps[1]]['exp_avg_sq'])
        if grads[1] is None:
            assert all(torch.equal(a, b) for a, b in zip(before, after)), step
        for i, (p, r) in enumerate(zip(ps, ref.p)):
            assert torch.allclose(p.detach().cpu().double(), r, rtol=2e-6, atol=1e-7), (step, i)
            worst = max(worst, float(((p.detach().cpu().double() - r).abs() / (1e-7 + 2e-6 * r.abs())).max()))
        assert float(opt.step_count) == step + 1.0
    assert ref.t == [5, 5, 5] and torch_like.t == [5, 2, 5]
    apart = float(((ref.p[1] - torch_like.p[1]).abs() / (1e-7 + 2e-6 * ref.p[1].abs())).max())
    _say('FusedAdam alternating parameter', err_over_bar=worst, per_parameter_count_over_bar=apart)
    assert apart > 10.0


# ------------------------------------------------------------------ F.absmax

@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 4100])
@pytest.mark.parametrize('B', [1, 3, 17])
def test_absmax_words(B, n):
    """Words == the bit pattern of x.abs().amax(): sizes that are no multiple of four and a pointer one element past the alignment take
    the scalar loop, the others the 16-byte loads."""
    F_ = _F()
    key = 'am.%d.%d' % (B, n)
    base = S.counter_tensor(47, key, (B * n + 5,))
    for variant in ('plain', 'last', 'first', 'special', 'tiny'):
        x = base.clone()
        flat = x[1:1 + B * n]
        if variant == 'tiny':                                               # zeros, -0.0 and one subnormal: the last image's maximum
            x.zero_()
            flat[0], flat[-1] = -0.0, float(np.float32(2.0 ** -130))
        if variant == 'last':
            flat[-1] = -1e6                                                 # the maximum is the very last element
        if variant == 'first':
            flat[0] = 1e6
        if variant == 'special':
            flat[0] = -0.0
            flat[-1] = float(np.float32(2.0 ** -130)) if n > 1 else -0.0
        for aligned in (True, False):
            if aligned:
                xg = flat.clone().view(B, n).cuda()
            else:
                xg = x.cuda().flatten()[1:1 + B * n].view(B, n)            # storage offset of one element: a misaligned pointer
                assert xg.is_contiguous() and xg.data_ptr() % 16 == 4
            want = flat.view(B, n).abs().amax(1).view(torch.int32)
            assert torch.equal(F_.absmax(xg).cpu(), want), (variant, aligned)
            assert int(F_.absmax(xg, per_image=False).cpu()) == int(flat.abs().max().view(torch.int32)), (variant, aligned)
    shared = F_.absmax(base[:n].view(1, n).cuda(), batch=B)                  # one [1, ...] tensor standing for B images: one word
    assert shared.shape == (1,) and int(shared.cpu()) == int(base[:n].abs().max().view(torch.int32))
    for bad in (float('inf'), float('-inf'), float('nan')):                 # non-finite contents: a word >= 0x7f800000
        x = base[:B * n].clone().view(B, n)
        x[B // 2, n // 2] = bad
        w = F_.absmax(x.cuda()).cpu()
        assert int(w[B // 2]) >= 0x7f800000 and int(F_.absmax(x.cuda(), per_image=False).cpu()) >= 0x7f800000
        others = [i for i in range(B) if i != B // 2]
        assert torch.equal(w[others], x[others].abs().amax(1).view(torch.int32))
        xo = torch.cat([torch.zeros(1), x.flatten()]).cuda()[1:].view(B, n)
        assert int(F_.absmax(xo).cpu()[B // 2]) >= 0x7f800000

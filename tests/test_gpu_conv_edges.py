"""The fp32 convolution path (csrc/modconv.hip, csrc/wino.hip, blur_bias_act_kernel of csrc/upfirdn2d.hip) at its tile, staging and
dispatch edges, each kernel against a plain fp64 reference (tests/conv_refs.py, itself checked on the CPU by
tests/test_cpu_conv_edges.py, which also proves that the case lists cross every rung and limit from both sides).

Two kinds of check (conv_refs.py): EXACT on small integers (every partial sum below 2^24 of its unit: torch.equal with the fp64
reference, every word of the output) and BOUNDED on synthetic.counter_tensor inputs through the real prepack with the a-priori
per-element bound (K + c) 2^-24 (|x s| (*) |w| |d| + |noise term| + |bias|), after an activation bound * gain + 2^-23 |ref|.  Every test
prints its worst error / bound ratio on a line starting with "conv-edges" (pytest -s); the bars are derived, never fitted.

group                     bar
F.prepack                 wp == fp32(w * scale32) bit for bit; q, qt: ratio <= 1 (K = k*k, c = 2), exact for k = 1 at Cin 4, 16, 64
F.prepack_wino            == scale32 * the restated pack within 2 ulp of the entry's magnitude sum |G| |w| |G^T| scale32
PLAIN3 (MFMA tiles)       exact; ratio <= 1 (K = 9 Cin, c = 8); refused widths raise "staged range"
direct kernel             exact; ratio <= 1; misaligned s / wp views == the aligned MFMA call bit for bit
split-K                   exact, == the unsplit launch bit for bit; ratio <= 1 (K = 9 Cin, c = 8 + splits)
UP3 / DOWN3               exact (UP3: the plane entries outside the transposed conv are 0); ratio <= 1 (K = 4 Cin / 9 Cin)
F.blur_bias_act           exact with both FIRs; ratio <= 1 (K = 16, c = 4); absmax words == bits of y.abs().amax((2, 3))
F.torgb                   exact at Cin 4, 16, 64, 256; ratio <= 1 (K = Cin, c = 8)
F.modconv_wino            exact through the test-built pack, == the direct fp32 kernel bit for bit; ratio <= 1 (K = Cin, c = 20, the
                          Winograd algorithm on absolute values)

Measured on an MI355X (worst error / bound over the cases of each group):
F.prepack                 q / qt 0.325
F.prepack_wino            1.71 ulp of the 2 ulp bar
PLAIN3 (MFMA tiles)       128x128 0.12, 64x256 0.151, 64x128 0.137, 64x64 0.13, 32x128 0.0488; epilogue kinds 0.0454
direct kernel             0.0984
split-K                   through modconv_raw 0.00969, through the entry 0.0312
UP3                       128x64 0.213, 64x64 0.218, 32x128 0.145
DOWN3                     128x128 0.12, 64x64 0.148, 32x128 0.0495
F.blur_bias_act           0.183
F.torgb                   0.222
F.modconv_wino            0.0203
The exact checks and the absmax words are bit for bit: they have no figure.  No kernel failed a check; the staged-range rule
leaves no spare element for PLAIN3 and DOWN3 tiles that lie in one row, in whole rows or in one image, and one spare element for
UP3 (xlen = PT + P + 2 where PT + P + 1 are read), so on the 64-pixel tile UP3 takes W = 701 at H = 1 (64 + 702 + 2 = 768) and
W = 702 is the first width refused.

Bite check (scratch builds, nothing committed): p.xlen one short in launch_modconv fails 59 cases (test_plain3_tiles 35,
test_down3_tiles, test_plain3_epilogue_kinds, the split-K tests, the Winograd == direct comparisons); the last K stage of a split-K
slice dropped fails 13 (test_splitk_through_modconv_raw 7, test_splitk_entry_with_unequal_and_single_stage_slices 5, the upsample
chain at Cin 64); ky and kx swapped in the blur's flipped taps fails 12 (test_blur_finish 7, test_blur_finish_grid_stride,
test_upsample_chain_is_conv_transpose_and_upfirdn 4).
"""
import numpy as np
import pytest
import torch

import conv_refs as R
from util import O, S

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
    print('conv-edges %-44s %s' % (what, '  '.join('%s %.3g' % kv for kv in figures.items())))


def _dev(i):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in i.items()}


def _eq(y, ref64):
    return y.dtype == torch.float32 and y.shape == ref64.shape and torch.equal(y, ref64.float().to(y.device))


def _ratio(y, ref, bound):
    """conv_refs.ratio on the device (the large cases stay there)."""
    err = (y.double() - ref).abs()
    assert y.shape == ref.shape and bool((err[bound == 0] == 0).all()), 'error under a zero bound'
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


def _no_splitk(F_):
    return F_.using(F_.config().replace(use_splitk=False))


def _firs():
    sym = O.make_fir([1, 3, 3, 1], gain=4.0)
    asym = torch.tensor([[1, -2, 3, 4], [5, 6, -7, 8], [-3, 2, 1, 7], [4, -6, 5, 2]], dtype=torch.float32) / 16
    return sym.to(DEV), asym.to(DEV)


def _inputs(F_, kind, c, seed=13):
    """Device inputs of a case; 'real' packs a counter-tensor weight with F.prepack (the pack under test elsewhere)."""
    i = _dev(R.conv_inputs(kind, c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W'], noise=c['noise'], bias=c['bias'],
                           bcast=c['bcast'], seed=seed))
    if kind == 'real':
        w = S.counter_tensor(seed, 'cvw.' + R.case_id(c), (1, c['cout'], c['cin'], 3, 3))
        i['wp'] = F_.prepack(w.to(DEV))[0]
    return i


def _launch(F_, c, i, act, slope=0.2, gain=2 ** 0.5):
    return F_.modconv_raw(i['x'], i['wp'], i['s'], i['d'], c['cout'], c['mode'], c['H'], c['W'], noise=i['noise'],
                          noise_weight=i['noise_w'], bias=i['bias'], activate=act, slope=slope, gain=gain, batch=c['B'])


def _reference(c, i, act, slope=0.2, gain=2 ** 0.5, extra=0):
    if c['mode'] == R.PLAIN3:
        return R.plain3_ref(i['x'], i['wp'], i['s'], i['d'], i['noise'], i['noise_w'], i['bias'], act, slope, gain, batch=c['B'],
                            c=8 + extra)
    if c['mode'] == R.UP3:
        return R.up3_ref(i['x'], i['wp'], i['s'], i['d'], batch=c['B'], c=8 + extra)
    x = i['x'].expand(c['B'], *i['x'].shape[1:]) if c['bcast'] else i['x']
    return R.down3_ref(x, i['wp'], i['s'], i['d'], None, None, i['bias'], act, slope, gain, c=8 + extra)


def _check_case(F_, c, tag):
    """EXACT on integers (all words of the output), then BOUNDED on real inputs; returns the worst ratio."""
    act = c['act'] and c['mode'] != R.UP3
    i = _inputs(F_, 'int', c)
    y = _launch(F_, c, i, act, **EX)
    ref, _ = _reference(c, i, act, **EX)
    assert _eq(y, ref), (tag, R.case_id(c), 'exact', float((y.double() - ref).abs().max()))
    if c['mode'] == R.UP3:
        assert bool((y[:, :, R.planes_outside(c['H'], c['W'], DEV)] == 0).all()), (tag, R.case_id(c), 'outside entries')
    worst = 0.0
    if c['real']:
        i = _inputs(F_, 'real', c)
        worst = _ratio(_launch(F_, c, i, act), *_reference(c, i, act))
    _say('%s %s %s' % (tag, R.case_id(c), R.plan(c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W'])[0]), ratio=worst)
    assert worst <= 1.0, (tag, R.case_id(c), worst)
    return worst


# ------------------------------------------------------------------ the packs

@pytest.mark.parametrize('cin,cout', [(8, 64), (16, 128), (64, 64), (20, 6)])
def test_wino_pack_restatement(cin, cout):
    """F.prepack_wino == scale32 * U[ci][o][(a ^ (o & 3)) * 4 + b] = (G w G^T)[a][b] of conv_refs.wino_pack.  The 2 ulp are taken at
    the entry's magnitude sum (|G| |w| |G^T|) scale32: an entry that cancels has no ulp of its own to be measured in."""
    F_ = _F()
    w = S.counter_tensor(17, 'wpk.%d.%d' % (cin, cout), (1, cout, cin, 3, 3))
    u = F_.prepack_wino(w.to(DEV)).cpu()
    sc = R.wscale32(9 * cin)
    want = R.wino_pack(w[0]) * sc
    mag = R.wino_pack(w[0].abs(), R.WG.abs()) * sc
    ulp = torch.from_numpy(np.spacing(mag.numpy().astype(np.float32)).astype(np.float64))
    worst = float(((u.double() - want).abs() / ulp).max())
    _say('prepack_wino %d->%d' % (cin, cout), ulps=worst)
    assert u.shape == (cin, cout, 16) and worst <= 2.0
    # the adjoint pack is the pack of the rotated, transposed kernel
    ua = F_.prepack_wino(w.to(DEV), adjoint=True).cpu()
    wa = w[0].flip(2, 3).transpose(0, 1).contiguous()
    worst = float(((ua.double() - R.wino_pack(wa) * sc).abs() /
                   torch.from_numpy(np.spacing((R.wino_pack(wa.abs(), R.WG.abs()) * sc).numpy().astype(np.float32)).astype(np.float64))).max())
    assert ua.shape == (cout, cin, 16) and worst <= 2.0


@pytest.mark.parametrize('cin,cout,k', [(8, 64, 3), (6, 10, 3), (64, 36, 3), (512, 3, 1), (16, 3, 1), (5, 7, 1)])
def test_prepack_bit_for_bit(cin, cout, k):
    F_ = _F()
    w = S.counter_tensor(19, 'pk.%d.%d.%d' % (cin, cout, k), (1, cout, cin, k, k))
    wp, q, qt = (t.cpu() for t in F_.prepack(w.to(DEV)))
    sc = np.float32(R.wscale32(cin * k * k))
    want = (w[0].numpy() * sc).astype(np.float32).reshape(cout, cin, k * k).transpose(1, 2, 0)
    assert wp.shape == (cin, k * k, cout) and np.array_equal(wp.numpy(), want)
    qref = (wp.double() ** 2).sum(1).t()                                    # [Cout,Cin] from the device's own wp
    worst = R.ratio(q, qref, (k * k + 2) * R.U * qref)
    _say('prepack q %d->%d k%d' % (cin, cout, k), ratio=worst)
    assert worst <= 1.0 and torch.equal(qt, q.t())
    if k == 1 and cin in (4, 16, 64):                                       # scale a power of two: integers stay exact
        wi = R.int_tensor(19, 'pki.%d' % cin, (cout, cin)).view(1, cout, cin, 1, 1)
        wp, q, qt = (t.cpu() for t in F_.prepack(wi.to(DEV)))
        assert torch.equal(wp, (wi[0, :, :, 0, 0].t() * float(sc)).reshape(cin, 1, cout))
        assert torch.equal(q, (wi[0, :, :, 0, 0] * float(sc)) ** 2) and torch.equal(qt, q.t())


def test_prepack_exact_on_a_power_of_four():
    """k = 1, Cin 4 / 16 / 64: 1/sqrtf(Cin) is a power of two, so wp, q and qt of integer weights are exact."""
    F_ = _F()
    for cin in (4, 16, 64):
        sc = R.wscale32(cin)
        wi = R.int_tensor(19, 'pkx.%d' % cin, (7, cin)).view(1, 7, cin, 1, 1)
        wp, q, qt = (t.cpu() for t in F_.prepack(wi.to(DEV)))
        assert sc * sc * cin == 1.0 and torch.equal(wp, (wi[0, :, :, 0, 0].t() * sc).reshape(cin, 1, 7))
        assert torch.equal(q, (wi[0, :, :, 0, 0] * sc) ** 2) and torch.equal(qt, q.t())


# ------------------------------------------------------------------ PLAIN3, MFMA tiles

@pytest.mark.parametrize('c', R.PLAIN_CASES, ids=R.case_id)
def test_plain3_tiles(c):
    """One sgdfr_modconv2d_fwd_f32 launch (split-K off: the tile the dispatch rule names runs alone)."""
    F_ = _F()
    tile, st = R.plan(R.PLAIN3, c['B'], c['cin'], c['cout'], c['H'], c['W'])
    assert tile != 'direct' and st['ok']
    with _no_splitk(F_):
        _check_case(F_, c, 'plain3')


@pytest.mark.parametrize('cout', [64, 32])
def test_plain3_epilogue_kinds(cout):
    """Noise absent / shared [1,1,H,W] / per sample, with and without bias and activation, batched and broadcast input."""
    F_ = _F()
    worst = 0.0
    with _no_splitk(F_):
        for noise in ('none', 'shared', 'per'):
            for bias in (False, True):
                for act in (False, True):
                    for bcast in (False, True):
                        c = R.C(R.PLAIN3, 5, 12, cout, 9, 11, noise=noise, bias=bias, act=act, bcast=bcast, real=True)
                        worst = max(worst, _check_case(F_, c, 'plain3 %s%s%s' % (noise, '+b' if bias else '', '+act' if act else '')))
                        i = _inputs(F_, 'int', c)
                        y = _launch(F_, c, dict(i, d=None), act, **EX)          # no demodulation: d = 1
                        assert _eq(y, _reference(c, dict(i, d=None), act, **EX)[0])
    assert worst <= 1.0


@pytest.mark.parametrize('mode,cases', [(R.PLAIN3, R.PLAIN_REFUSED), (R.UP3, R.UP_REFUSED), (R.DOWN3, R.DOWN_REFUSED)],
                         ids=['plain', 'up', 'down'])
def test_too_wide_images_are_refused(mode, cases):
    """The first width the staged-range rule refuses (its left neighbour runs EXACT in the tile tests): a clean RuntimeError."""
    F_ = _F()
    for B, cin, cout, H, W in cases:
        assert not R.plan(mode, B, cin, cout, H, W)[1]['ok']
        c = R.C(mode, B, cin, cout, H, W, noise='none', bias=False)
        i = _inputs(F_, 'int', c)
        with _no_splitk(F_), pytest.raises(RuntimeError, match='staged range'):
            _launch(F_, c, i, False)


# ------------------------------------------------------------------ the direct kernel

@pytest.mark.parametrize('c', R.DIRECT_CASES + [R.DIRECT_STRIDE_CASE], ids=R.case_id)
def test_direct_kernel(c):
    F_ = _F()
    assert R.tile_of(c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W']) == 'direct'
    _check_case(F_, c, 'direct')


@pytest.mark.parametrize('mode', [R.PLAIN3, R.UP3, R.DOWN3])
def test_misaligned_s_and_wp_take_the_direct_kernel(mode):
    """s / wp one float off 16 bytes (channel counts that otherwise run on the MFMA tiles): the same words as the aligned call."""
    F_ = _F()
    c = R.C(mode, 3, 8, 64, 9, 11, noise='per' if mode == R.PLAIN3 else 'none', bias=mode != R.UP3, act=mode != R.UP3)
    assert R.tile_of(mode, 3, 8, 64, 9, 11) == (64, 64, 3) and R.tile_of(mode, 3, 8, 64, 9, 11, aligned=False) == 'direct'
    i = _inputs(F_, 'int', c)

    def off(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    act = mode != R.UP3
    with _no_splitk(F_):
        y = _launch(F_, c, i, act, **EX)
        ref = _reference(c, i, act, **EX)[0]
        assert _eq(y, ref)
        for which in (('s',), ('wp',), ('s', 'wp')):
            y2 = _launch(F_, c, dict(i, **{k: off(i[k]) for k in which}), act, **EX)
            assert torch.equal(y2, y), (mode, which)


# ------------------------------------------------------------------ split-K

@pytest.mark.parametrize('case', R.SPLITK_RAW_CASES, ids=lambda t: '-'.join(str(int(v)) for v in t))
def test_splitk_through_modconv_raw(case):
    F_ = _F()
    mode, B, cin, cout, H, W, bcast, splits = case
    assert _N().load().sgdfr_modconv2d_splitk_hint(B, cin, cout, H, W, mode) == splits == R.splitk_hint(B, cin, cout, H, W, mode)
    c = R.C(mode, B, cin, cout, H, W, bcast=bcast, noise='per' if mode == R.PLAIN3 else 'none', bias=True, act=True, real=True)
    act = mode == R.PLAIN3
    i = _inputs(F_, 'int', c)
    y = _launch(F_, c, i, act, **EX)                                         # default configuration: use_splitk on
    assert F_.config().use_splitk and _eq(y, _reference(c, i, act, **EX)[0])
    with _no_splitk(F_):
        assert torch.equal(_launch(F_, c, i, act, **EX), y)                  # bit-identical to the unsplit launch
    i = _inputs(F_, 'real', c)
    worst = _ratio(_launch(F_, c, i, act), *_reference(c, i, act, extra=splits))
    _say('splitK%d %s' % (splits, R.case_id(c)), ratio=worst)
    assert worst <= 1.0


def _splitk_entry(c, i, splits, act, slope=0.2, gain=2 ** 0.5):
    N = _N()
    B, cin, cout, H, W, mode = c['B'], c['cin'], c['cout'], c['H'], c['W'], c['mode']
    shape = (B, cout, 4, H + 1, W + 1) if mode == R.UP3 else (B, cout, H, W)
    y = torch.empty(shape, device=DEV)
    part = torch.empty((max(splits, 1),) + shape, device=DEV)
    nz = i['noise']
    N.call('sgdfr_modconv2d_splitk_f32', N.ptr(i['x']), i['x'][0].numel(), N.ptr(i['wp']), N.ptr(i['s']), N.ptr(i['d']), N.ptr(nz),
           0 if nz is None or nz.shape[0] == 1 else H * W, N.ptr(i['noise_w']) if nz is not None else None, N.ptr(i['bias']), N.ptr(y),
           N.ptr(part), splits, B, cin, cout, H, W, mode, int(act), float(slope), float(gain), N.stream())
    return y


@pytest.mark.parametrize('case', R.SPLITK_DIRECT_CASES, ids=lambda t: '-'.join(str(int(v)) for v in t))
def test_splitk_entry_with_unequal_and_single_stage_slices(case):
    """sgdfr_modconv2d_splitk_f32 itself: splits = Cin / 4 (one K stage per slice) and 16 stages split 5 + 5 + 6."""
    F_ = _F()
    mode, B, cin, cout, H, W, splits = case
    c = R.C(mode, B, cin, cout, H, W, noise='shared' if mode == R.PLAIN3 else 'none', bias=True, act=True, real=True)
    act = mode == R.PLAIN3
    i = _inputs(F_, 'int', c)
    y = _splitk_entry(c, i, splits, act, **EX)
    assert _eq(y, _reference(c, i, act, **EX)[0])
    with _no_splitk(F_):
        assert torch.equal(_launch(F_, c, i, act, **EX), y)
    i = _inputs(F_, 'real', c)
    worst = _ratio(_splitk_entry(c, i, splits, act), *_reference(c, i, act, extra=splits))
    _say('splitK entry %d slices %s' % (splits, R.case_id(c)), ratio=worst)
    assert worst <= 1.0


def test_splitk_entry_refusals():
    F_ = _F()
    for mode, cin, cout, splits in ((R.PLAIN3, 16, 32, 2), (R.DOWN3, 16, 64, 2), (R.PLAIN3, 16, 64, 5), (R.PLAIN3, 16, 64, 1)):
        c = R.C(mode, 2, cin, cout, 5, 7, noise='none', bias=False)
        i = _inputs(F_, 'int', c)
        with pytest.raises(RuntimeError, match='modconv_splitk'):
            _splitk_entry(c, i, splits, False)


# ------------------------------------------------------------------ UP3, DOWN3

@pytest.mark.parametrize('c', R.UP_CASES, ids=R.case_id)
def test_up3_tiles(c):
    F_ = _F()
    assert R.plan(R.UP3, c['B'], c['cin'], c['cout'], c['H'], c['W'])[1]['ok']
    with _no_splitk(F_):
        _check_case(F_, c, 'up3')


@pytest.mark.parametrize('c', R.DOWN_CASES, ids=R.case_id)
def test_down3_tiles(c):
    F_ = _F()
    assert R.plan(R.DOWN3, c['B'], c['cin'], c['cout'], c['H'], c['W'])[1]['ok']
    _check_case(F_, c, 'down3')


# ------------------------------------------------------------------ the blur finish

def _blur_inputs(kind, B, Cc, H, W, noise, seed=23):
    key = 'bl.%s.%d.%d.%d.%d' % (kind, B, Cc, H, W)
    mk = (lambda k, shape: R.int_tensor(seed, key + k, shape)) if kind == 'int' else (lambda k, shape: S.counter_tensor(seed, key + k, shape))
    planes = mk('t', (B, Cc, 4, H + 1, W + 1))
    nz = None if noise == 'none' else mk('n', (1 if noise == 'shared' else B, 1, 2 * H, 2 * W))
    nw = torch.tensor([3.0 if kind == 'int' else 0.3])
    return planes.to(DEV), (nz.to(DEV) if nz is not None else None), nw.to(DEV), mk('b', (Cc, 1)).view(Cc).to(DEV)


@pytest.mark.parametrize('H', R.BLUR_H)
def test_blur_finish(H):
    """F.blur_bias_act over the strip tails (H) and the wave_planes switch (W), every plane entry random (the kernel reads them all)."""
    F_ = _F()
    worst = 0.0
    for n, W in enumerate(R.BLUR_W):
        noise = ('none', 'shared', 'per')[(n + H) % 3]
        B, Cc = 2, 3
        for fir in _firs():
            t, nz, nw, b = _blur_inputs('int', B, Cc, H, W, noise)
            for bias, act in ((b, True), (None, False)):
                am = torch.zeros(B, Cc, dtype=torch.int32, device=DEV)
                y = F_.blur_bias_act(t, fir, H, W, nz, nw, bias, act, absmax_out=am, **EX)
                assert _eq(y, R.blur_ref(t, fir, nz, nw if nz is not None else None, bias, act, **EX)[0]), (H, W, noise, act)
                assert torch.equal(am, y.abs().amax((2, 3)).view(torch.int32)), (H, W, 'absmax')
            t, nz, nw, b = _blur_inputs('real', B, Cc, H, W, noise)
            am = torch.zeros(B, Cc, dtype=torch.int32, device=DEV)
            y = F_.blur_bias_act(t, fir, H, W, nz, nw, b, True, absmax_out=am)
            worst = max(worst, _ratio(y, *R.blur_ref(t, fir, nz, nw if nz is not None else None, b, True)))
            assert torch.equal(am, y.abs().amax((2, 3)).view(torch.int32))
    _say('blur H=%d' % H, ratio=worst)
    assert worst <= 1.0


def test_blur_finish_grid_stride():
    """More strips than the 8192 x 256 threads of the capped grid: the kernel strides."""
    F_ = _F()
    B, Cc, H, W = R.BLUR_STRIDE_CASE
    g = torch.Generator().manual_seed(5)
    t = torch.randint(-8, 9, (B, Cc, 4, H + 1, W + 1), generator=g).float().to(DEV)
    nz = torch.randint(-8, 9, (B, 1, 2 * H, 2 * W), generator=g).float().to(DEV)
    b = torch.randint(-8, 9, (Cc,), generator=g).float().to(DEV)
    nw = torch.tensor([3.0], device=DEV)
    fir = _firs()[1]
    am = torch.zeros(B, Cc, dtype=torch.int32, device=DEV)
    y = F_.blur_bias_act(t, fir, H, W, nz, nw, b, True, absmax_out=am, **EX)
    assert _eq(y, R.blur_ref(t, fir, nz, nw, b, True, **EX)[0])
    assert torch.equal(am, y.abs().amax((2, 3)).view(torch.int32))


@pytest.mark.parametrize('B,cin,cout,H,W', [(3, 8, 64, 9, 11), (2, 6, 10, 5, 7), (2, 8, 32, 1, 33), (1, 64, 64, 8, 8)])
def test_upsample_chain_is_conv_transpose_and_upfirdn(B, cin, cout, H, W):
    """modconv3x3(upsample=True) = UP3 + blur against the fp64 chain conv_transpose2d + upfirdn2d(pad 1,1) (what up3_ref and blur_ref
    are, tests/test_cpu_conv_edges.py), EXACT; the default configuration (split-K where the hint gives it)."""
    F_ = _F()
    c = R.C(R.UP3, B, cin, cout, H, W)
    i = _inputs(F_, 'int', c)
    nz = R.int_tensor(29, 'chn%d' % W, (B, 4 * H * W)).view(B, 1, 2 * H, 2 * W).to(DEV)
    b = R.int_tensor(29, 'chb%d' % W, (cout, 1)).view(cout).to(DEV)
    nw = torch.tensor([3.0], device=DEV)
    for fir in _firs():
        y, planes = F_.modconv3x3(i['x'], i['wp'], i['s'], i['d'], cout, upsample=True, fir=fir, noise=nz, noise_weight=nw, bias=b,
                                  activate=True, return_planes=True, **EX)
        pref = R.up3_ref(i['x'], i['wp'], i['s'], i['d'])[0]
        assert _eq(planes, pref) and _eq(y, R.blur_ref(pref, fir, nz, nw, b, True, **EX)[0])


# ------------------------------------------------------------------ ToRGB

def _torgb_inputs(kind, B, cin, H, W, skip, bias, seed=31):
    key = 'rgb.%s.%d.%d.%d.%d' % (kind, B, cin, H, W)
    if kind == 'int':
        mk = lambda k, shape: R.int_tensor(seed, key + k, tuple(shape) + (1,)).view(shape)                    # noqa: E731
        s = R.choice_tensor(seed, key + 's', (B, cin), (1.0, 2.0))
    else:
        mk = lambda k, shape: S.counter_tensor(seed, key + k, shape)                                          # noqa: E731
        s = S.counter_tensor(seed, key + 's', (B, cin), 1.0, 0.3)
    x, w = mk('x', (B, cin, H, W)), mk('w', (3, cin)).view(1, 3, cin, 1, 1)
    b = mk('b', (3, 1)).view(1, 3, 1, 1) if bias else None
    sk = mk('k', (B, 3, H // 2, W // 2)) if skip else None
    return tuple(t.to(DEV) if t is not None else None for t in (x, w, s, b, sk))


@pytest.mark.parametrize('B,cin,H,W,skip,bias', R.TORGB_CASES)
def test_torgb(B, cin, H, W, skip, bias):
    F_ = _F()
    worst = 0.0
    for fir in _firs():
        if cin in R.TORGB_EXACT_CIN:
            x, w, s, b, sk = _torgb_inputs('int', B, cin, H, W, skip, bias)
            assert _eq(F_.torgb(x, w, s, b, sk, fir if skip else None), R.torgb_ref(x, w, s, b, sk, fir)[0])
        x, w, s, b, sk = _torgb_inputs('real', B, cin, H, W, skip, bias)
        y = F_.torgb(x, w, s, b, sk, fir if skip else None)
        worst = max(worst, _ratio(y, *R.torgb_ref(x, w, s, b, sk, fir)))
        # an x view one float off 16 bytes takes the one-pixel-per-lane kernel: the same sum in another order
        buf = torch.empty(x.numel() + 1, device=DEV)
        xv = buf[1:].view(x.shape)
        xv.copy_(x)
        assert xv.data_ptr() % 16 == 4
        worst = max(worst, _ratio(F_.torgb(xv, w, s, b, sk, fir if skip else None), *R.torgb_ref(x, w, s, b, sk, fir)))
        if cin in R.TORGB_EXACT_CIN:
            x, w, s, b, sk = _torgb_inputs('int', B, cin, H, W, skip, bias)
            buf = torch.empty(x.numel() + 1, device=DEV)
            xv = buf[1:].view(x.shape)
            xv.copy_(x)
            assert _eq(F_.torgb(xv, w, s, b, sk, fir if skip else None), R.torgb_ref(x, w, s, b, sk, fir)[0])
    _say('torgb B%d %d ch %dx%d%s' % (B, cin, H, W, ' skip' if skip else ''), ratio=worst)
    assert worst <= 1.0


# ------------------------------------------------------------------ Winograd F(2x2, 3x3)

def _wino_inputs(kind, B, cin, cout, H, W, noise, bcast, seed=37):
    key = 'wn.%s.%d.%d.%d.%d.%d' % (kind, B, cin, cout, H, W)
    xshape = (1 if bcast else B, cin, H, W)
    if kind == 'int':
        x = R.int_tensor(seed, key + 'x', xshape, -4, 4)
        w = R.int_tensor(seed, key + 'w', (cout, cin, 3, 3), -2, 2) * 4
        s = R.choice_tensor(seed, key + 's', (B, cin), (1.0, 2.0))
        d = R.choice_tensor(seed, key + 'd', (B, cout), (0.5, 1.0, 2.0))
        mk = lambda k, shape: R.int_tensor(seed, key + k, shape)          # noqa: E731
        nw = torch.tensor([3.0])
    else:
        x = S.counter_tensor(seed, key + 'x', xshape)
        w = S.counter_tensor(seed, key + 'w', (cout, cin, 3, 3))
        s = S.counter_tensor(seed, key + 's', (B, cin), 1.0, 0.3)
        d = S.counter_tensor(seed, key + 'd', (B, cout), 1.0, 0.3)
        mk = lambda k, shape: S.counter_tensor(seed, key + k, shape)       # noqa: E731
        nw = torch.tensor([0.3])
    nz = None if noise == 'none' else mk('n', (1 if noise == 'shared' else B, 1, H, W))
    b = mk('b', (cout, 1)).view(cout)
    return tuple(t.to(DEV) if t is not None else None for t in (x, w, s, d, nz, nw if nz is not None else None, b))


@pytest.mark.parametrize('B,cin,cout,H,W,noise,bcast', R.wino_cases())
def test_winograd(B, cin, cout, H, W, noise, bcast):
    """F.modconv_wino (the default two-wave variant).  EXACT through a test-built pack of weights that are multiples of 4 (G w G^T
    integral) and == the direct fp32 kernel on the same weights; BOUNDED through F.prepack_wino."""
    F_ = _F()
    assert R.wino_supported(B, cin, cout, H, W) and _N().load().sgdfr_modconv2d_wino_supported(B, cin, cout, H, W)
    x, w, s, d, nz, nw, b = _wino_inputs('int', B, cin, cout, H, W, noise, bcast)
    u = R.wino_pack(w).float().contiguous()
    assert torch.equal(u, u.round())
    wp = R.wp_of(w)
    for bias, act in ((b, True), (None, False)):
        y = F_.modconv_wino(x, u, s, d, cout, nz, nw, bias, act, batch=B, **EX)
        assert _eq(y, R.plain3_ref(x, wp, s, d, nz, nw, bias, act, batch=B, **EX)[0]), (H, W, act)
        with _no_splitk(F_):
            yd = F_.modconv_raw(x, wp, s, d, cout, R.PLAIN3, H, W, noise=nz, noise_weight=nw, bias=bias, activate=act, batch=B, **EX)
        assert torch.equal(y, yd)
    x, w, s, d, nz, nw, b = _wino_inputs('real', B, cin, cout, H, W, noise, bcast)
    sc = R.wscale32(9 * cin)
    u = F_.prepack_wino(w[None])
    worst = 0.0
    for act in (False, True):
        y = F_.modconv_wino(x, u, s, d, cout, nz, nw, b, act, batch=B)
        ref, _ = R.plain3_ref(x, R.wp_of(w).double() * sc, s, d, nz, nw, b, False, batch=B)
        bound = R.wino_bound(x, w.double() * sc, s, d, nz, nw, b, batch=B)
        if act:
            ref, bound = R.apply_act(ref, bound, True, 0.2, 2 ** 0.5)
        worst = max(worst, _ratio(y, ref, bound))
    _say('wino B%d %d->%d %dx%d %s' % (B, cin, cout, H, W, R.wino_span(H, W)[1]), ratio=worst)
    assert worst <= 1.0


def test_winograd_refuses_what_its_support_rule_refuses():
    F_ = _F()
    for B, H, W in R.WINO_REFUSED:
        assert not R.wino_supported(B, 8, 64, H, W)
        with F_.using(F_.config().replace(use_winograd=True, winograd_min_blocks=0)):
            assert not F_.wino_ok(B, 8, 64, H, W) and F_.wino_ok(2, 8, 64, 2, 256)
        x, w, s, d, nz, nw, b = _wino_inputs('int', B, 8, 64, H, W, 'none', False)
        with pytest.raises(RuntimeError, match='not supported'):
            F_.modconv_wino(x, R.wino_pack(w).float().contiguous(), s, d, 64, batch=B)

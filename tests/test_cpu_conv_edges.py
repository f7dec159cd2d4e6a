"""Self-checks of the reference machinery of tests/test_gpu_conv_edges.py (tests/conv_refs.py), on the CPU: the shifted-slice fp64
references are torch's fp64 convolutions, the restated split-K and Winograd-support rules are the library's host functions, every
exact case keeps its sums below 2^24, and the case lists cross every dispatch rung and staging limit from both sides."""
import itertools

import pytest
import torch
import torch.nn.functional as TF

import conv_refs as R
from util import O, S  # noqa: F401  (puts the repository root on sys.path)

P3, U3, D3 = R.PLAIN3, R.UP3, R.DOWN3


def _w_oihw(wp):
    """packed [Cin,9,Cout] -> [Cout,Cin,3,3]"""
    return wp.permute(2, 0, 1).reshape(wp.shape[2], wp.shape[0], 3, 3).double()


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('B,cin,cout,H,W', [(2, 3, 5, 4, 6), (3, 4, 2, 1, 1), (1, 2, 3, 5, 1), (2, 5, 4, 7, 9)])
def test_references_are_torchs_fp64_convolutions(B, cin, cout, H, W):
    for kind in ('int', 'real'):
        i = R.conv_inputs(kind, P3, B, cin, cout, H, W, noise='per', bias=True)
        xs = i['x'].double() * i['s'].double()[:, :, None, None]
        want = TF.conv2d(xs, _w_oihw(i['wp']), padding=1) * i['d'].double()[:, :, None, None]
        want = want + float(i['noise_w']) * i['noise'].double() + i['bias'].double()[None, :, None, None]
        ref, bound = R.plain3_ref(**i)
        assert _close(ref, want) and bool((bound >= 0).all())
        act, _ = R.plain3_ref(act=True, slope=0.25, gain=2.0, **i)
        assert _close(act, torch.where(want > 0, want, want * 0.25) * 2.0)
        # the constant-input broadcast is the repeated batch
        ib = R.conv_inputs(kind, P3, B, cin, cout, H, W, bcast=True)
        assert torch.equal(R.plain3_ref(batch=B, **ib)[0], R.plain3_ref(**dict(ib, x=ib['x'].repeat(B, 1, 1, 1)))[0])
        # UP3: the planes interleave to conv_transpose2d; what lies outside it is exactly zero
        i = R.conv_inputs(kind, U3, B, cin, cout, H, W)
        planes, _ = R.up3_ref(i['x'], i['wp'], i['s'], i['d'])
        T = R.planes_to_full(planes)
        xs = i['x'].double() * i['s'].double()[:, :, None, None]
        wt = _w_oihw(i['wp']).permute(1, 0, 2, 3)                         # conv_transpose2d takes [Cin,Cout,3,3]
        want = TF.conv_transpose2d(xs, wt, stride=2) * i['d'].double()[:, :, None, None]
        assert want.shape[2:] == (2 * H + 1, 2 * W + 1) and _close(T[:, :, :2 * H + 1, :2 * W + 1], want)
        out = R.planes_outside(H, W)
        assert bool((planes[:, :, out] == 0).all()) and int(out.sum()) == 4 * (H + 1) * (W + 1) - (2 * H + 1) * (2 * W + 1)
        assert bool((T[:, :, 2 * H + 1] == 0).all()) and bool((T[:, :, :, 2 * W + 1] == 0).all())
        # DOWN3: the stride-2 conv of the interleaved planes
        i = R.conv_inputs(kind, D3, B, cin, cout, H, W, noise='shared', bias=True)
        Tin = R.planes_to_full(i['x'].double() * i['s'].double()[:, :, None, None, None])
        want = TF.conv2d(Tin, _w_oihw(i['wp']), stride=2)[:, :, :H, :W] * i['d'].double()[:, :, None, None]
        want = want + float(i['noise_w']) * i['noise'].double() + i['bias'].double()[None, :, None, None]
        assert _close(R.down3_ref(i['x'], i['wp'], i['s'], i['d'], i['noise'], i['noise_w'], i['bias'])[0], want)
        # blur: conv with the flipped taps over the planes padded by one; on true planes it is upfirdn2d(T, K, pad=(1,1))
        k = blur_firs()[1 if kind == 'int' else 0]
        full = R.planes_to_full(planes)
        want = TF.conv2d(TF.pad(full, (1, 0, 1, 0)).reshape(-1, 1, 2 * H + 3, 2 * W + 3), k.double().flip(0, 1)[None, None])
        got = R.blur_ref(planes, k)[0]
        assert _close(got, want.reshape(B, cout, 2 * H, 2 * W))
        assert _close(got, O.upfirdn2d(T[:, :, :2 * H + 1, :2 * W + 1], k.double(), pad=(1, 1)))
        # chained: conv_transpose2d + upfirdn2d is what modconv3x3(upsample=True) computes
        assert got.shape == (B, cout, 2 * H, 2 * W)


def blur_firs():
    """(the generator's FIR, an asymmetric integer 4x4 over 16): taps that are integers over 16."""
    sym = O.make_fir([1, 3, 3, 1], gain=4.0)
    asym = torch.tensor([[1, -2, 3, 4], [5, 6, -7, 8], [-3, 2, 1, 7], [4, -6, 5, 2]], dtype=torch.float32) / 16
    return sym, asym


def test_fir_taps_are_integers_over_sixteen():
    for k in blur_firs():
        assert torch.equal(k * 16, (k * 16).round()) and float((k * 16).abs().max()) <= 9
    a = blur_firs()[1]
    assert not torch.equal(a, a.t()) and not torch.equal(a, a.flip(0)) and not torch.equal(a, a.flip(1)) and not torch.equal(a, a.flip(0, 1))


@pytest.mark.parametrize('B,cin,H,W,skip', [(2, 5, 4, 6, True), (1, 4, 3, 5, False), (2, 16, 2, 2, True)])
def test_torgb_reference(B, cin, H, W, skip):
    x = S.counter_tensor(3, 'trx', (B, cin, H, W))
    w = S.counter_tensor(3, 'trw', (1, 3, cin, 1, 1))
    s = S.counter_tensor(3, 'trs', (B, cin))
    b = S.counter_tensor(3, 'trb', (1, 3, 1, 1))
    k = S.counter_tensor(3, 'trk', (4, 4))
    sk = S.counter_tensor(3, 'trk2', (B, 3, H // 2, W // 2)) if skip else None
    ref, bound = R.torgb_ref(x, w, s, b, sk, k)
    want = TF.conv2d(x.double() * s.double()[:, :, None, None], w.double().reshape(3, cin, 1, 1) * R.wscale32(cin)) + b.double()
    if skip:
        want = want + O.upfirdn2d(sk.double(), k.double(), up=2, pad=(2, 1))
    assert _close(ref, want) and bool((bound > 0).all())


@pytest.mark.parametrize('B,cin,cout,H,W', [(2, 3, 5, 4, 6), (3, 2, 4, 2, 2), (1, 4, 7, 6, 10)])
def test_winograd_restatement_is_the_convolution(B, cin, cout, H, W):
    """The restated pack, un-swizzled, run through F(2x2,3x3) in fp64 gives the plain conv; its absolute-value form bounds it."""
    w = S.counter_tensor(5, 'wgw', (cout, cin, 3, 3))
    x = S.counter_tensor(5, 'wgx', (B, cin, H, W))
    s = S.counter_tensor(5, 'wgs', (B, cin), 1.0, 0.3)
    u = R.wino_pack(w).reshape(cin, cout, 4, 4)
    o = torch.arange(cout)
    un = torch.stack([u[:, o, a ^ (o & 3)] for a in range(4)], 2)                   # quad a back from slot a ^ (o & 3)
    assert _close(un, torch.einsum('ak,oikl,bl->ioab', R.WG, w.double(), R.WG))
    xs = TF.pad(x.double() * s.double()[:, :, None, None], (1, 1, 1, 1))
    pt = xs.unfold(2, 4, 2).unfold(3, 4, 2)
    V = torch.einsum('ak,bihwkl,cl->bihwac', R.WBT, pt, R.WBT)
    M = torch.einsum('bihwac,ioac->bohwac', V, un)
    Y = torch.einsum('pa,bohwac,qc->bohpwq', R.WAT, M, R.WAT).reshape(B, cout, H, W)
    ref, bound = R.plain3_ref(x, R.wp_of(w), s)
    assert _close(Y, ref)
    wb = R.wino_bound(x, w, s)
    assert bool((wb >= bound * (cin + 20) / (9 * cin + 8) * (1 - 1e-12)).all())       # |Winograd| dominates the direct magnitude
    # integer pack: weights that are multiples of 4 give integral G w G^T
    wi = R.int_tensor(5, 'wgi', (cout, cin * 9), -2, 2).view(cout, cin, 3, 3) * 4
    ui = R.wino_pack(wi)
    assert torch.equal(ui, ui.round()) and float(ui.abs().max()) <= 18


def test_restated_host_rules_are_the_librarys():
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    n = 0
    for B, cin, cout, H, W, mode in itertools.product((1, 2, 3, 5, 47, 48, 191, 192), (4, 6, 32, 64, 68, 160, 512), (4, 32, 36, 64, 512),
                                                      (1, 4, 8, 31), (1, 4, 8, 33), (P3, U3, D3)):
        assert R.splitk_hint(B, cin, cout, H, W, mode) == lib.sgdfr_modconv2d_splitk_hint(B, cin, cout, H, W, mode), (B, cin, cout, H, W, mode)
        n += 1
    for cin, cout, H, W in itertools.chain(
            itertools.product((8, 12, 64), (64, 96, 128), (1, 2, 3, 4, 6, 16, 40, 64, 128), range(1, 300)),
            itertools.product((8,), (64,), (2, 4, 8, 64, 512), range(300, 1100, 2))):
        assert R.wino_supported(2, cin, cout, H, W) == lib.sgdfr_modconv2d_wino_supported(2, cin, cout, H, W), (cin, cout, H, W)
        n += 1
    assert n > 10000
    for case in R.SPLITK_RAW_CASES:
        mode, B, cin, cout, H, W, _, want = case
        assert lib.sgdfr_modconv2d_splitk_hint(B, cin, cout, H, W, mode) == want, case


def _all_modconv_cases():
    return R.PLAIN_CASES + R.DIRECT_CASES + [R.DIRECT_STRIDE_CASE] + R.UP_CASES + R.DOWN_CASES


def test_every_exact_case_keeps_its_sums_below_two_to_the_24():
    """A priori, from the value ranges alone (conv_refs.exact_condition): 9 Cin max|x s| max|w| max|d| + |noise term| + |bias|."""
    for c in _all_modconv_cases():
        assert R.exact_condition(c['cin']), R.case_id(c)
        assert 9 * c['cin'] * (8 * 2) * 8 * 2 + 8 * 3 + 8 < 2 ** 24            # the condition as the issue words it
    for case in R.SPLITK_RAW_CASES + R.SPLITK_DIRECT_CASES:
        assert R.exact_condition(case[2]), case
    for cin in (3, 4, 16, 20, 64, 256, 512):
        assert R.exact_condition(cin, taps=1, s=(1.0, 2.0), d=1.0, noise=16 * 8 * 16, bias=8)   # ToRGB (skip: 16 taps of 8 * k/16, in 1/16)
    assert 16 * 16 * 8 * 9 + 16 * (8 * 3 + 8) < 2 ** 24                        # blur, in units of 1/16: 16 taps, |T| <= 8, |16 k| <= 9
    for B, cin, cout, H, W, _, _ in R.wino_cases():
        assert R.wino_exact_condition(cin) and R.exact_condition(cin, x=4, w=8, s=(1.0, 2.0))
    # the inputs are what the condition assumes
    i = R.conv_inputs('int', P3, 3, 8, 36, 5, 7, noise='per', bias=True)
    assert float(i['x'].abs().max()) <= 8 and float(i['wp'].abs().max()) <= 8 and set(i['s'].unique().tolist()) <= {0.5, 1.0, 2.0}
    assert set(i['d'].unique().tolist()) <= {0.5, 1.0, 2.0} and float(i['noise'].abs().max()) <= 8 and float(i['noise_w']) == 3.0
    assert float(i['x'].view(-1)[0]) != 0 and float(i['x'].view(-1)[-1]) != 0 and float(i['wp'].view(-1)[-1]) != 0


def test_fp32_on_the_cpu_meets_the_bound_and_is_exact_on_integers():
    """torch's own fp32 convolution as a stand-in kernel: exact on the integer inputs, inside the a-priori bound on the real ones."""
    for cin, cout, H, W in ((8, 36, 9, 11), (64, 32, 5, 7)):
        i = R.conv_inputs('int', P3, 3, cin, cout, H, W, noise='per', bias=True)
        y = TF.conv2d(i['x'] * i['s'][:, :, None, None], _w_oihw(i['wp']).float(), padding=1) * i['d'][:, :, None, None]
        y = y + i['noise_w'] * i['noise'] + i['bias'][None, :, None, None]
        assert torch.equal(y, R.plain3_ref(**i)[0].float())
        i = R.conv_inputs('real', P3, 3, cin, cout, H, W, noise='per', bias=True)
        y = TF.conv2d(i['x'] * i['s'][:, :, None, None], _w_oihw(i['wp']).float(), padding=1) * i['d'][:, :, None, None]
        y = y + i['noise_w'] * i['noise'] + i['bias'][None, :, None, None]
        assert R.ratio(y, *R.plain3_ref(**i)) <= 1.0


def test_the_sweeps_cross_every_dispatch_edge():
    """From the restated rules (conv_refs.tile_of / staged / wino_span, citing csrc/modconv.hip:585-611, :660-695 and csrc/wino.hip:624-649):
    every tile instantiation, each pixel-count threshold from both sides, the staging limits from both sides, the segment switch, every
    rows / images-crossed branch, the direct kernel, every Winograd branch."""
    def plans(cases):
        return [R.plan(c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W']) for c in cases]
    tiles = {(m, t) for m, cs in ((P3, R.PLAIN_CASES), (U3, R.UP_CASES), (D3, R.DOWN_CASES)) for t, _ in plans(cs)}
    assert {(P3, t) for t in ((128, 128, 3), (64, 256, 4), (64, 128, 3), (64, 64, 3), (32, 128, 3))} <= tiles
    assert {(U3, t) for t in ((128, 64, 3), (64, 64, 3), (32, 128, 3))} <= tiles
    assert {(D3, t) for t in ((128, 128, 3), (64, 64, 3), (32, 128, 3))} <= tiles
    assert all(R.plan(c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W'])[0] == 'direct' for c in R.DIRECT_CASES)
    assert {c['mode'] for c in R.DIRECT_CASES} == {P3, U3, D3}
    c = R.DIRECT_STRIDE_CASE
    assert c['B'] * c['cout'] * c['H'] * c['W'] > 4096 * 256 and R.tile_of(P3, c['B'], c['cin'], c['cout'], c['H'], c['W']) == 'direct'

    def t(mode, B, cin, cout, H, W):
        return R.tile_of(mode, B, cin, cout, H, W)
    # the thresholds, one step below and at (the pairs of the case lists)
    assert t(P3, 1, 4, 128, 255, 256) == (64, 64, 3) and t(P3, 1, 4, 128, 256, 256) == (128, 128, 3)
    assert t(P3, 1, 4, 256, 255, 128) == (64, 64, 3) and t(P3, 2, 4, 256, 128, 128) == (128, 128, 3) and 255 * 128 == 32641 - 1
    assert t(P3, 1, 4, 64, 255, 256) == (64, 64, 3) and t(P3, 1, 4, 64, 256, 256) == (64, 128, 3)
    for co in (64, 192):
        assert t(P3, 3, 4, co, 256, 256) == (64, 128, 3) and t(P3, 4, 4, co, 256, 256) == (64, 256, 4)
    assert t(U3, 2, 4, 128, 127, 126) == (64, 64, 3) and t(U3, 2, 4, 128, 127, 127) == (128, 64, 3)
    assert t(D3, 1, 4, 128, 255, 256) == (64, 64, 3) and t(D3, 1, 4, 128, 256, 256) == (128, 128, 3)
    ids = {R.case_id(c) for c in R.PLAIN_CASES + R.UP_CASES + R.DOWN_CASES}
    for want in ('plain-B1-4to128-255x256', 'plain-B1-4to128-256x256', 'plain-B1-4to256-255x128', 'plain-B2-4to256-128x128',
                 'plain-B1-4to64-255x256', 'plain-B1-4to64-256x256', 'plain-B3-4to64-256x256', 'plain-B4-4to64-256x256',
                 'plain-B3-4to192-256x256', 'plain-B4-8to192-256x256', 'up-B2-4to128-127x126', 'up-B2-4to128-127x127',
                 'down-B1-4to128-255x256', 'down-B1-4to128-256x256'):
        assert want in ids, want
    assert {c['cout'] for c in R.PLAIN_TILE_CASES} >= {4, 32, 36, 100, 132} and {c['cin'] for c in R.PLAIN_K_CASES} == {4, 8, 12, 64}
    # rows / images crossed: each of the three branches of both, for the 64- and the 128-pixel tile
    for PT in (64, 128):
        seen_r, seen_i = set(), set()
        for (tl, st), c in zip(plans(R.PLAIN_CASES), R.PLAIN_CASES):
            if tl != 'direct' and tl[1] == PT and not st['seg']:
                W, HW = c['W'], c['H'] * c['W']
                seen_r.add('zero' if W % PT == 0 else 'whole' if PT % W == 0 else 'general')
                seen_i.add('zero' if HW % PT == 0 else 'whole' if PT % HW == 0 else 'general')
        assert seen_r == {'zero', 'whole', 'general'} and seen_i == {'zero', 'whole', 'general'}, (PT, seen_r, seen_i)
    assert all(c['H'] * c['W'] % 128 and c['H'] * c['W'] % 64 for c in R.PLAIN_STRADDLE_CASES if c['B'] == 3)
    assert {c['W'] for c in R.PLAIN_STRADDLE_CASES} >= {1, 2, 3, 5, 19, 33, 63, 65}
    assert max(st['imgs'] for _, st in plans(R.PLAIN_STRADDLE_CASES)) == 31        # many images in one tile (2x2 at B = 70)
    # the segment switch, both sides on both tiles
    seg = {(tl[1], c['W'], st['seg']) for (tl, st), c in zip(plans(R.PLAIN_SEG_CASES), R.PLAIN_SEG_CASES)}
    assert seg == {(64, 128, True), (64, 256, True), (128, 256, True), (64, 64, False), (128, 128, False)}
    assert R.plan(P3, 1, 4, 128, 256, 256)[1]['seg'] and R.plan(P3, 4, 4, 64, 256, 256)[1] == dict(rows=0, imgs=0, xlen=772, seg=False, ok=True)
    # the staging limits: the widest accepted image and the first refused one
    assert R.first_refused_w(P3, 2, 8, 64, 1) == 233 and R.first_refused_w(P3, 2, 8, 64, 3) == 233
    assert R.first_refused_w(P3, 2, 8, 32, 3) == 212 and R.first_refused_w(D3, 2, 8, 64, 3) == 350 and R.first_refused_w(D3, 2, 8, 32, 3) == 318
    assert R.plan(P3, 1, 4, 64, 64, 349)[1]['xlen'] == 767 and not R.plan(P3, 1, 4, 64, 64, 350)[1]['ok']
    assert R.plan(P3, 2, 8, 64, 3, 232)[1]['xlen'] == 766 and R.plan(P3, 2, 8, 32, 3, 211)[1]['xlen'] == 767
    # UP3: xlen = PT + P + 2 with P = W + 1, so 64 + 702 + 2 = 768 is still accepted: W = 701 is the last, 702 the first refused
    assert R.first_refused_w(U3, 2, 4, 64, 1) == 702 and R.first_refused_w(U3, 2, 4, 32, 1) == 638
    for mode, cases, refused in ((P3, R.PLAIN_LIMIT_CASES, R.PLAIN_REFUSED), (U3, R.UP_CASES, R.UP_REFUSED), (D3, R.DOWN_CASES, R.DOWN_REFUSED)):
        ok = {(c['B'], c['cin'], c['cout'], c['H'], c['W']) for c in cases}
        for B, cin, cout, H, W in refused:
            assert not R.plan(mode, B, cin, cout, H, W)[1]['ok'], (mode, W)
            assert (B, cin, cout, H, W - 1) in ok and R.plan(mode, B, cin, cout, H, W - 1)[1]['ok'], (mode, W)
    assert all(st is None or st['ok'] for _, st in plans(_all_modconv_cases()))
    # Winograd: every branch of wino_span, nex 1 and 2, simgs 1 ... 65, both sides of the limit at H = 2
    br = {R.wino_span(H, W)[1] for _, H, W in R.WINO_SHAPES}
    assert br == {'row', 'rows', 'general'}
    nex = {(R.wino_xlen(H, W) + 511) // 512 for _, H, W in R.WINO_SHAPES}
    sim = {R.wino_simgs(H, W) for _, H, W in R.WINO_SHAPES}
    assert nex == {1, 2} and {1, 65} <= sim and len(sim) >= 5 and R.wino_xlen(4, 4) == 504
    assert all(R.wino_supported(B, 8, 64, H, W) for B, H, W in R.WINO_SHAPES) and not any(R.wino_supported(B, 8, 64, H, W) for B, H, W in R.WINO_REFUSED)
    assert max(W for W in range(2, 2000, 2) if R.wino_supported(2, 8, 64, 2, W)) == 256 and (2, 2, 256) in R.WINO_SHAPES and (2, 2, 258) in R.WINO_REFUSED
    assert R.wino_xlen(2, 144) == 1022 and R.wino_xlen(2, 146) > 1024
    assert any(B * (H // 2) * (W // 2) % 64 for B, H, W in R.WINO_SHAPES)          # a partial last tile block
    assert {c[1] for c in R.wino_cases()} == {8, 16, 64} and {c[2] for c in R.wino_cases()} == {64, 128}
    # blur, ToRGB
    assert {((h + 3) // 4 * w) % 64 == 0 for h in R.BLUR_H for w in R.BLUR_W} == {True, False}
    B, Cc, H, W = R.BLUR_STRIDE_CASE
    assert B * Cc > 4096 and B * Cc * W > 256 * 32 * 256
    groups = {(H * W // 4 if H * W % 4 == 0 else H * W) for _, _, H, W, _, _ in R.TORGB_CASES}
    assert {1, 3, 4, 5, 63, 64, 65} <= groups and {c[1] for c in R.TORGB_CASES} == {3, 4, 16, 20, 64, 256, 512}
    assert all(R.wscale32(c) * R.wscale32(c) * c == 1.0 and (c ** 0.5) % 1 == 0 for c in R.TORGB_EXACT_CIN)

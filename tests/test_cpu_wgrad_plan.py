"""CPU: the host split-K plan of csrc/wgrad.hip against its restatement (tests/wgrad_restatement.py), the restatement's tap and flip
convention against the whole-layer oracle, and the coverage condition over the shapes tests/test_gpu_wgrad_edges.py runs."""
import itertools
import math

import pytest
import torch

from util import O, S
import wgrad_restatement as R


def _ksplit(case):
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    B, Cin, Cout, H, W, up = case
    return lib.sgdfr_modconv_wgrad_ksplit(B, Cin, Cout, H, W, _native.MODE_UP3 if up else _native.MODE_PLAIN3)


def _want(case):
    p = R.plan(*case)
    return 0 if p is None else p['K']


def test_plan_matches_the_c_abi_on_the_cases_and_a_sweep():
    for case in R.CASES:
        assert _ksplit(case) == _want(case), case
    n = 0
    for B, H, W, Cin, Cout, up in itertools.product(range(1, 6), range(1, 10), (3, 4, 5, 6, 8, 12, 16, 32, 64, 96, 128, 192),
                                                    (6, 33, 64, 65), (6, 33, 64, 65), (0, 1)):
        case = (B, Cin, Cout, H, W, up)
        assert _ksplit(case) == _want(case), case
        n += 1
    assert n == 5 * 9 * 12 * 16 * 2
    # what the library refuses is no plan either
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    assert lib.sgdfr_modconv_wgrad_ksplit(0, 8, 8, 4, 4, 0) == 0 and lib.sgdfr_modconv_wgrad_ksplit(1, 8, 8, 0, 4, 0) == 0


def test_plan_of_the_named_cases():
    """The plan figures the case table was chosen for, written out."""
    def fig(case):
        p = R.plan(*case)
        return None if p is None else (p['ntile'], p['K'], p['ragged'], p['straddle'], p['capped'])
    assert fig((1, 8, 8, 4, 4, 0)) == (1, 1, False, False, False)
    assert fig((4, 8, 8, 1, 4, 0)) == (1, 1, False, True, False)
    assert fig((1, 8, 8, 8, 4, 0)) == (1, 2, False, False, False)
    assert fig((3, 8, 8, 3, 4, 0)) == (1, 3, False, False, False)
    assert fig((5, 16, 8, 4, 4, 1)) == (1, 5, False, False, False)
    assert fig((17, 6, 6, 1, 4, 1)) == (1, 5, True, True, False)
    assert fig((1, 6, 6, 21, 4, 0)) == (1, 6, True, False, False)
    assert fig((1, 33, 31, 5, 4, 1)) == (1, 2, True, False, False)
    assert fig((1, 16, 8, 7, 8, 0)) == (1, 2, True, False, False)
    assert fig((3, 16, 8, 5, 8, 0)) == fig((3, 16, 8, 5, 8, 1)) == (1, 4, True, True, False)
    assert fig((3, 40, 24, 9, 8, 0)) == fig((2, 24, 40, 13, 8, 1)) == (1, 7, True, True, False)
    assert fig((2, 65, 70, 5, 16, 0)) == fig((2, 70, 65, 5, 16, 1)) == (4, 3, True, True, False)
    assert R.plan(1, 8, 8, 3, 192, 0)['chunks_per_row'] == R.plan(1, 8, 8, 3, 96, 1)['chunks_per_row'] == 3
    assert fig((1, 8, 8, 4, 4, 1))[1] == 1 and fig((2, 16, 16, 9, 64, 1))[1] == 9
    assert fig((2, 192, 192, 57, 64, 0)) == (9, 29, True, True, False)
    assert fig((1, 512, 512, 2, 4, 0)) == (64, 1, False, False, False)
    assert fig((5, 512, 512, 16, 16, 0)) == (64, 16, False, True, True)         # 80 chunks in slices of 5, images of 16
    for case in ((1, 8, 8, 3, 96, 0), (2, 8, 8, 4, 6, 0), (2, 6, 10, 3, 5, 1), (1, 512, 512, 3, 3, 0)):
        assert R.plan(*case) is None
    # K = 5 and 7 leave the four slice groups of the oik finish unequal counts, K = 1 and 2 leave groups without a slice
    assert [len(range(kg, 5, 4)) for kg in range(4)] == [2, 1, 1, 1] and [len(range(kg, 7, 4)) for kg in range(4)] == [2, 2, 2, 1]
    assert [len(range(kg, 2, 4)) for kg in range(4)] == [1, 1, 0, 0]


def _classes():
    """name -> predicate(case, plan or None) of the coverage condition."""
    c = {}
    for up, mode in ((0, 'plain'), (1, 'up')):
        def mfma(f, up=up):
            return lambda case, p: case[5] == up and p is not None and f(case, p)
        c[mode + ' K = 1'] = mfma(lambda case, p: p['K'] == 1)
        c[mode + ' K = 2'] = mfma(lambda case, p: p['K'] == 2)
        c[mode + ' K = 5 or 7'] = mfma(lambda case, p: p['K'] in (5, 7))
        c[mode + ' K > 8'] = mfma(lambda case, p: p['K'] > 8)
        c[mode + ' ragged'] = mfma(lambda case, p: p['ragged'])
        c[mode + ' straddle'] = mfma(lambda case, p: p['straddle'])
        c[mode + ' three chunks per row'] = mfma(lambda case, p: p['chunks_per_row'] == 3)
        c[mode + ' W = 4, H != 4'] = mfma(lambda case, p: case[4] == 4 and case[3] != 4)
        c[mode + ' direct'] = (lambda case, p, up=up: case[5] == up and p is None)
    c['plain H = 1'] = lambda case, p: case[5] == 0 and p is not None and case[3] == 1
    c['plain direct W = 96'] = lambda case, p: case[5] == 0 and p is None and case[4] == 96
    c['capped'] = lambda case, p: p is not None and p['capped']
    c['Cin % 64 = 1'] = lambda case, p: p is not None and case[1] % 64 == 1
    c['Cout % 64 = 6'] = lambda case, p: p is not None and case[2] % 64 == 6
    c['33..63 channels'] = lambda case, p: p is not None and (33 <= case[1] <= 63 or 33 <= case[2] <= 63)
    c['MFMA under 32 channels'] = lambda case, p: p is not None and (case[1] < 32 or case[2] < 32)
    c['512 x 512 MFMA'] = lambda case, p: p is not None and case[1] * case[2] * 9 > 4096 * 256
    c['512 x 512 direct'] = lambda case, p: p is None and case[1] * case[2] * 9 > 4096 * 256
    return c


def missing(cases):
    """The classes of the coverage condition that no case of `cases` shows."""
    classes = _classes()
    plans = [(case, R.plan(*case)) for case in cases]
    return sorted(name for name, pred in classes.items() if not any(pred(case, p) for case, p in plans))


def test_cases_cover_every_seam():
    """The coverage condition over the GPU case table: nobody thins the table without noticing."""
    assert len(set(R.CASES)) == len(R.CASES)
    for case in R.CASES:
        p = R.plan(*case)
        print(R.case_id(case), 'direct' if p is None else ' '.join('%s=%s' % kv for kv in p.items()))
    assert missing(R.CASES) == []
    # every case is small: x and g together stay under 12 MB (the largest is the K = 29 case)
    for B, Cin, Cout, H, W, up in R.CASES:
        assert 4 * B * (Cin + Cout * (4 if up else 1)) * (H + up) * (W + up) <= 12 << 20
    # the condition has teeth: for every class, the table without the cases that show it fails on that class
    classes = _classes()
    for name, pred in classes.items():
        thinned = [case for case in R.CASES if not pred(case, R.plan(*case))]
        assert len(thinned) < len(R.CASES) and name in missing(thinned), name


def test_planes_and_image_are_inverse():
    img = S.counter_tensor(41, 'wgp.img', (2, 3, 7, 9)).double()
    planes = R.image_to_planes(img, outside=1e30)
    assert planes.shape == (2, 3, 4, 4, 5)
    assert torch.equal(R.planes_to_image(planes), img)
    out = R.outside_mask(3, 4)
    assert int(out.sum()) == 2 * 5 + 2 * 4 - 1 and bool((planes[:, :, out] == 1e30).all()) and bool((planes[:, :, ~out] != 1e30).all())
    assert float(planes[1, 2, 3, 2, 1]) == float(img[1, 2, 5, 3])          # plane 2*1+1, row 2, col 1 -> pixel (5, 3)


@pytest.mark.parametrize('up', [False, True])
def test_tap_and_flip_convention_against_the_whole_layer_oracle(up):
    """finish64(dwc64(g, d, x, s), w, dq64(a, d, s)) is dL/dW of oracle.styled_conv, with g = dL/d(conv output) (plain) or the parity
    planes of dL/d(transposed-conv output) (up), d the demodulation factors and a = d * dL/dd = sum_p g * out.  Asymmetric sizes and
    channel counts, so a transposed or flipped tap, a swapped parity plane or swapped channel axes cannot pass."""
    B, Cin, Cout, H, W, D = 2, 5, 3, 4, 6, 7
    key = 'wgp.pin.%d.' % up
    names = ('conv.weight', 'conv.modulation.weight', 'conv.modulation.bias', 'noise.weight', 'activate.bias')
    shapes = ((1, Cout, Cin, 3, 3), (Cin, D), (Cin,), (1,), (Cout,))
    P = {'L.' + n: S.counter_tensor(41, key + n, sh).double() for n, sh in zip(names, shapes)}
    P['L.conv.modulation.bias'] = P['L.conv.modulation.bias'] * 0.1 + 1.0
    P['L.conv.weight'].requires_grad_(True)
    x = S.counter_tensor(41, key + 'x', (B, Cin, H, W)).double()
    style = S.counter_tensor(41, key + 'style', (B, D)).double()
    r = 2 if up else 1
    noise = S.counter_tensor(41, key + 'noise', (B, 1, r * H, r * W)).double()
    gy = S.counter_tensor(41, key + 'gy', (B, Cout, r * H, r * W)).double()
    (O.styled_conv(P, 'L', x, style, noise, upsample=up) * gy).sum().backward()
    want = P['L.conv.weight'].grad[0]

    # the same layer once more in pieces, for the gradient at the conv output
    w = P['L.conv.weight'].detach()
    s = O.equal_linear(style, P['L.conv.modulation.weight'], P['L.conv.modulation.bias'])
    d = torch.rsqrt(((w * R.scale_of(Cin)) ** 2 * (s * s).view(B, 1, Cin, 1, 1)).sum([2, 3, 4]) + 1e-8)
    out = O.modulated_conv2d(x, style, w, P['L.conv.modulation.weight'], P['L.conv.modulation.bias'], upsample=up).requires_grad_(True)
    (O.fused_leaky_relu(out + P['L.noise.weight'] * noise, P['L.activate.bias']) * gy).sum().backward()
    g = out.grad
    a = (g * out.detach()).sum([2, 3])
    if up:          # through the blur: the adjoint of a linear map is its autograd gradient at any point
        T = torch.zeros(B, Cout, 2 * H + 1, 2 * W + 1, dtype=torch.float64, requires_grad=True)
        (O.upfirdn2d(T, O.make_fir([1, 3, 3, 1], gain=4.0, dtype=torch.float64), pad=O.up_blur_pad()) * g).sum().backward()
        g = R.image_to_planes(T.grad)
        assert g.shape == (B, Cout, 4, H + 1, W + 1)
    got = R.finish64(R.dwc64(g, d, x, s, up), w, R.dq64(a, d, s))
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print('up=%d: max |restatement - oracle| %.3e of %.3e' % (up, err, top))
    assert err <= 1e-12 * top
    # the demodulation term is no rounding matter: without it the two differ visibly
    assert float((R.finish64(R.dwc64(g, d, x, s, up), w, None) - want).abs().max()) > 1e-3 * top
    # |.| form: an upper bound of the signed one, elementwise
    assert bool((R.absdwc64(g, d, x, s, up) >= R.dwc64(g, d, x, s, up).abs() - 1e-12).all())
    # x with one row is the broadcast input
    x1 = x[:1]
    assert torch.equal(R.dwc64(g, d, x1, s, up), R.dwc64(g, d, x1.expand(B, -1, -1, -1).contiguous(), s, up))
    assert math.isclose(R.scale_of(Cin), 1 / math.sqrt(45))

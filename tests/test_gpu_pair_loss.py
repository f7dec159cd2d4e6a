"""GPU: the kernels of csrc/pairloss.hip through pair_loss.py, alone -- against the reference's fixture kat19 and, at the sizes the
fixture does not hold, against the float64 restatement tests/pair_loss_restatement.py evaluated on the device.

Sizes: the fixture's [2,3,32,32] and [2,14,512]; n = 7 (less than one vector per thread, less than one wave); [2,3,31,33] (n = 6138,
not a multiple of 4: a tail); a view whose storage offset breaks 16-byte alignment (the dword path); [1,3,256,256] (48 blocks of
partials); 2048 tiles and a bit (the grid-stride loop, entered above 2048 tiles only); and 2^31 + 4099 elements (indices past int32).

Bars: pair_loss_restatement.T_ABS / MEAN_REL / GRAD_REL, as tests/test_cpu_pair_loss.py derives them.  Exact: a gradient of 0 where x
was clamped, a non-zero one at x = +-1, only s * g255 where x == y, and equal bits from two runs -- and from the 16-byte and the
dword path, whose additions are ordered alike.  Every test prints the figures it asserts on.
"""
import pytest
import torch

from util import golden, t
import pair_loss_restatement as R

pytestmark = pytest.mark.gpu

KAT = 'kat19_paired_losses.npz'
TILE = 4096
SHAPES = {'n7': (7,), 'tail': (2, 3, 31, 33), 'fixture_image': (2, 3, 32, 32), 'latents': (2, 14, 512), 'blocks48': (1, 3, 256, 256),
          'grid_stride': (2048 * TILE + 3 * TILE + 5,)}
PLANTED = ((0, 1.0, 0.3), (1, -1.0, 0.2), (2, 1.5, 2.0), (3, -2.0, -1.0), (4, 0.25, 0.25), (5, -0.5, -0.5))     # index, x, y


def PL():
    from stylegan_directions_face_reenactment_amd import pair_loss
    return pair_loss


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(shape, seed, misaligned=False):
    """x, y ~ N(0, 0.8^2) with the planted values of the fixture at flat indices 0..5, and a weight image c; with `misaligned`
    each is a contiguous view one float into a longer buffer: 4-byte aligned, not 16."""
    gen = torch.Generator().manual_seed(seed)
    n = 1
    for d in shape:
        n *= d
    x, y, c = torch.randn(n, generator=gen) * 0.8, torch.randn(n, generator=gen) * 0.8, torch.randn(n, generator=gen)
    if n >= 6:
        for i, vx, vy in PLANTED:
            x[i], y[i] = vx, vy
    out = []
    for v in (x, y, c):
        if misaligned:
            buf = torch.empty(n + 1, device='cuda')
            buf[1:].copy_(v)
            v = buf[1:]
        else:
            v = v.cuda()
        assert (v.data_ptr() % 16 != 0) == misaligned and v.is_contiguous()
        out.append(v.view(shape))
    return out


def _check_planted(x, dx, c, g255_given):
    xf, df = x.reshape(-1), dx.reshape(-1)
    assert xf[0] == 1 and xf[1] == -1 and bool((df[:2] != 0).all())               # the clamp's bounds pass gradient
    assert bool((df[2:4] == 0).all()) and not bool(torch.signbit(df[2:4]).any())  # x clamped: exactly +0
    # x == y: sign(0) = 0, only s * g255 passes -- (g255 * 255) / (2 + 1e-5) as torch's CPU kernels round it (true division)
    want = (c.reshape(-1)[4:6].cpu() * 255.0) / 2.00001 if g255_given else torch.zeros(2)
    assert _bits(df[4:6].cpu(), want), (df[4:6], want)


def test_fixture_images_losses_and_gradients():
    g = golden(KAT)
    x, y, c, lat, tw = (t(g[k]).cuda() for k in ('x', 'y', 'c', 'lat', 'tw'))
    x.requires_grad_(True)
    loss, x255, y255 = PL().pixel_wise_255(x, y, True)
    assert loss.dim() == 0 and loss.is_cuda and x255.shape == x.shape and not y255.requires_grad and x255.requires_grad
    (float(g['g_pw']) * loss + (c * x255).sum()).backward()
    et = max(float((x255.detach().cpu().double() - t(g['tx']).double()).abs().max()), float((y255.cpu().double() - t(g['ty']).double()).abs().max()))
    same = int((x255.detach().cpu() == t(g['tx'])).sum()) + int((y255.cpu() == t(g['ty'])).sum())
    ep = abs(float(loss.detach()) - float(g["pw"])) / float(g["pw"])
    eg = R.rel(x.grad, t(g['gx']))
    lat.requires_grad_(True)
    wreg = PL().l1_mean(lat, tw)
    (float(g['g_wreg']) * wreg).backward()
    ew, el = abs(float(wreg.detach()) - float(g['wreg'])) / float(g['wreg']), R.rel(lat.grad, t(g['glat']))
    print('fixture: t %.3e (bar %.3e; %d of %d values bit-equal to the reference); pw %.3e, wreg %.3e (bar %.0e); gx %.3e, glat %.3e (bar %.0e)'
          % (et, R.T_ABS, same, 2 * x.numel(), ep, ew, R.MEAN_REL, eg, el, R.GRAD_REL))
    assert et <= R.T_ABS and ep <= R.MEAN_REL and ew <= R.MEAN_REL and eg <= R.GRAD_REL and el <= R.GRAD_REL
    gx = x.grad.reshape(-1).cpu()
    assert (gx[t(g['clamped_idx'])] == 0).all() and (gx[t(g['bound_idx'])] != 0).all()
    assert _bits(gx[t(g['equal_idx'])], t(g['gx']).reshape(-1)[t(g['equal_idx'])])          # only s * g255: (c * 255) / (2 + 1e-5)
    assert (lat.grad[0, 0, :3] == 0).all() and (lat.grad[1, 13, 500:] == 0).all()


# (the dword path at the grid-stride size adds nothing the smaller sizes do not show)
@pytest.mark.parametrize('name,misaligned', [(k, m) for k in SHAPES for m in (False, True) if not (m and k == 'grid_stride')])
def test_range255_against_the_restatement(name, misaligned):
    """pixel_wise_255 with and without the images and with and without an upstream image gradient, forward and backward against
    the float64 restatement (closed-form gradient) on the device; two runs give the same bits."""
    shape = SHAPES[name]
    x, y, c = _inputs(shape, 11, misaligned)
    n, g = x.numel(), 0.37
    want_loss, tx, ty = R.pixel_wise(x, y), R.t(x), R.t(y)
    for want_images, use_g255, use_loss in ((True, True, True), (True, False, True), (False, False, True), (True, True, False)):
        runs = []
        for _ in range(2):
            xr = x.detach().requires_grad_(True)
            loss, x255, y255 = PL().pixel_wise_255(xr, y, want_images)
            assert (x255 is None) == (y255 is None) == (not want_images)
            total = (g * loss if use_loss else 0) + ((c * x255).sum() if use_g255 else 0)
            total.backward()
            runs.append((loss.detach(), x255, y255, xr.grad))
        (loss, x255, y255, dx), again = runs
        assert _bits(loss, again[0]) and _bits(dx, again[3])
        ep = abs(float(loss) - float(want_loss)) / float(want_loss)
        want_dx = R.pixel_wise_grad(x, y, g if use_loss else 0.0, c if use_g255 else None)
        eg = R.rel(dx, want_dx)
        et = 0.0
        if want_images:
            assert _bits(x255.detach(), again[1].detach()) and _bits(y255, again[2])
            et = max(float((x255.detach().double() - tx).abs().max()), float((y255.double() - ty).abs().max()))
        print('%s%s n=%d images=%s g255=%s g=%s: loss rel %.3e (bar %.0e), t %.3e (bar %.3e), dx rel %.3e (bar %.0e)'
              % (name, ' misaligned' if misaligned else '', n, want_images, use_g255, use_loss, ep, R.MEAN_REL, et, R.T_ABS, eg, R.GRAD_REL))
        assert ep <= R.MEAN_REL and et <= R.T_ABS and eg <= R.GRAD_REL
        if n >= 6:
            _check_planted(x, dx, c, use_g255)


@pytest.mark.parametrize('name', list(SHAPES))
def test_plain_against_the_restatement(name):
    shape = SHAPES[name]
    for misaligned in (False, True):
        x, y, _ = _inputs(shape, 12, misaligned)
        runs = []
        for _ in range(2):
            xr = x.detach().requires_grad_(True)
            loss = PL().l1_mean(xr, y)
            (0.61 * loss).backward()
            runs.append((loss.detach(), xr.grad))
        (loss, dx), again = runs
        assert _bits(loss, again[0]) and _bits(dx, again[1])
        ep = abs(float(loss) - float(R.l1_mean(x, y))) / float(R.l1_mean(x, y))
        eg = R.rel(dx, R.l1_mean_grad(x, y, 0.61))
        print('%s%s n=%d plain: loss rel %.3e (bar %.0e), dx rel %.3e (bar %.0e)' % (name, ' misaligned' if misaligned else '', x.numel(), ep,
                                                                                      R.MEAN_REL, eg, R.GRAD_REL))
        assert ep <= R.MEAN_REL and eg <= R.GRAD_REL
        if x.numel() >= 6:
            assert bool((dx.reshape(-1)[4:6] == 0).all()) and bool((dx.reshape(-1)[:4] != 0).all())      # sign(0) = 0; no clamp here


def test_aligned_and_misaligned_calls_give_the_same_bits():
    """The element -> thread assignment depends on n alone: the dword path adds the same numbers in the same order."""
    for name in ('tail', 'blocks48'):
        xa, ya, ca = _inputs(SHAPES[name], 13, False)
        xm, ym, cm = _inputs(SHAPES[name], 13, True)
        assert _bits(xa, xm) and _bits(ya, ym)
        out = []
        for x, y, c in ((xa, ya, ca), (xm, ym, cm)):
            xr = x.detach().requires_grad_(True)
            loss, x255, y255 = PL().pixel_wise_255(xr, y, True)
            (0.37 * loss + (c * x255).sum()).backward()
            out.append((loss.detach(), x255.detach(), y255, xr.grad, PL().l1_mean(x, y)))
        assert all(_bits(a, b) for a, b in zip(*out)), name


def test_backward_agrees_with_autograd_of_the_restatement():
    """gradcheck-style: the ONE backward launch of pixel_wise_255 (gradients of loss and of x255 together) against torch autograd of
    the float64 restatement on the device -- clamp's mask, abs's sign and the chain through t come from torch here, not from the
    closed form."""
    for name in ('tail', 'fixture_image', 'blocks48'):
        x, y, c = _inputs(SHAPES[name], 14)
        xr = x.detach().requires_grad_(True)
        loss, x255, _ = PL().pixel_wise_255(xr, y, True)
        (0.37 * loss + (c * x255).sum()).backward()
        x64 = x.detach().double().requires_grad_(True)
        (0.37 * R.pixel_wise(x64, y) + (c.double() * R.t(x64)).sum()).backward()
        eg = R.rel(xr.grad, x64.grad)
        print('%s: dx against autograd of the restatement, rel %.3e (bar %.0e)' % (name, eg, R.GRAD_REL))
        assert eg <= R.GRAD_REL
        _check_planted(x, xr.grad, c, True)


def test_torch_range_1_to_255_is_a_differentiable_copy():
    x, _, c = _inputs(SHAPES['tail'], 15)
    before = x.clone()
    xr = x.requires_grad_(True)
    before_count = PL().COUNTERS['images_255']
    out = PL().torch_range_1_to_255(xr)
    assert PL().COUNTERS['images_255'] == before_count + 1
    assert out.data_ptr() != x.data_ptr() and _bits(x.detach(), before)           # the input is never modified
    et = float((out.detach().double() - R.t(x)).abs().max())
    (c * out).sum().backward()
    eg = R.rel(xr.grad, R.pixel_wise_grad(x.detach(), x.detach(), 0.0, c))
    print('torch_range_1_to_255: t %.3e (bar %.3e), dx rel %.3e (bar %.0e); range %.4f..%.4f' % (et, R.T_ABS, eg, R.GRAD_REL, float(out.min()),
                                                                                                 float(out.max())))
    assert et <= R.T_ABS and eg <= R.GRAD_REL and float(out.min()) == 0.0 and 254.99 < float(out.max()) < 255.0
    sliced = x.detach()[:, :, ::2]                                                # a non-contiguous argument is copied, not refused
    assert float((PL().torch_range_1_to_255(sliced).double() - R.t(sliced)).abs().max()) <= R.T_ABS


def test_input_rules():
    a = torch.zeros(2, 3, 8, 8, device='cuda')
    with pytest.raises(ValueError, match=r'\(2, 3, 8, 8\) and \(2, 3, 8, 9\)'):
        PL().pixel_wise_255(a, torch.zeros(2, 3, 8, 9, device='cuda'))
    with pytest.raises(ValueError, match=r'\(2, 3, 8, 8\) and \(384,\)'):
        PL().l1_mean(a, torch.zeros(384, device='cuda'))
    with pytest.raises(RuntimeError, match='second argument'):
        PL().pixel_wise_255(a, torch.zeros_like(a).requires_grad_(True))
    with pytest.raises(RuntimeError, match='second argument'):
        PL().l1_mean(a, torch.zeros_like(a).requires_grad_(True))
    with torch.no_grad():                                                         # ... which is no objection where nothing records
        assert float(PL().l1_mean(a, torch.zeros_like(a).requires_grad_(True))) == 0
    for bad in (a.double(), a.half()):
        with pytest.raises(RuntimeError, match='expected float32'):
            PL().l1_mean(bad, bad)
    with pytest.raises(ValueError, match='empty'):
        PL().l1_mean(a[:0], a[:0])


def test_indices_past_int32():
    """n = 2^31 + 4099 zeros with three planted values of x beyond and just below index 2^31: both modes' means and the positions
    and values of the only non-zero gradient entries.  (Every index in the kernels is 64-bit; a 32-bit one would wrap here.)"""
    n = 2 ** 31 + TILE + 3
    x, y = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    spots = torch.tensor([2 ** 31 - 1, 2 ** 31 + 5, n - 1], device='cuda')
    vals = torch.tensor([0.5, -3.0, 1.0], device='cuda')
    x[spots] = vals
    small_y = torch.zeros(3, device='cuda')
    # (the restatement's gradients divide by the three elements they are given: * 3 / n)
    for mode, want, want_g in (('plain', vals.double().abs().sum() / n, R.l1_mean_grad(vals, small_y, 0.61) * 3 / n),
                               ('range255', (R.t(small_y) - R.t(vals)).abs().sum() / n, R.pixel_wise_grad(vals, small_y, 0.61) * 3 / n)):
        xr = x.detach().requires_grad_(True)
        loss = PL().l1_mean(xr, y) if mode == 'plain' else PL().pixel_wise_255(xr, y, False)[0]
        (0.61 * loss).backward()
        ep = abs(float(loss.detach()) - float(want)) / float(want)
        got = xr.grad[spots]
        eg = R.rel(got, want_g)
        nonzero = int(torch.count_nonzero(xr.grad))
        print('n = 2^31 + %d, %s: loss rel %.3e (bar %.0e); gradient at the planted indices rel %.3e (bar %.0e), %d non-zero entries'
              % (n - 2 ** 31, mode, ep, R.MEAN_REL, eg, R.GRAD_REL, nonzero))
        assert ep <= R.MEAN_REL and eg <= R.GRAD_REL and nonzero == (3 if mode == 'plain' else 2)
        del xr, loss

"""Self-checks of the reference machinery of tests/test_gpu_dense_edges.py (tests/dense_refs.py), on the CPU: the sweep covers what
it claims, the integer inputs are discriminating, the a-priori bound holds for both accumulation orders of the linear kernels emulated
in float32, the host range-exponent rule reproduces hand-computed cases, the uint8 probe set is sharp, and the fp64 Adam restatement is
torch.optim.Adam."""
import numpy as np
import pytest
import torch

import dense_refs as R
from util import S  # noqa: F401  (puts the repository root on sys.path)


def test_linear_sweep_covers_every_value_pair_and_both_kernels():
    cases = R.linear_cases()
    assert len(cases) == len(set(cases)) and 40 <= len(cases) <= 52, len(cases)
    for axis, vals in enumerate((R.LIN_M, R.LIN_K, R.LIN_N)):
        assert {c[axis] for c in cases} == set(vals)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        vals = (R.LIN_M, R.LIN_K, R.LIN_N)
        assert {(c[a], c[b]) for c in cases} == {(x, y) for x in vals[a] for y in vals[b]}
    skinny = [c for c in cases if R.is_skinny(*c)]
    assert len(skinny) >= 12 and len(cases) - len(skinny) >= 12, (len(skinny), len(cases))
    # each threshold with the other two conditions true: both sides
    for lo, hi in (((128, 512, 64), (129, 512, 64)), ((128, 512, 64), (128, 513, 64)), ((128, 512, 64), (128, 512, 63))):
        assert lo in cases and hi in cases and R.is_skinny(*lo) and not R.is_skinny(*hi)


def test_integer_inputs_are_discriminating():
    for shape in ((129, 513), (67, 64), (5, 3), (128, 1), (1, 65)):
        a = R.int_tensor(3, 'disc%s' % (shape,), shape).numpy()
        assert a.min() >= -8 and a.max() <= 8 and (a == np.round(a)).all()
        assert a.any(1).all()                                           # no all-zero row
        if shape[1] >= 3:
            assert len(np.unique(a, axis=0)) == shape[0]                # no two equal rows
        else:
            assert (a[1:] != a[:-1]).any(1).all()                       # (17 values cannot fill 128 rows: neighbours differ)
        if shape[0] >= 3 and shape[1] > 1:
            assert len(np.unique(a, axis=1).T) == shape[1]              # no two equal columns
    assert torch.equal(R.int_tensor(3, 'same', (9, 9)), R.int_tensor(3, 'same', (9, 9)))


@pytest.mark.parametrize('M,K,N', R.linear_cases())
def test_both_accumulation_orders_meet_the_bound_and_are_exact_on_integers(M, K, N):
    worst = 0.0
    for emu in (R.emulate_skinny, R.emulate_tiled):
        x, w, b = R.linear_inputs('int', M, K, N)
        ref, _ = R.linear_ref(x, w, b, 0.5, 2.0)
        assert float(x.abs().max()) <= 8 and float((x.double().abs() @ w.double().abs().t()).max()) < 2 ** 24
        y = R.epilogue32(emu(x.numpy(), w.numpy()), b.numpy(), 0.5, 2.0)
        assert np.array_equal(y, ref.float().numpy())
        # one element dropped at a tail position: the integer check must notice
        for drop in ((M - 1, N - 1, K - 1), (0, N - 1, K - 1), (M - 1, 0, K - 1)):
            y = R.epilogue32(emu(x.numpy(), w.numpy(), drop=drop), b.numpy(), 0.5, 2.0)
            assert not np.array_equal(y, ref.float().numpy()), drop
        x, w, b = R.linear_inputs('real', M, K, N)
        ref, bound = R.linear_ref(x, w, b, 0.3, 2.0)
        y = R.epilogue32(emu(x.numpy(), w.numpy()), b.numpy(), 0.3, 2.0)
        worst = max(worst, R.ratio(torch.from_numpy(y), ref, bound))
    assert worst <= 1.0, worst


def test_bound_rejects_reduced_precision_and_a_wrong_scale():
    x, w, b = R.linear_inputs('real', 5, 512, 67)
    ref, bound = R.linear_ref(x, w, b, 0.3, 2.0)
    y16 = R.epilogue32(R.emulate_tiled(x.bfloat16().float().numpy(), w.numpy()), b.numpy(), 0.3, 2.0)
    assert R.ratio(torch.from_numpy(y16), ref, bound) > 10
    ys = R.epilogue32(R.emulate_tiled(x.numpy(), w.numpy()), b.numpy(), 0.3 * (1 + 2.0 ** -9), 2.0)
    assert R.ratio(torch.from_numpy(ys), ref, bound) > 1


def test_ulps_and_structured_style_layers():
    ref = torch.tensor([1.0, 0.25, 3.0], dtype=torch.float64)
    y = torch.tensor(np.array([1.0 + 2.0 ** -23, 0.25, 3.0 - 2.0 ** -21], np.float32))
    assert R.ulps(y, ref) == 2.0            # the spacing at 1.0 is 2^-23 (one step), at 3.0 it is 2^-22 (two steps)
    for D in (64, 256, 193, 512):
        mw, mb, q = R.structured_style_layer(5, 'ss%d' % D, D, 130, 16)
        style = R.int_tensor(5, 'ss.st%d' % D, (7, D), -2, 2)
        s, _ = R.style_ref(style, mw, mb, D)
        assert torch.equal(s, s.round()) and float(s.abs().max()) <= 4 and bool((s != 0).any(1).all())
        assert float(q.min()) >= 1 and float(q.max()) <= 4
        if R.pow4(D):
            assert len(torch.unique(s, dim=0)) > 1          # the rows differ between images
    assert R.wscale32(64) == 0.125 and R.wscale32(256) == 0.0625


def test_range_exponent_rule_hand_cases():
    """include/sgdfr.h: e = 18 - headroom - L - floor(log2 max|s|), |x| < 2^L; L = x_log2 or floor(log2 max|x|) + 1."""
    f = R.range_exponent
    assert f(1.0, 0, x_log2=10) == 8                    # 18 - 0 - 10 - 0
    assert f(1.5, 6, x_log2=10) == 2
    assert f(0.75, 0, x_log2=-3) == 22                  # floor(log2 0.75) = -1
    assert f(1024.0, 12, x_log2=4) == -8
    w = lambda v: int(np.float32(v).view(np.uint32))
    assert f(1.0, 0, word=w(37.0)) == 12                # floor(log2 37) + 1 = 6
    assert f(1.0, 0, word=w(32.0)) == 12 and f(1.0, 0, word=w(31.999)) == 13
    assert f(2.0 ** -100, 0, x_log2=-100) == 120        # 18 + 100 + 100 -> clamp
    assert f(2.0 ** 100, 12, x_log2=100) == -120        # 6 - 200 -> clamp
    assert f(0.0, 0, x_log2=10) == 0 and f(-0.0, 3, x_log2=1) == 0
    assert f(float('inf'), 0, x_log2=10) == 0 and f(float('nan'), 0, x_log2=10) == 0
    assert f(1.0, 0, word=0) == 0 and f(1.0, 0, word=0x7f800000) == 0 and f(1.0, 0, word=0x7fc00000) == 0
    sub = np.float32(2.0 ** -130)                       # subnormal styles count as 2^-126
    assert f(sub, 0, x_log2=30) == 18 - 30 + 126 and f(sub, 0, x_log2=10) == 120
    assert f(2.0 ** 30, 12, word=1) == 18 - 12 - (-126 + 1) - 30     # subnormal max |x| counts as 2^-126
    s = torch.tensor([[0.5, -3.0], [0.0, 0.0]])
    d = torch.tensor([[1.0], [7.0]])
    s_n, d_n, e = R.apply_range(s, d, 6, x_log2=10)
    assert e.tolist() == [1, 0] and torch.equal(s_n, torch.tensor([[1.0, -6.0], [0.0, 0.0]])) and torch.equal(d_n, torch.tensor([[0.5], [7.0]]))


def test_uint8_probe_set_is_sharp():
    p = R.u8_probe_set()
    assert p.dtype == np.float32 and len(p) == 1788
    a, b, c = R.u8_np32(p), R.u8_torch32(p), R.u8_f64(p)
    assert np.array_equal(a, b)
    assert set(a.tolist()) == set(range(255))
    assert 100 < int((a != c).sum()) < 400              # the fp64 evaluation rounds differently at many boundaries
    assert np.abs(a.astype(int) - c.astype(int)).max() == 1
    img = R.u8_image(2, 17, 35)
    assert img.size >= len(p) and set(img.ravel().tolist()) >= set(p[np.isfinite(p)].tolist())
    out, mask = R.u8_grid_host([img[:1], None, img], 2, True)
    assert out.shape == (2, 17, 105, 3) and not mask[:, :, 35:70].any() and mask[:, :, :35].all()
    assert np.array_equal(out[1, 3, 4], R.u8_np32(img[0, ::-1, 3, 4])) and np.array_equal(out[1, 3, 74], R.u8_np32(img[1, ::-1, 3, 4]))


def test_adam_restatement_is_torch_adam_in_fp64():
    torch.manual_seed(1)
    ps = [torch.randn(n, dtype=torch.float64) for n in (1, 7, 300)]
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam(ref, lr=3e-3, foreach=False)
    mine = R.Adam64(ps, lr=3e-3)
    for step in range(5):
        grads = [torch.randn_like(p) * 10.0 ** (step - 2) for p in ps]
        if step == 2:
            grads[1] = None                                 # a parameter without a gradient is skipped (its own step count waits)
        for r, g in zip(ref, grads):
            r.grad = None if g is None else g.clone()
        opt.step()
        mine.step(grads)
        for r, m in zip(ref, mine.p):
            assert torch.allclose(r.detach(), m, rtol=1e-13, atol=1e-15)
    # the shared-count variant (FusedAdam): the same while every parameter is live at every step, another bias correction after a skip
    a, b = R.Adam64(ps), R.Adam64(ps, shared_count=True)
    for step in range(4):
        grads = [torch.randn_like(p) for p in ps]
        if step == 2:
            assert all(torch.equal(x, y) for x, y in zip(a.p, b.p))
            grads[1] = None
        a.step(grads)
        b.step(grads)
    assert torch.equal(a.p[0], b.p[0]) and torch.equal(a.p[2], b.p[2]) and a.t[1] == 3 and b.t[1] == 4
    assert float(((a.p[1] - b.p[1]).abs() / (1e-7 + 2e-6 * b.p[1].abs())).max()) > 10        # far outside the bars of the GPU test


@pytest.mark.parametrize('D', [1, 63, 64, 65, 512, 515])
def test_pixel_norm_gradient_needs_the_eps_term_apart(D):
    """The bar of the pixel-norm gradient, (D/64 + 16) * 2^-23 of max |ref| per row, on the host: the form with the eps term apart
    (what pixelnorm_bwd_kernel evaluates) meets it at every D; the float32 difference r*g - x*r^3*mean(g*x) cannot at D = 1, where the
    whole gradient is the eps*r^2 remainder of two cancelling terms."""
    x = S.counter_tensor(31, 'pn.x%d.%d' % (5, D), (5, D))
    x[-1] = 0.0
    g = S.counter_tensor(31, 'pn.g%d.%d' % (5, D), (5, D))
    _, ref = R.pixelnorm_ref(x, g)

    def rel(form):
        got = torch.from_numpy(R.pixelnorm_bwd_emulated(x.numpy(), g.numpy(), form)).double()
        return float(((got - ref).abs() / ref.abs().amax(1, keepdim=True)).max())
    assert rel('eps-apart') <= 0.1 * R.pixelnorm_bar(D)
    assert (rel('difference') > 1e3 * R.pixelnorm_bar(D)) == (D == 1)
    assert torch.equal(ref[-1], g[-1].double() * R.PIXELNORM_EPS ** -0.5)          # the all-zero row: g * rsqrt(eps)

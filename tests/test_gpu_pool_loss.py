"""GPU: the pooled image loss (pool_loss.PoolMse, csrc/sweep.hip) against the stock expression in fp64 on the CPU
(tests/pool_loss_restatement.py), and PTI with finetune.PooledPtiLoss against the stock expression on the device.

Bars.  pooled: the bits of reenact.pool_images.  mse and dx: 8 x the deviation of the stock fp32 expression from the stock fp64
one on the same inputs, computed here on the CPU: the same sum in another order.  Parameter gradients of a PTI step: 5e-4 relative,
the project's gradient bar.  Every test prints the figures it asserts on.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from util import S, SEED, hip_generator
import pool_loss_restatement as PR

pytestmark = pytest.mark.gpu

BAR = 8.0
# (B, P, f, off): the smallest shapes that reach both walk paths and the partial-then-finish reduction with more than one block.
# off: x (and, in the backward, dx) is a view that many floats behind a 16-byte boundary
SHAPES = [(1, 6, 2, 0),        # 16-byte path, one block
          (2, 5, 2, 0),        # dword path: P * f = 10 is no multiple of 4
          (1, 8, 4, 0),
          (3, 16, 1, 0),       # f = 1: four pixels per lane, 3 blocks
          (1, 64, 4, 1),       # dword path at f = 4 through the alignment test, 16 blocks
          (1, 256, 2, 0)]      # many blocks: 128 on the 16-byte path
IDS = ['%dx%d_f%d%s' % (B, P, f, '_off' if off else '') for B, P, f, off in SHAPES]
_CASES = {}


def _offset_view(t, off):
    """The values of t in a contiguous view `off` floats behind a 16-byte boundary (torch's allocations start on one)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def case(B, P, f, off):
    """Inputs and the stock results of a shape, computed once on the CPU and shared by the tests: fp64, and fp32's deviation."""
    key = (B, P, f, off)
    if key not in _CASES:
        tag = 'pool.%d.%d.%d' % (B, P, f)
        x = S.counter_tensor(SEED, tag + '.x', (B, 3, P * f, P * f), 0.0, 0.5)
        real = S.counter_tensor(SEED, tag + '.r', (B, 3, P, P), 0.0, 0.5)
        gp = S.counter_tensor(SEED, tag + '.gp', (B, 3, P, P), 0.0, 1.0)
        gm = torch.tensor(0.75)
        c = {'x': x, 'real': real, 'gp': gp, 'gm': gm}
        p64, m64 = PR.forward(x.double(), real.double(), P)
        p32, m32 = PR.forward(x, real, P)
        c['pooled64'], c['mse64'], c['dev_mse'] = p64, float(m64), abs(float(m32) - float(m64))
        for name, a, b in (('both', gp, gm), ('pooled', gp, None), ('mse', None, gm)):
            d64 = PR.backward(x.double(), real.double(), P, None if a is None else a.double(), None if b is None else b.double())
            d32 = PR.backward(x, real, P, a, b)
            c['dx64_' + name], c['dev_dx_' + name] = d64, float((d32.double() - d64).abs().max())
        _CASES[key] = c
    return _CASES[key]


@pytest.mark.parametrize('B,P,f,off', SHAPES, ids=IDS)
def test_forward_pooled_bits_and_mse(B, P, f, off):
    from stylegan_directions_face_reenactment_amd.pool_loss import PoolMse
    from stylegan_directions_face_reenactment_amd.reenact import pool_images
    c = case(B, P, f, off)
    x = _offset_view(c['x'].cuda(), off)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 * off
    real = c['real'].cuda()
    pooled, mse = PoolMse.apply(x, real, P)
    pooled2, mse2 = PoolMse.apply(x, real, P)
    torch.cuda.synchronize()
    err_p = float((pooled.double().cpu() - c['pooled64']).abs().max())
    err = abs(float(mse) - c['mse64'])
    print('B %d P %d f %d off %d: mse %.9g  |HIP - fp64| %.3e = %.2f x the stock fp32 deviation %.3e   bar %.0f x;  pooled |HIP - fp64| %.3e'
          % (B, P, f, off, float(mse), err, err / max(c['dev_mse'], 1e-300), c['dev_mse'], BAR, err_p))
    assert tuple(pooled.shape) == (B, 3, P, P) and mse.dim() == 0 and not pooled.requires_grad
    assert torch.equal(pooled, pool_images(x, P))                         # the walk's bits, whatever the path
    assert err <= BAR * c['dev_mse']
    assert torch.equal(mse, mse2) and torch.equal(pooled, pooled2)        # no atomics: the same bits from call to call


@pytest.mark.parametrize('which', ['both', 'pooled', 'mse'])
@pytest.mark.parametrize('B,P,f,off', SHAPES, ids=IDS)
def test_backward_against_fp64_autograd(B, P, f, off, which):
    from stylegan_directions_face_reenactment_amd.pool_loss import PoolMse, pool_mse_backward
    c = case(B, P, f, off)
    x = _offset_view(c['x'].cuda(), off).requires_grad_(True)
    real, gp, gm = c['real'].cuda(), c['gp'].cuda(), c['gm'].cuda()
    pooled, mse = PoolMse.apply(x, real, P)
    total = 0
    if which != 'mse':
        total = total + (pooled * gp).sum()
    if which != 'pooled':
        total = total + mse * gm
    dx, = torch.autograd.grad(total, x)
    torch.cuda.synchronize()
    want, dev = c['dx64_' + which], c['dev_dx_' + which]
    err = float((dx.double().cpu() - want).abs().max())
    print('B %d P %d f %d off %d, gradients of %s: max |HIP - fp64| %.3e = %.2f x the stock fp32 deviation %.3e   bar %.0f x' % (
        B, P, f, off, which, err, err / max(dev, 1e-300), dev, BAR))
    assert tuple(dx.shape) == (B, 3, P * f, P * f)
    assert err <= BAR * dev
    # the dword path and the 16-byte path store the same values
    a = None if which == 'mse' else gp
    b = None if which == 'pooled' else gm.reshape(1)
    pd = pooled.detach()
    aligned = pool_mse_backward(a, pd, real, b, f)
    shifted = torch.empty(dx.numel() + 4, device='cuda')
    out = shifted[1:1 + dx.numel()].view(dx.shape)
    assert aligned.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    pool_mse_backward(a, pd, real, b, f, out=out)
    assert torch.equal(aligned, out) and torch.equal(aligned, dx)


def test_an_unused_output_and_a_real_with_grad():
    from stylegan_directions_face_reenactment_amd.pool_loss import PoolMse
    c = case(1, 8, 4, 0)
    x = c['x'].cuda().requires_grad_(True)
    real = c['real'].cuda()
    pooled, mse = PoolMse.apply(x, real, 8)
    assert pooled.requires_grad and mse.requires_grad
    with pytest.raises(ValueError, match='no gradient'):
        PoolMse.apply(x, real.clone().requires_grad_(True), 8)
    with torch.no_grad():
        p2, m2 = PoolMse.apply(x, real, 8)
    assert not p2.requires_grad and torch.equal(p2, pooled) and torch.equal(m2, mse)


# ---------------------------------------------------------------------------------------------------------------- PTI
def _lpips():
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    m = LPIPS()
    m.load_state_dict(S.synthetic_lpips_state(SEED))
    return m.cuda()


@pytest.fixture(scope='module')
def pti():
    G0 = hip_generator(256, 1)
    w = S.synthetic_latents(SEED, 1, n_latent=G0.n_latent, key='pti.w').cuda()
    trunc = S.counter_tensor(SEED, 'pti.t', (1, 512)).cuda()
    with torch.no_grad():
        base, _ = G0([w], input_is_latent=True, truncation=0.7, truncation_latent=trunc)
    return G0, _lpips(), w, trunc, base


def _target(base, P):
    pooled = F.adaptive_avg_pool2d(base, (P, P))
    return (pooled + 0.3 * S.counter_tensor(SEED, 'pti.pool.d%d' % P, tuple(pooled.shape)).cuda()).clamp(-1, 1).contiguous()


@pytest.mark.parametrize('P', [128, 64])
def test_first_step_gradients_against_the_stock_expression(pti, P):
    """The parameter gradients of one PTI step through PooledPtiLoss against adaptive_avg_pool2d + mse_loss + the same LPIPS
    module by autograd, on the device: 5e-4 relative, per tensor, to the tensor's largest gradient."""
    from stylegan_directions_face_reenactment_amd import finetune
    G0, m, w, trunc, base = pti
    target = _target(base, P)
    loss_fn = finetune.PooledPtiLoss(m, target, P)
    grads = {}
    for name in ('hip', 'stock'):
        G = copy.deepcopy(G0).train()
        params, lam = finetune.pti_parameters(G)
        img, _ = G([w], input_is_latent=True, truncation=0.7, truncation_latent=trunc)
        if name == 'hip':
            loss = loss_fn(img, target, lam)
        else:
            pooled = F.adaptive_avg_pool2d(img, (P, P))
            loss = F.mse_loss(pooled, target) * lam + m(pooled, m.target(target))
        grads[name] = (float(loss.detach()), torch.autograd.grad(loss, params))
    torch.cuda.synchronize()
    (l_hip, g_hip), (l_stock, g_stock) = grads['hip'], grads['stock']
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_hip, g_stock))
    print('P %d: loss %.6f against stock %.6f; %d parameter gradients, worst max |HIP - stock| / max |stock| = %.3e   bar 5e-4' % (
        P, l_hip, l_stock, len(g_hip), worst))
    assert lam == 100 and len(g_hip) == len(g_stock) > 0 and all(float(b.abs().max()) > 0 for b in g_stock)
    assert abs(l_hip - l_stock) <= 1e-5 * abs(l_stock)
    assert worst <= 5e-4


@pytest.mark.parametrize('P', [128, 64])
def test_pooled_pti_graph_replay_matches_eager_steps(pti, P):
    """finetune.optimize_g with PooledPtiLoss: 12 steps replayed as one captured hipGraph end at the weights of 12 eager steps (the
    tolerances of test_pti_with_the_real_loss_graph_replay_matches_eager_steps), and the loss goes down."""
    from stylegan_directions_face_reenactment_amd import finetune
    G0, m, w, trunc, base = pti
    target = _target(base, P)
    runs = {}
    for graph in (False, True):
        G = copy.deepcopy(G0)
        loss_fn = finetune.PooledPtiLoss(m, target, P)
        with torch.no_grad():
            first = loss_fn(G([w], input_is_latent=True, truncation=0.7, truncation_latent=trunc)[0], target, 100).item()
        G, loss = finetune.optimize_g(G, w, target, trunc, opt_steps=12, lr=1e-3, graph=graph, loss_fn=loss_fn)
        print('P %d graph %s: loss %.6f after 12 steps, %.6f before' % (P, graph, loss.item(), first))
        assert loss.item() < first
        runs[graph] = (G, loss.item())
    assert abs(runs[False][1] - runs[True][1]) <= 2e-3 * abs(runs[False][1])
    for (k, a), (_, b) in zip(runs[False][0].state_dict().items(), runs[True][0].state_dict().items()):
        assert torch.allclose(a, b, rtol=2e-3, atol=2e-4), k
    loss_fn = finetune.PooledPtiLoss(m, target, P)
    with pytest.raises(RuntimeError, match='different real image'):
        loss_fn(base, target.clone(), 100)

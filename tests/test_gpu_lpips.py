"""GPU: the HIP LPIPS (lpips.LPIPS, csrc/lpips.hip) against the fp64 restatement -- taps, loss, dL/dx, the conv0 padding rule,
determinism under graph replay -- and PTI with its real loss (finetune.PtiLoss)."""
import copy

import pytest
import torch

from util import S, SEED, hip_generator
import lpips_restatement as R

pytestmark = pytest.mark.gpu


def _module(seed=SEED):
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    sd = S.synthetic_lpips_state(seed)
    m = LPIPS()
    m.load_state_dict(sd)
    return m.cuda(), sd


def _images(key, shape):
    return S.counter_tensor(SEED, key, shape, 0.0, 0.5).clamp(-1, 1)


def _hip_taps(m, x):
    """The five taps of the HIP forward (for comparisons and to fix the fp64 reference's masks)."""
    from stylegan_directions_face_reenactment_amd import lpips as L
    B, _, H, W = x.shape
    feats = L._features(m.packed(), x.cuda().contiguous(), None, H, W).cpu()
    out, o = [], 0
    for t in R.taps(m.state_dict(), torch.zeros(B, 3, H, W, dtype=torch.float64)):
        n = t.numel()
        out.append(feats[o:o + n].view(t.shape))
        o += n
    assert o == feats.numel()
    return out


def _rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize('B,H,W', [(1, 256, 256), (3, 256, 256), (2, 80, 72)])
def test_lpips_forward_matches_fp64(B, H, W):
    m, sd = _module()
    x, y = _images('lp.x%d' % H, (B, 3, H, W)), _images('lp.y%d' % H, (B, 3, H, W))
    for a, b in zip(_hip_taps(m, x), R.taps(sd, x)):
        assert a.shape == b.shape
        assert _rel(a, b) <= 1e-5
    ref = float(R.lpips(sd, x, y))
    live = float(m(x.cuda(), y.cuda()))
    cached = float(m(x.cuda(), m.target(y.cuda())))
    assert abs(live - ref) <= 1e-5 * abs(ref), (live, ref)
    assert abs(cached - ref) <= 1e-5 * abs(ref), (cached, ref)


def test_lpips_broadcast_target():
    m, sd = _module()
    x, y = _images('lp.bx', (3, 3, 64, 64)), _images('lp.by', (1, 3, 64, 64))
    ref = float(R.lpips(sd, x, y))
    got = float(m(x.cuda(), m.target(y.cuda())))
    assert abs(got - ref) <= 1e-5 * abs(ref)


@pytest.mark.parametrize('B,H,W,cached', [(1, 256, 256, True), (2, 64, 64, False), (2, 80, 72, True)])
def test_lpips_input_gradient_matches_fp64(B, H, W, cached):
    m, sd = _module()
    x, y = _images('lp.gx%d' % H, (B, 3, H, W)), _images('lp.gy%d' % H, (B, 3, H, W))
    xh = x.cuda().requires_grad_(True)
    loss = m(xh, m.target(y.cuda()) if cached else y.cuda())
    (loss * 3.0).backward()
    xr = x.double().requires_grad_(True)
    (R.lpips(sd, xr, y, fixed=_hip_taps(m, x)) * 3.0).backward()
    err = _rel(xh.grad, xr.grad)
    assert err <= 1e-4, err


def test_lpips_conv0_padding_is_zero_after_the_z_score():
    """A bright frame around a dark image: conv0's windows that reach into the padding see 0 (not (0 - mean) / std)."""
    m, sd = _module()
    x = torch.full((1, 3, 64, 64), -0.9)
    x[:, :, :3, :] = x[:, :, -3:, :] = x[:, :, :, :3] = x[:, :, :, -3:] = 0.95
    y = torch.zeros(1, 3, 64, 64)
    ref = float(R.lpips(sd, x, y))
    # the other rule: pad the raw image with zeros and z-score afterwards
    mean, std = sd['net.mean'].double(), sd['net.std'].double()
    xp = torch.nn.functional.pad(x.double(), (2, 2, 2, 2))
    z = (xp - mean) / std
    w0 = sd['net.layers.0.weight'].double()
    wrong_tap1 = torch.relu(torch.nn.functional.conv2d(z, w0, sd['net.layers.0.bias'].double(), 4, 0))
    right_tap1 = R.taps(sd, x)[0]
    assert float((wrong_tap1 - right_tap1).abs().max()) > 1e-2      # the fixture separates the two rules
    hip_tap1 = _hip_taps(m, x)[0]
    assert _rel(hip_tap1, right_tap1) <= 1e-5
    got = float(m(x.cuda(), y.cuda()))
    assert abs(got - ref) <= 1e-5 * abs(ref)
    xh = x.cuda().requires_grad_(True)
    m(xh, y.cuda()).backward()
    xr = x.double().requires_grad_(True)
    R.lpips(sd, xr, y, fixed=_hip_taps(m, x)).backward()
    assert _rel(xh.grad, xr.grad) <= 1e-4


def test_lpips_is_deterministic_and_replays_bit_identically():
    from stylegan_directions_face_reenactment_amd import functional as F_
    m, _ = _module()
    x = _images('lp.dx', (1, 3, 256, 256)).cuda()
    tgt = m.target(_images('lp.dy', (1, 3, 256, 256)).cuda())
    xs = x.clone().requires_grad_(True)

    def step():
        xs.grad = None
        loss = m(xs, tgt)
        loss.backward()
        return loss.detach(), xs.grad

    l1, g1 = [v.clone() for v in step()]
    l2, g2 = [v.clone() for v in step()]
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with F_.capture_graph(graph):
        lg = m(xs, tgt)
        lg.backward()
    gg = xs.grad
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lg.detach(), l1) and torch.equal(gg, g1)


def test_lpips_rejects_trainable_weights_and_stale_targets():
    m, _ = _module()
    x = _images('lp.rx', (1, 3, 64, 64)).cuda()
    tgt = m.target(x)
    m.lin[0][1].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='requires_grad'):
        m(x, tgt)
    m.lin[0][1].weight.requires_grad_(False)
    with torch.no_grad():
        m.lin[0][1].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match='target'):
        m(x, tgt)
    with pytest.raises(RuntimeError, match='y'):
        m(x, x.clone().requires_grad_(True))


def test_pti_with_the_real_loss_graph_replay_matches_eager_steps():
    """finetune.optimize_g with PtiLoss (100 * MSE + LPIPS): 12 steps replayed as one captured hipGraph end at the weights of 12
    eager steps (the tolerance of test_pti_driver_graph_replay_matches_eager_steps), and the loss goes down."""
    from stylegan_directions_face_reenactment_amd import finetune
    G0 = hip_generator(256, 1)
    m, _ = _module()
    w = S.synthetic_latents(SEED, 1, n_latent=G0.n_latent, key='pti.w').cuda()
    trunc = S.counter_tensor(SEED, 'pti.t', (1, 512)).cuda()
    with torch.no_grad():
        base, _ = G0([w], input_is_latent=True, truncation=0.7, truncation_latent=trunc)
    target = (base + 0.3 * S.counter_tensor(SEED, 'pti.d', tuple(base.shape)).cuda()).clamp(-1, 1)
    runs = {}
    for graph in (False, True):
        G = copy.deepcopy(G0)
        loss_fn = finetune.PtiLoss(m, target)
        with torch.no_grad():
            first = loss_fn(G([w], input_is_latent=True, truncation=0.7, truncation_latent=trunc)[0], target, 100).item()
        G, loss = finetune.optimize_g(G, w, target, trunc, opt_steps=12, lr=1e-3, graph=graph, loss_fn=loss_fn)
        assert loss.item() < first
        runs[graph] = (G, loss.item())
    assert abs(runs[False][1] - runs[True][1]) <= 2e-3 * abs(runs[False][1])
    for (k, a), (_, b) in zip(runs[False][0].state_dict().items(), runs[True][0].state_dict().items()):
        assert torch.allclose(a, b, rtol=2e-3, atol=2e-4), k
    loss_fn = finetune.PtiLoss(m, target)
    with pytest.raises(RuntimeError, match='different real image'):
        loss_fn(base, target.clone(), 100)
    target.add_(0.0)
    with pytest.raises(RuntimeError, match='modified in place'):
        loss_fn(base, target, 100)


def test_compat_install_lpips_serves_the_reference_constructor():
    import sys
    from stylegan_directions_face_reenactment_amd import compat
    sd = S.synthetic_lpips_state(SEED)
    saved = {k: v for k, v in sys.modules.items() if k == 'libs' or k.startswith('libs.')}
    try:
        compat.install_lpips(sd)
        from libs.criteria.lpips.lpips import LPIPS
        m = LPIPS(net_type='alex')
        x, y = _images('lp.cx', (1, 3, 64, 64)), _images('lp.cy', (1, 3, 64, 64))
        ref = float(R.lpips(sd, x, y))
        assert abs(float(m(x.cuda(), y.cuda())) - ref) <= 1e-5 * abs(ref)
    finally:
        for k in [k for k in sys.modules if k == 'libs' or k.startswith('libs.')]:
            del sys.modules[k]
        sys.modules.update(saved)

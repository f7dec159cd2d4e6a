"""GPU: the HIP identity loss (id_loss.IDLoss, csrc/idloss.hip) against the reference's own code (kat10), the fp64 restatement
(per-stage activations, dL/dx) and the stock MIOpen module with the same weights; determinism under graph replay; the trainer's
direction step; the opt-in compat mount."""
import os
import sys

import numpy as np
import pytest
import torch

from util import S, SEED, golden, hip_generator, t
import idloss_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STATE = {}


def _state(seed):
    if seed not in _STATE:
        _STATE[seed] = S.synthetic_arcface_state(seed)
    return _STATE[seed]


def _module(seed=SEED):
    from stylegan_directions_face_reenactment_amd.id_loss import IDLoss
    sd = _state(seed)
    m = IDLoss()
    m.load_state_dict(sd)
    return m.cuda().eval(), sd


def _images(key, shape):
    return S.counter_tensor(SEED, key, shape, 0.0, 0.5).clamp(-1, 1)


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max() / b.detach().double().abs().max())


def _outside_window_nonzero(g):
    out = g.detach().cpu().clone()
    out[:, :, 35:223, 32:220] = 0
    return int(torch.count_nonzero(out))


def _hip_masks(m, x, crop):
    """The HIP forward's saved activations and its PReLU / SE-ReLU decisions (masks for the fp64 restatement)."""
    from stylegan_directions_face_reenactment_amd import id_loss as L
    _, saved = L._forward(m.facenet.packed(), x.cuda().contiguous(), None, crop, True)
    V = L.saved_views(saved.cpu(), x.shape[0])
    return V, {'p0': V['p0'] > 0, 'p1': [p > 0 for p in V['p1']], 'h': [gt[:, gt.shape[1] * 16 // 17:] > 0 for gt in V['gate']]}


def _own_masks(masks, sd, x, crop):
    """(HIP decision, fp64 decision) pairs of every PReLU / SE-ReLU input."""
    ref = R.backbone(sd, x.cpu(), crop)
    pairs = [(masks['p0'], ref['p0'] > 0)]
    pairs += [(a, b > 0) for a, b in zip(masks['p1'], ref['p1'])]
    pairs += [(a, b > 0) for a, b in zip(masks['h'], ref['h'])]
    return pairs


def _stock(sd):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import loss_heads as LH
    m = LH.IdLoss()
    m.facenet.load_state_dict(sd)
    m = m.cuda().eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_kat10_on_the_hip_path():
    g = golden('kat10_idloss.npz')
    seed = int(g['seed'])
    m, _ = _module(seed)
    for name, shape, crop in (('crop', (1, 3, 256, 256), True), ('nocrop', (2, 3, 120, 112), False)):
        x = S.counter_tensor(seed, str(g['x_key_' + name]), shape, 0.0, 0.5).clamp(-1, 1).cuda()
        y = S.counter_tensor(seed, str(g['y_key_' + name]), shape, 0.0, 0.5).clamp(-1, 1).cuda()
        with torch.no_grad():
            ex, ey = m.extract_feats(x, crop), m.extract_feats(y, crop)
        for e, ref in ((ex, t(g['ex_' + name])), (ey, t(g['ey_' + name]))):
            assert float((e.cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), name
        xg = x.clone().requires_grad_(True)
        loss = m(xg, y, crop=crop)
        loss.backward()
        ref = float(g['loss_' + name])
        assert ref >= 0.05 and abs(loss.item() - ref) <= 1e-5, (name, loss.item(), ref)
        dref = t(g['dx_' + name])
        dx = xg.grad.cpu()
        if crop:
            assert _outside_window_nonzero(dx) == 0                          # exactly 0 outside the window
        # dL/dx is discontinuous where a PReLU / SE-ReLU input crosses 0: the few decisions that fp32 and fp64 take differently
        # move it by ~1e-2 max near those pixels.  With the HIP forward's decisions, the fp64 restatement (pinned to this fixture
        # on the CPU) agrees to 1e-4 max; against the fixture itself the bar is the size of such a flip.
        _, masks = _hip_masks(m, x, crop)
        pairs = _own_masks(masks, _state(seed), x, crop)
        flips, total = sum(int((a != b).sum()) for a, b in pairs), sum(a.numel() for a, _ in pairs)
        assert flips <= 1e-4 * total, (flips, total)
        xr = x.cpu().double().requires_grad_(True)
        R.id_loss(_state(seed), xr, y.cpu(), crop, masks).backward()
        assert _rel(dx, xr.grad) <= 1e-4, name
        inner = dx[:, :, 35:223, 32:220] if crop else dx
        assert float((inner - dref).abs().max()) <= 3e-2 * float(dref.abs().max()), name


@pytest.mark.parametrize('B,H,W,crop', [(1, 256, 256, True), (3, 256, 256, True), (2, 120, 112, False), (1, 200, 180, True)])
def test_stages_and_input_gradient_match_fp64(B, H, W, crop):
    from stylegan_directions_face_reenactment_amd import id_loss as L
    m, sd = _module()
    x = _images('idl.x%d_%d' % (B, H), (B, 3, H, W))
    emb, saved = L._forward(m.facenet.packed(), x.cuda().contiguous(), None, crop, True)
    V = L.saved_views(saved.cpu(), B)
    ref = R.backbone(sd, x, crop)
    assert _rel(V['p0'], ref['p0']) <= 1e-4
    first = [i for i, u in enumerate(R.UNITS) if u[2] == 2]
    for i in first + [i - 1 for i in first[1:]] + [len(R.UNITS) - 1]:   # each stage's first (stride-2) unit and each stage's last
        assert _rel(V['p1'][i], ref['p1'][i]) <= 1e-4, i
        assert _rel(V['c2'][i], ref['c2'][i]) <= 1e-4, i
        d = ref['c2'][i].shape[1]
        assert _rel(V['gate'][i][:, :d], ref['g'][i]) <= 1e-4, i
    assert _rel(emb, ref['e']) <= 1e-4
    # dL/dx for a fixed dL/de, the fp64 reference taking the HIP forward's PReLU / SE-ReLU decisions
    ge = S.counter_tensor(SEED, 'idl.ge%d_%d' % (B, H), (B, 512))
    xg = x.cuda().requires_grad_(True)
    (m.extract_feats(xg, crop) * ge.cuda()).sum().backward()
    _, masks = _hip_masks(m, x, crop)
    xr = x.double().requires_grad_(True)
    (R.backbone(sd, xr, crop, masks)['e'] * ge.double()).sum().backward()
    assert _rel(xg.grad, xr.grad) <= 1e-4
    if crop:
        assert _outside_window_nonzero(xg.grad) == 0


def _live_cached_broadcast_agree(B):
    m, _ = _module()
    x = _images('idl.bx', (B, 3, 256, 256)).cuda()
    y1 = _images('idl.by', (1, 3, 256, 256)).cuda()
    runs = []
    for y in (y1, m.target(y1), y1.expand(B, -1, -1, -1).contiguous()):
        xg = x.clone().requires_grad_(True)
        loss = m(xg, y)
        loss.backward()
        runs.append((loss.detach(), xg.grad))
    for loss, g in runs[1:]:
        assert abs(float(loss) - float(runs[0][0])) <= 1e-5 * abs(float(runs[0][0]))   # target(y) alone: its own split-K plan
        assert _rel(g, runs[0][1]) <= 1e-5


def test_live_y_cached_target_and_broadcast_agree():
    _live_cached_broadcast_agree(3)


def test_live_y_cached_target_and_broadcast_agree_at_b16():
    """At 16 rows most convs keep K in one slice: the rule that x's rows decide the plan holds there as where everything is sliced."""
    _live_cached_broadcast_agree(16)


def test_eager_calls_and_graph_replay_are_bit_identical():
    from stylegan_directions_face_reenactment_amd import functional as F_
    m, _ = _module()
    x = _images('idl.gx', (2, 3, 256, 256)).cuda()
    y = _images('idl.gy', (2, 3, 256, 256)).cuda()
    xs = x.clone().requires_grad_(True)

    def step():
        xs.grad = None
        loss = m(xs, y)
        loss.backward()
        return loss.detach().clone(), xs.grad.clone()

    l1, g1 = step()
    l2, g2 = step()
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with F_.capture_graph(graph):
        lg = m(xs, y)
        lg.backward()
    gg = xs.grad
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lg.detach(), l1) and torch.equal(gg, g1)


def test_b16_matches_the_stock_module():
    m, sd = _module()
    stock = _stock(sd)
    x = _images('idl.sx', (16, 3, 256, 256)).cuda()
    y = _images('idl.sy', (16, 3, 256, 256)).cuda()
    out = []
    for mod in (m, stock):
        xg = x.clone().requires_grad_(True)
        loss = mod(xg, y)
        loss.backward()
        out.append((float(loss), xg.grad))
    (lh, gh), (ls, gs) = out
    assert abs(lh - ls) <= 1e-4 * abs(ls), (lh, ls)
    # two fp32 implementations take a few PReLU decisions near 0 differently (see test_kat10_on_the_hip_path): measured 3.1e-3
    assert _rel(gh, gs) <= 1e-2


def test_trainer_direction_step_matches_the_stock_head():
    """10 * IDLoss(G(z, shift = A(sv)), source) back to the direction matrix A (trainer.py:177-189, utils_train.py:423): dL/dA
    with the HIP IDLoss against the stock head with the same weights."""
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    m, sd = _module()
    stock = _stock(sd)
    G = hip_generator(256, 1)
    for p in G.parameters():
        p.requires_grad_(False)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(SEED, num_layers=8))
    A = A.cuda()
    B = 4
    zs = S.synthetic_z(SEED, B, key='idl.zs').cuda()
    sv = S.counter_tensor(SEED, 'idl.sv', (B, 15), 0.0, 3.0).cuda()
    trunc = S.counter_tensor(SEED, 'idl.trunc', (1, 512)).cuda()
    with torch.no_grad():
        src = generate_image(G, zs, 0.7, trunc, input_is_latent=False, return_latents=False)
    grads = []
    for head in (m, stock):
        A.zero_grad()
        img, _ = generate_image(G, zs, 0.7, trunc, shift_code=A(sv), input_is_latent=False, return_latents=True)
        (10.0 * head(img, src)).backward()
        grads.append(torch.cat([p.grad.flatten() for p in A.parameters()]))
    assert _rel(grads[0], grads[1]) <= 1e-3


def test_stale_targets_trainable_weights_and_train_mode_raise():
    m, _ = _module()
    y = _images('idl.ry', (1, 3, 256, 256)).cuda()
    x = _images('idl.rx', (1, 3, 256, 256)).cuda()
    tgt = m.target(y)
    y.add_(0.1)
    with pytest.raises(RuntimeError, match='modified'):
        m(x, tgt)
    tgt = m.target(y)
    with torch.no_grad():
        m.facenet.body[3].res_layer[1].weight.mul_(1.01)
    with pytest.raises(RuntimeError, match='other weights'):
        m(x, tgt)
    m.facenet.output_layer[3].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='requires_grad'):
        m(x, y)
    m.facenet.output_layer[3].weight.requires_grad_(False)
    m.facenet.train()
    with pytest.raises(RuntimeError, match='eval'):
        m(x, y)


def test_compat_mount_serves_the_unchanged_constructor(tmp_path):
    from stylegan_directions_face_reenactment_amd import compat
    sd = _state(SEED)
    path = str(tmp_path / 'model_ir_se50.pth')
    torch.save(sd, path)
    saved = {k: sys.modules.get(k) for k in ('libs', 'libs.criteria', compat.ID_LOSS_ALIAS)}
    try:
        compat.install_id_loss(path)
        from libs.criteria import id_loss
        idl = id_loss.IDLoss().cuda().eval()                     # utils_train.py:53
        m, _ = _module()
        x = _images('idl.cx', (2, 3, 256, 256)).cuda()
        y = _images('idl.cy', (2, 3, 256, 256)).cuda()
        assert torch.equal(idl(x, y), m(x, y))
        assert np.isfinite(float(idl(x, y)))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v

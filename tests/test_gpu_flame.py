"""GPU: the HIP FLAME decode and ShapeLoss (flame.py, csrc/flame.hip) against the reference's own code (kat11), the fp64 restatement
(outputs, dynamic contour rows, coefficient gradients for smooth cotangents) and the torch composition of the reference's losses on
the decode's outputs; determinism under graph replay; what is saved; the trainer's direction step.

Bars.  kat11 (set by the fixture): outputs within 4 x the reference's own fp32-vs-fp64 deviation, terms and gradients within
max(4 x dev, 2e-6) relative.  Smooth cotangents: SMOOTH_BAR = 2e-5 of the largest gradient element -- each gradient element is a
random-sign sum of 15 069 products per row, so its fp32 rounding error is about eps * sqrt(15 069) = 6e-8 * 123 = 7e-6 of the typical
product sum, taken with a factor of three for the chain behind it (skinning, kinematic chain, Rodrigues).
Measured on an MI355X: kat11 outputs 0.8 ... 1.1 x the reference's own fp32 deviation, gradients 1.3e-7 ... 4.5e-7; smooth cotangents at most 4.8e-7.
"""
import numpy as np
import pytest
import torch

from util import S, SEED, golden, hip_generator, t
import flame_restatement as R
from test_cpu_flame import flame_state, kat_inputs

pytestmark = pytest.mark.gpu

SMOOTH_BAR = 2e-5
_MODULES = {}


def _module(seed):
    from stylegan_directions_face_reenactment_amd.flame import FLAME
    if seed not in _MODULES:
        m = FLAME()
        m.load_state_dict(flame_state(seed))
        _MODULES[seed] = m.cuda()
    return _MODULES[seed]


def _cuda(c, grad=()):
    return {k: v.clone().cuda().requires_grad_(k in grad) for k, v in c.items()}


def _maxabs(a, b):
    return float((a.detach().double().cpu() - torch.as_tensor(b).double()).abs().max())


def _rel(a, b):
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a.detach().double().cpu() - b).abs().max() / b.abs().max())


def _bar(dev):
    return max(4.0 * float(dev), 2e-6)


def test_kat11_on_the_hip_path():
    from stylegan_directions_face_reenactment_amd import flame as FL
    g = golden('kat11_flame.npz')
    m = _module(int(g['seed']))
    gt, reen = kat_inputs(g)
    stride = int(g['stride'])
    cr = _cuda(reen, ('shape', 'exp', 'pose'))
    verts, _, _ = m(cr['shape'], cr['exp'], cr['pose'])
    fixed = R.fixed_cam(cr)
    l2, l3, tv = FL.decode(m, fixed)
    figures = {'vertices': (_maxabs(verts[:, ::stride], g['vertices']), 4 * float(g['dev_vertices'])),
               'trans_verts': (_maxabs(tv[:, ::stride], g['trans_verts']), 4 * float(g['dev_trans_verts'])),
               'landmarks2d': (_maxabs(l2, g['landmarks2d']), 4 * float(g['dev_landmarks2d'])),
               'landmarks3d': (_maxabs(l3, g['landmarks3d']), 4 * float(g['dev_landmarks3d']))}
    assert torch.equal(FL.dynamic_rows(m, cr['pose']).cpu().long(), t(g['dyn_reen']))
    assert torch.equal(FL.dynamic_rows(m, gt['pose'].cuda()).cpu().long(), t(g['dyn_gt']))
    loss, terms = FL.ShapeLoss(m)(_cuda(gt), cr, 1.0, 1.0, 1.0)
    loss.backward()
    for k in ('loss_shape', 'loss_mouth', 'loss_eye'):
        figures[k] = (_rel(terms[k], g[k]), _bar(g['dev_' + k]))
    figures['total'] = (_rel(loss, g['total']), _bar(g['dev_total']))
    for k in ('shape', 'exp', 'pose'):
        figures['grad_' + k] = (_rel(cr[k].grad, g['grad_' + k]), _bar(g['dev_grad_' + k]))
    for k, (v, bar) in figures.items():
        print('kat11 %-12s hip deviation %.3e   bar %.3e   reference fp32 deviation %.3e' % (k, v, bar, float(g['dev_' + k])))
    for k, (v, bar) in figures.items():
        assert v <= bar, (k, v, bar)


def _smooth_case(rows, key):
    yaw = [0.3 * ((i % 7) - 3) for i in range(rows)]
    if rows > 1:
        yaw[1] = 0.95                                        # beyond the 39 degree clamp
    c = S.synthetic_flame_coeffs(SEED, key, rows, yaw)
    if rows > 2:
        c['pose'][2] = 0.0                                   # a zero rotation vector: Rodrigues at its 1e-8 offset
    w = {'l2': S.counter_tensor(SEED, key + '.w2', (rows, 68, 3)), 'l3': S.counter_tensor(SEED, key + '.w3', (rows, 68, 3)),
         'tv': S.counter_tensor(SEED, key + '.wv', (rows, 5023, 3), 0.0, 0.02)}
    return c, w


@pytest.mark.parametrize('rows', [1, 3, 16, 32, 17, 24, 33, 40])      # partial first chunk, whole chunks, partial chunks after full ones
def test_decode_backward_matches_fp64_for_smooth_cotangents(rows):
    from stylegan_directions_face_reenactment_amd import flame as FL
    m = _module(SEED)
    T = R.tables(flame_state(SEED))
    c, w = _smooth_case(rows, 'flame.smooth%d' % rows)
    names = ('shape', 'exp', 'pose', 'cam')
    ch = _cuda(c, names)
    l2, l3, tv = FL.decode(m, ch)
    ((l2 * w['l2'][:, :, :2].cuda()).sum() + (l3 * w['l3'].cuda()).sum() + (tv * w['tv'].cuda()).sum()).backward()
    dyn = FL.dynamic_rows(m, ch['pose']).cpu().long()
    cd = {k: v.double().requires_grad_(True) for k, v in c.items()}
    r2, r3, rv, out = R.decode(T, cd, dyn=dyn)
    assert torch.equal(out['dyn'], R.dynamic_row(R.rodrigues(c['pose'][:, :3].double()))[0])        # the HIP rows are the fp64 rows
    if rows > 1:
        assert float(out['deg'][1].detach()) > 39.5
    ((r2 * w['l2'][:, :, :2].double()).sum() + (r3 * w['l3'].double()).sum() + (rv * w['tv'].double()).sum()).backward()
    for a, b, what in ((l2, r2, 'landmarks2d'), (l3, r3, 'landmarks3d'), (tv, rv, 'trans_verts')):
        assert _rel(a, b) <= 2e-6, what
    for k in names:
        rel = _rel(ch[k].grad, cd[k].grad)
        print('smooth rows=%d d%s rel %.3e' % (rows, k, rel))
        assert rel <= SMOOTH_BAR, (k, rel)
    # the un-projected triple (FLAME.forward) through the same kernels
    ch = _cuda(c, names[:3])
    v, f2, f3 = m(ch['shape'], ch['exp'], ch['pose'])
    ((f2 * w['l2'].cuda()).sum() + (f3 * w['l3'].cuda()).sum() + (v * w['tv'].cuda()).sum()).backward()
    cd = {k: c[k].double().requires_grad_(True) for k in names[:3]}
    out = R.flame_forward(T, cd['shape'], cd['exp'], cd['pose'], dyn=dyn)
    ((out['landmarks2d'] * w['l2'].double()).sum() + (out['landmarks3d'] * w['l3'].double()).sum() + (out['vertices'] * w['tv'].double()).sum()).backward()
    assert _rel(v, out['vertices']) <= 2e-6
    for k in names[:3]:
        rel = _rel(ch[k].grad, cd[k].grad)
        print('smooth rows=%d un-projected d%s rel %.3e' % (rows, k, rel))
        assert rel <= SMOOTH_BAR, (k, rel)


def _composition(m, gt, reen):
    """Losses o decode o cam = (8, 0, 0) with torch autograd on flame.decode's outputs (the formulas of losses.py:20-62)."""
    from stylegan_directions_face_reenactment_amd import flame as FL
    l2g, _, tvg = FL.decode(m, R.fixed_cam(gt))
    l2r, _, tvr = FL.decode(m, R.fixed_cam(reen))
    return R.losses(l2g, tvg, l2r, tvr)


def test_shape_loss_equals_the_composition_of_the_reference_losses():
    from stylegan_directions_face_reenactment_amd import flame as FL
    g = golden('kat11_flame.npz')
    m = _module(int(g['seed']))
    T = R.tables(flame_state(int(g['seed'])))
    gt, reen = kat_inputs(g)
    lam = (0.7, 1.3, 2.0)
    # fp64 restatement: the yardstick of the composition's own deviation
    cd = {k: v.double().requires_grad_(k != 'cam') for k, v in reen.items()}
    l2g, _, tvg, _ = R.decode(T, R.fixed_cam({k: v.double() for k, v in gt.items()}))
    l2r, _, tvr, _ = R.decode(T, R.fixed_cam(cd))
    terms64 = R.losses(l2g, tvg, l2r, tvr)
    (lam[1] * terms64[1] + lam[0] * terms64[0] + lam[2] * terms64[2]).backward()
    # torch composition on the HIP decode
    cg, cc = _cuda(gt, ('shape', 'exp', 'pose')), _cuda(reen, ('shape', 'exp', 'pose'))
    termsc = _composition(m, cg, cc)
    (lam[1] * termsc[1] + lam[0] * termsc[0] + lam[2] * termsc[2]).backward()
    # the fused path
    ch, chg = _cuda(reen, ('shape', 'exp', 'pose')), _cuda(gt, ('shape', 'exp', 'pose'))
    cam_before = ch['cam'].clone()
    loss, terms = FL.ShapeLoss(m)(chg, ch, *lam)
    loss.backward()
    assert torch.equal(ch['cam'], cam_before) and torch.equal(chg['cam'], gt['cam'].cuda())
    assert all(chg[k].grad is None for k in ('shape', 'exp', 'pose'))
    assert all(v.dim() == 0 and v.is_cuda for v in list(terms.values()) + [loss])
    for i, k in enumerate(('loss_shape', 'loss_mouth', 'loss_eye')):
        dev = _rel(termsc[i], terms64[i])
        rel = _rel(terms[k], lam[i] * termsc[i])
        print('ShapeLoss %-10s vs composition %.3e   composition vs fp64 %.3e' % (k, rel, dev))
        assert rel <= _bar(dev), (k, rel, dev)
    for k in ('shape', 'exp', 'pose'):
        dev = _rel(cc[k].grad, cd[k].grad)
        rel = _rel(ch[k].grad, cc[k].grad)
        print('ShapeLoss d%-9s vs composition %.3e   composition vs fp64 %.3e' % (k, rel, dev))
        assert rel <= _bar(dev), (k, rel, dev)


def test_eager_calls_side_stream_and_graph_replays_are_bit_identical():
    from stylegan_directions_face_reenactment_amd import flame as FL, functional as F_
    m = _module(SEED)
    sl = FL.ShapeLoss(m)
    gt = _cuda(S.synthetic_flame_coeffs(SEED, 'flame.det.gt', 16, [0.1 * (i - 8) for i in range(16)]))
    reen = _cuda(S.synthetic_flame_coeffs(SEED, 'flame.det.re', 16, [0.12 * (7 - i) for i in range(16)]), ('shape', 'exp', 'pose'))

    def step():
        for k in ('shape', 'exp', 'pose'):
            reen[k].grad = None
        loss, _ = sl(gt, reen, 1.0, 0.5, 2.0)
        loss.backward()
        return loss.detach().clone(), [reen[k].grad.clone() for k in ('shape', 'exp', 'pose')]

    l1, g1 = step()
    l2, g2 = step()
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l3, g3 = step()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(l1, l3) and all(torch.equal(a, b) for a, b in zip(g1, g3))
    for k in ('shape', 'exp', 'pose'):
        reen[k].grad = None
    graph = torch.cuda.CUDAGraph()
    with F_.capture_graph(graph):
        lg, _ = sl(gt, reen, 1.0, 0.5, 2.0)
        lg.backward()
    gg = [reen[k].grad for k in ('shape', 'exp', 'pose')]
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lg.detach(), l1) and all(torch.equal(a, b) for a, b in zip(gg, g1))


def test_nothing_is_saved_without_a_gradient_and_buffer_edits_rebuild_the_pack():
    from stylegan_directions_face_reenactment_amd import flame as FL
    m = FL.FLAME()
    m.load_state_dict(flame_state(SEED))
    m = m.cuda()
    c = _cuda(S.synthetic_flame_coeffs(SEED, 'flame.save', 3), ('shape', 'exp', 'pose'))
    kept = []

    def count(fn):
        kept.clear()
        with torch.autograd.graph.saved_tensors_hooks(lambda x: kept.append(x.numel()) or x, lambda x: x):
            fn()
        return sum(kept)

    assert count(lambda: FL.decode(m, c)) > 0
    with torch.no_grad():
        assert count(lambda: FL.decode(m, c)) == 0
        assert count(lambda: FL.ShapeLoss(m)(c, c)) == 0
        out = FL.decode(m, c)
    assert all(o.grad_fn is None for o in out)
    plain = {k: v.detach() for k, v in c.items()}
    assert count(lambda: FL.decode(m, plain)) == 0 and count(lambda: FL.ShapeLoss(m)(plain, plain)) == 0
    pack = m.packed()
    assert m.packed() is pack
    with torch.no_grad():
        m.v_template[:, 0] += 0.01
    tv2 = FL.decode(m, plain)[2]
    assert m.packed() is not pack
    assert float((tv2 - out[2]).abs().max()) > 1.0            # 0.01 * 8 * 112 pixels
    assert m.cpu()._pack is None


def test_shape_loss_is_at_most_ten_launches():
    from stylegan_directions_face_reenactment_amd import flame as FL
    from torch.profiler import ProfilerActivity, profile
    m = _module(SEED)
    sl = FL.ShapeLoss(m)
    gt = _cuda(S.synthetic_flame_coeffs(SEED, 'flame.n.gt', 16))
    reen = _cuda(S.synthetic_flame_coeffs(SEED, 'flame.n.re', 16), ('shape', 'exp', 'pose'))
    sl(gt, reen)[0].backward()
    torch.cuda.synchronize()
    for k in ('shape', 'exp', 'pose'):
        reen[k].grad = None
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        sl(gt, reen)[0].backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
    own = [n for n in names if 'flame_' in n]
    print('ShapeLoss forward + backward: %d device kernels, %d of them csrc/flame.hip: %s' % (len(names), len(own), names))
    assert len(own) == 7 and len(names) <= 10


def test_trainer_direction_step_matches_the_torch_composition():
    """ShapeLoss(coefficients of G(z, shift = A(sv))) back to the direction matrix A (trainer.py:175-189), a small seeded Linear on
    mean-pooled pixels standing for the coefficient encoder: dL/dA with the fused ShapeLoss against the same step with the torch
    composition of the reference's losses on flame.decode, within 1e-3 relative (the bar of test_trainer_direction_step_matches_the_stock_head
    for the same comparison through the same generator backward).  Measured on an MI355X: 9.6e-8."""
    from stylegan_directions_face_reenactment_amd import flame as FL
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    m = _module(SEED)
    sl = FL.ShapeLoss(m)
    G = hip_generator(256, 1)
    for p in G.parameters():
        p.requires_grad_(False)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(SEED, num_layers=8))
    A = A.cuda()
    B = 4
    enc = torch.nn.Linear(3 * 8 * 8, 159).cuda()
    with torch.no_grad():
        enc.weight.copy_(S.counter_tensor(SEED, 'flame.enc.w', (159, 192), 0.0, 0.3))
        enc.bias.copy_(S.counter_tensor(SEED, 'flame.enc.b', (159,), 0.0, 0.2))
    for p in enc.parameters():
        p.requires_grad_(False)
    zs = S.synthetic_z(SEED, B, key='flame.zs').cuda()
    sv = S.counter_tensor(SEED, 'flame.sv', (B, 15), 0.0, 3.0).cuda()
    trunc = S.counter_tensor(SEED, 'flame.trunc', (1, 512)).cuda()
    gt = _cuda(S.synthetic_flame_coeffs(SEED, 'flame.tr.gt', B, [0.4, -0.3, 0.1, -0.6]))

    def coefficients(img):
        p = enc(torch.nn.functional.adaptive_avg_pool2d(img, 8).flatten(1))
        return {'shape': p[:, :100], 'exp': p[:, 100:150], 'pose': 0.3 * p[:, 150:156], 'cam': p[:, 156:159].contiguous()}

    grads = []
    for fused in (True, False):
        A.zero_grad()
        img, _ = generate_image(G, zs, 0.7, trunc, shift_code=A(sv), input_is_latent=False, return_latents=True)
        c = coefficients(img)
        if fused:
            loss, _ = sl(gt, c, 1.0, 1.0, 1.0)
        else:
            ls, lm, le = _composition(m, gt, c)
            loss = lm + ls + le
        loss.backward()
        grads.append(torch.cat([p.grad.flatten() for p in A.parameters()]))
    assert float(grads[1].abs().max()) > 0
    rel = _rel(grads[0], grads[1])
    print('trainer step: dL/dA fused ShapeLoss vs torch composition rel %.3e' % rel)
    assert rel <= 1e-3

"""CPU: the DECA coefficient-encoder head without a GPU -- the fp64 restatement (tests/deca_restatement.py) against the fixture
kat12 written from the reference's own ResnetEncoder and rotation_converter (scripts/make_golden_deca.py), the module's key list,
crop_matrix against a least-squares similarity fit and against F.affine_grid + F.grid_sample, the refused configurations,
pickling, the synthetic state's scale and the C ABI of csrc/deca.hip."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from util import S, golden
import deca_restatement as R

from stylegan_directions_face_reenactment_amd import deca as D

KAT = 'kat12_deca_encoder.npz'


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def state(kat):
    return S.synthetic_deca_encoder_state(int(kat['seed']))


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_matches_reference_fixture(kat, state, name):
    """fp64 restatement (crop_matrix + grid_sample front, BatchNorm unfolded) against the reference's fp64 run: parameters and the
    windowed dL/dx within 1e-9 of their maxima, angles within one fp32 ulp (the reference stores them in a float32 tensor)."""
    x, boxes, g = R.fixture_inputs(S, int(kat['seed']), name)
    assert np.array_equal(boxes.numpy(), kat['boxes_' + name])
    H, W = x.shape[2:]
    M = D.crop_matrix(boxes, (H, W), dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    rec = R.run(state, xr, M)
    ref = torch.from_numpy(kat['params_' + name])
    err = float((rec['params'].detach() - ref).abs().max() / ref.abs().max())
    print('parameters: %.3g of max' % err)
    assert err <= 1e-9
    ang = torch.from_numpy(kat['angles_' + name])
    aerr = (rec['angles'] - ang).abs()
    assert bool((aerr <= 2.0 ** -22 * ang.abs().clamp(min=1.0)).all()), float(aerr.max())
    (rec['params'] * g.double()).sum().backward()
    dx = xr.grad
    wy, wx = R.window(name)
    scale = float(kat['dx_max_' + name])
    werr = float((dx[0, :, wy, wx] - torch.from_numpy(kat['dx_window_' + name]).double()).abs().max()) / scale
    print('dL/dx window: %.3g of max' % werr)
    assert werr <= 2.0 ** -23                       # the window is stored in float32
    sums = torch.from_numpy(kat['dx_abs_sum_' + name])
    assert float(((dx.abs().sum((1, 2, 3)) - sums).abs() / sums).max()) <= 1e-9
    assert int(torch.count_nonzero(dx[x.abs() > 1])) == 0
    if name == 'a':                                 # folded BatchNorm (what the kernels run) is the same function
        with torch.no_grad():
            folded = R.run(state, x.double(), M, fold=True)['params']
        assert float((folded - ref).abs().max() / ref.abs().max()) <= 1e-9


def test_restatement_under_its_own_decisions_gives_the_same_gradient(kat, state):
    """The masked form of the restatement (ReLU as a multiplication, max-pool as a gather) with the decisions of the plain form
    is the same function and has the same gradient."""
    x, boxes, g = R.fixture_inputs(S, int(kat['seed']), 'a')
    M = D.crop_matrix(boxes, x.shape[2:], dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    rec = R.run(state, xr, M)
    (rec['params'] * g.double()).sum().backward()
    pres = R.relu_decisions(rec)
    masks = {'stem': pres[0] > 0, 'arg': rec['arg'], 'm1': [p > 0 for p in pres[1:-1:3]], 'm2': [p > 0 for p in pres[2:-1:3]],
             'm3': [p > 0 for p in pres[3:-1:3]], 'fc': pres[-1] > 0}
    x2 = x.double().requires_grad_(True)
    rec2 = R.run(state, x2, M, masks=masks)
    (rec2['params'] * g.double()).sum().backward()
    assert float((rec2['params'] - rec['params']).abs().max()) <= 1e-12
    assert float((x2.grad - xr.grad).abs().max()) <= 1e-12 * float(xr.grad.abs().max()) + 1e-18


def test_key_list_and_shapes_match_the_reference_module(kat):
    ours = ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in D.ResnetEncoder().state_dict().items()]
    assert ours == [str(k) for k in kat['keys']]
    assert len(ours) == 322
    assert sum(p.numel() for p in D.ResnetEncoder().parameters()) == 25848108


def test_crop_matrix_closed_form_against_similarity_fit_and_grid_sample():
    boxes = torch.tensor([[60.0, 80.0, 290.0, 300.0], [70.0, 40.0, 230.0, 180.0], [20.5, 30.25, 180.0, 171.5], [-30.0, -10.0, 90.0, 120.0]],
                         dtype=torch.float64)
    for H, W in ((256, 256), (200, 300)):
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
        ramp = torch.stack([xx, yy])[None]
        u = torch.arange(224, dtype=torch.float64)
        vv, uu = torch.meshgrid(u, u, indexing='ij')
        for b in range(boxes.shape[0]):
            T = R.box_transform(boxes[b].tolist())
            # the fit through the three corner points is exact: scale (crop - 1) / size, no rotation
            left, top, right, bottom = boxes[b].tolist()
            size = int((right - left + bottom - top) / 2 * 1.1 * 1.25)
            s = 223.0 / size
            cx, cy = right - (right - left) / 2, bottom - (bottom - top) / 2
            want = np.array([[s, 0, -s * (cx - size / 2)], [0, s, -s * (cy - size / 2)], [0, 0, 1]])
            assert np.abs(T - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
            theta = torch.tensor(T, dtype=torch.float64)[None, :2]
            for ac in (False, True):
                M = D.crop_matrix(boxes[b:b + 1], (H, W), align_corners=ac, dtype=torch.float64)[0]
                sx = M[0, 0] * uu + M[0, 1] * vv + M[0, 2]
                sy = M[1, 0] * uu + M[1, 1] * vv + M[1, 2]
                out = R.warp_affine_composed(ramp, theta, align_corners=ac)[0]
                inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
                assert int(inside.sum()) > 1000
                assert float((out[0] - sx)[inside].abs().max()) <= 1e-9 * W
                assert float((out[1] - sy)[inside].abs().max()) <= 1e-9 * H
    M32 = D.crop_matrix(boxes, (256, 256))
    assert M32.dtype == torch.float32 and tuple(M32.shape) == (4, 2, 3)
    with pytest.raises(ValueError):
        D.crop_matrix(torch.zeros(4), (256, 256))


def test_front_restatement_equals_the_composed_warp(kat):
    """tests/deca_restatement.front with crop_matrix's matrix is the reference's range map + composed warp_affine + / 255."""
    x, boxes, _ = R.fixture_inputs(S, int(kat['seed']), 'b')
    x = x.double()
    M = D.crop_matrix(boxes, x.shape[2:], dtype=torch.float64)
    mine = R.front(x, M)
    v = (x.clamp(-1, 1) + 1) / (2 + 1e-5) * 255.0
    for b in range(x.shape[0]):
        theta = torch.tensor(R.box_transform(boxes[b].tolist()), dtype=torch.float64)[None, :2]
        want = R.warp_affine_composed(v[b:b + 1], theta) / 255.0
        assert float((mine[b:b + 1] - want).abs().max()) <= 1e-10


def test_refused_configurations_raise_before_any_launch():
    with pytest.raises(NotImplementedError):
        D.ResnetEncoder(outsize=512)
    with pytest.raises(NotImplementedError):
        D.ResnetEncoder(outsize=236, last_op=torch.tanh)
    E = D.ResnetEncoder()
    assert not any(p.requires_grad for p in E.parameters())
    x, M = torch.zeros(1, 3, 256, 256), torch.zeros(1, 2, 3)
    with pytest.raises(RuntimeError, match='eval mode'):
        D.encode(E, x, M)                                  # a fresh module is in training mode
    E.eval()
    E.layers[0].weight.requires_grad = True
    with pytest.raises(RuntimeError, match='no gradient for the encoder weights'):
        D.calculate_shapemodel(E, x, M)
    E.layers[0].weight.requires_grad = False
    with pytest.raises(RuntimeError, match='no CPU path'):
        D.encode(E, x, M)
    E.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        E(x, M)


def test_deepcopy_and_pickle_drop_the_pack():
    E = D.ResnetEncoder().eval()
    E._pack = ('key', torch.zeros(1), [])
    E2 = pickle.loads(pickle.dumps(E))
    assert E2._pack is None and not E2.training
    E3 = copy.deepcopy(E)
    assert E3._pack is None
    assert list(E2.state_dict().keys()) == list(E.state_dict().keys())
    E.load_state_dict(E.state_dict())
    assert E._pack is None


def test_split_parameters_follows_param_list():
    p = torch.arange(2 * 236, dtype=torch.float32).view(2, 236)
    code = D.split_parameters(p)
    assert [(k, tuple(v.shape[1:])) for k, v in code.items()] == [('shape', (100,)), ('tex', (50,)), ('exp', (50,)), ('pose', (6,)),
                                                                  ('cam', (3,)), ('light', (9, 3))]
    assert float(code['pose'][0, 0]) == 200.0 and float(code['cam'][1, 0]) == 236 + 206.0


def test_synthetic_state_keeps_activations_in_range(state):
    """fp32 on the CPU, one 224^2 crop: the rms of every bottleneck's output stays within [0.1, 10], the parameters are O(1)."""
    crop = S.counter_tensor(7, 'deca.scale.crop', (1, 3, 224, 224), 0.5, 0.25).clamp(0, 1)
    with torch.no_grad():
        rec = R.encoder(state, crop)
    rms = [float(o.pow(2).mean().sqrt()) for o in rec['out']]
    print('stage rms', ['%.2f' % r for r in rms], 'max |parameters| %.2f' % float(rec['params'].abs().max()))
    assert all(0.1 <= r <= 10 for r in rms), rms
    assert 0.05 <= float(rec['params'].abs().max()) <= 50
    again = S.synthetic_deca_encoder_state(int(golden(KAT)['seed']))
    assert torch.equal(again['encoder.layer3.4.conv2.weight'], state['encoder.layer3.4.conv2.weight'])


def test_angles_restatement_branches():
    import math
    pose = torch.tensor([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1], [0.0, -math.pi / 2, 0.0], [0.0, math.pi / 2, 0.0]], dtype=torch.float64)
    a = R.angles(pose)
    assert float(a[0].abs().max()) == 0.0
    assert abs(float(a[2, 0]) - 90.0) < 1e-9 and float(a[2, 2]) == 0.0          # R20 = -2wy = 1 > 0.998
    assert abs(float(a[3, 0]) + 90.0) < 1e-9 and float(a[3, 2]) == 0.0
    assert 5 < float(a[1].abs().max()) < 30


def test_native_symbols_and_sizes():
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    for name in ('sgdfr_deca_pack_elems', 'sgdfr_deca_saved_elems', 'sgdfr_deca_debug_elems', 'sgdfr_deca_workspace_bytes',
                 'sgdfr_deca_prepack_f32', 'sgdfr_deca_forward_f32', 'sgdfr_deca_backward_f32'):
        assert hasattr(lib, name), name
    assert _native.DECA_PARAMS == 134 == len(D.ResnetEncoder().folded())
    n_params = sum(p.numel() for p in D.ResnetEncoder().parameters())
    assert 1.9 * n_params < lib.sgdfr_deca_pack_elems() < 2.1 * n_params      # forward + input-gradient weights
    for rows in (1, 3):
        saved = torch.zeros(lib.sgdfr_deca_saved_elems(rows), dtype=torch.uint8)
        v = D.saved_views(saved, rows)                                        # asserts the total
        assert len(v['m1']) == len(v['m2']) == len(v['m3']) == 16
        decisions = sum(t.numel() for k in ('m1', 'm2', 'm3') for t in v[k]) + v['stem'].numel() + v['fc'].numel()
        want, h = 64 * 112 * 112 + 1024, 56                                   # stem, regressor, 3 per bottleneck
        for i, (planes, count) in enumerate(R.LAYERS):
            for k in range(count):
                ho = h // 2 if (k == 0 and i > 0) else h
                want += planes * h * h + planes * ho * ho + 4 * planes * ho * ho
                h = ho
        assert decisions == rows * want == rows * 9609728
        D.debug_views(torch.zeros(lib.sgdfr_deca_debug_elems(rows)), rows)
    assert lib.sgdfr_deca_saved_elems(0) == -1 and lib.sgdfr_deca_workspace_bytes(1, 0, 256) == -1
    assert lib.sgdfr_deca_workspace_bytes(2, 256, 256) > lib.sgdfr_deca_workspace_bytes(1, 256, 256) > 0
    rc = lib.sgdfr_deca_forward_f32(None, None, 1, 256, 256, None, None, None, None, None, None, None, 0, None)
    assert rc != 0 and b'null pointer' in lib.sgdfr_last_error()
    rc = lib.sgdfr_deca_backward_f32(None, None, None, None, 0, 256, 256, None, None, None, 0, None)
    assert rc != 0 and b'unsupported size' in lib.sgdfr_last_error()
    arr = (ctypes.c_void_p * _native.DECA_PARAMS)()
    rc = lib.sgdfr_deca_prepack_f32(arr, ctypes.c_void_p(8), None)
    assert rc != 0 and b'parameter 0 is null' in lib.sgdfr_last_error()


def test_plan_rule_reproduces_the_documented_split_counts():
    """The split-K rule as test_gpu_deca_fan_plans restates it (the GPU tests assert the counted finish launches against it) gives
    DESIGN 4.15's counts -- 45 / 44 convs split K at B = 1, 43 / 41 at 3, 18 / 17 at 16 and 17, 2 / 1 at 48 (of 55 / 50) -- and
    4.16's: 188, 165, 132, 108, 96 of 191."""
    import test_gpu_deca_fan_plans as P
    fwd, bwd = P.deca_layers()
    assert (len(fwd), len(bwd), len(P.fan_layers())) == (55, 50, 191)
    deca = [(P.planned_finishes(fwd, B), P.planned_finishes(bwd, B)) for B in P.ROW_COUNTS]
    fan = [P.planned_finishes(P.fan_layers(), B) for B in P.ROW_COUNTS]
    print('plan rule: deca finishes forward / backward %s; fan %s' % (deca, fan))
    assert P.ROW_COUNTS == (1, 3, 16, 17, 48)
    assert deca == [(45, 44), (43, 41), (18, 17), (18, 17), (2, 1)]
    assert fan == [188, 165, 132, 108, 96]

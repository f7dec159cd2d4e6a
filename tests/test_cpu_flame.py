"""CPU: the FLAME decode and shape losses -- the fp64 restatement of the tests (flame_restatement.py) against the reference's own
DECA.decode and Losses (tests/golden/kat11_flame.npz, scripts/make_golden_flame.py), the seeded synthetic FLAME model and its two
files, the host contract of flame.FLAME / decode / ShapeLoss, and the C ABI of csrc/flame.hip."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

from util import ROOT, S, golden, t
import flame_restatement as R

_STATE = {}


def flame_state(seed):
    if seed not in _STATE:
        _STATE[seed] = S.synthetic_flame_state(seed)
    return _STATE[seed]


def kat_inputs(g):
    seed, rows = int(g['seed']), int(g['rows'])
    gt = S.synthetic_flame_coeffs(seed, str(g['gt_key']), rows, g['yaw_gt'])
    reen = S.synthetic_flame_coeffs(seed, str(g['reen_key']), rows, g['yaw_reen'])
    return gt, reen


def _close(a, b, tol=1e-9):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    rel = float((a - b).abs().max() / b.abs().max())
    assert rel <= tol, rel


def test_restatement_matches_the_reference_decode_and_losses():
    g = golden('kat11_flame.npz')
    T = R.tables(flame_state(int(g['seed'])))
    gt, reen = kat_inputs(g)
    cg = R.fixed_cam({k: v.double() for k, v in gt.items()})
    cr = R.fixed_cam({k: v.double().requires_grad_(k != 'cam') for k, v in reen.items()})
    l2g, _, tvg, og = R.decode(T, cg)
    l2r, l3r, tvr, orr = R.decode(T, cr)
    stride = int(g['stride'])
    _close(orr['vertices'].detach()[:, ::stride], g['vertices'])
    _close(tvr.detach()[:, ::stride], g['trans_verts'])
    _close(l2r.detach(), g['landmarks2d'])
    _close(l3r.detach(), g['landmarks3d'])
    assert torch.equal(og['dyn'], t(g['dyn_gt'])) and torch.equal(orr['dyn'], t(g['dyn_reen']))
    ls, lm, le = R.losses(l2g, tvg, l2r, tvr)
    _close(ls.detach(), g['loss_shape'])
    _close(lm.detach(), g['loss_mouth'])
    _close(le.detach(), g['loss_eye'])
    total = lm + ls + le
    _close(total.detach(), g['total'])
    total.backward()
    for k in ('shape', 'exp', 'pose'):
        _close(cr[k].grad, g['grad_' + k])
    # the fixture's own conditions: four branches of the contour-row remap, room at every rounding, no term near zero
    deg = orr['deg'].detach()
    assert bool((deg < -39.5).any()) and bool(((deg > -39) & (deg < 0)).any()) and bool(((deg > 0) & (deg < 39)).any()) and bool((deg > 39.5).any())
    for d in (deg, og['deg']):
        assert float((d - torch.floor(d) - 0.5).abs().min()) >= 0.05
    assert float((tvg - tvr).detach().abs().min()) >= 8 * float(g['dev_trans_verts'])
    assert min(float(g['loss_shape']), float(g['loss_mouth']), float(g['loss_eye'])) >= 0.05


def test_forced_decisions_reproduce_the_free_run():
    g = golden('kat11_flame.npz')
    T = R.tables(flame_state(int(g['seed'])))
    gt, reen = kat_inputs(g)
    cg, cr = R.fixed_cam({k: v.double() for k, v in gt.items()}), R.fixed_cam({k: v.double() for k, v in reen.items()})
    l2g, _, tvg, _ = R.decode(T, cg)
    l2r, _, tvr, _ = R.decode(T, cr, dyn=g['dyn_reen'])
    ls, lm, _ = R.losses(l2g, tvg, l2r, tvr)
    assert float(R.shape_term(tvg, tvr, torch.sign(tvg - tvr))) == pytest.approx(float(ls), rel=1e-12)
    signs = []
    for a, b in R.MOUTH_PAIRS:
        dr = l2r[:, a] - l2r[:, b]
        signs.append((torch.sign((l2g[:, a] - l2g[:, b]).abs() - dr.abs()), torch.sign(dr)))
    assert float(R.pair_term(l2g, l2r, R.MOUTH_PAIRS, signs)) == pytest.approx(float(lm), rel=1e-12)


def test_synthetic_flame_state_is_pinned_and_round_trips_through_the_files(tmp_path):
    from stylegan_directions_face_reenactment_amd import flame as FL
    g = golden('kat11_flame.npz')
    sd = flame_state(int(g['seed']))
    again = S.synthetic_flame_state(int(g['seed']))
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    other = S.synthetic_flame_state(int(g['seed']) + 1)
    assert not torch.equal(sd['v_template'], other['v_template'])
    # element values of the counter generator (exact on any host)
    assert sd['v_template'][0, 0].item() == S.counter_tensor(int(g['seed']), 'flame.v_template', (1,), 0.0, 0.08).item()
    assert abs(float(sd['v_template'].std()) - 0.08) < 0.004 and abs(float(sd['shapedirs'].std()) - 0.002) < 1e-4
    assert float((sd['J_regressor'].sum(1) - 1).abs().max()) < 1e-5 and float(sd['J_regressor'].min()) >= 0
    assert float((sd['lbs_weights'].sum(1) - 1).abs().max()) < 1e-5 and float(sd['lbs_weights'].min()) >= 0
    for k in ('lmk_bary_coords', 'dynamic_lmk_bary_coords', 'full_lmk_bary_coords'):
        assert float((sd[k].sum(-1) - 1).abs().max()) < 1e-5 and float(sd[k].min()) > 0
    assert 0 <= int(sd['faces_tensor'].min()) and int(sd['faces_tensor'].max()) < FL.V
    for k in ('lmk_faces_idx', 'dynamic_lmk_faces_idx', 'full_lmk_faces_idx'):
        assert 0 <= int(sd[k].min()) and int(sd[k].max()) < FL.FACES
    pkl, npy = S.write_flame_files(sd, str(tmp_path))
    m = FL.FLAME.from_files(pkl, npy)
    msd = m.state_dict()
    assert ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in msd.items()] == [str(k) for k in g['keys']]
    for k, v in sd.items():
        assert torch.equal(msd[k], v), k
    # a state dict in the reference's keys loads; a scipy-sparse or dense regressor reads the same
    m2 = FL.FLAME()
    m2.load_state_dict(sd)
    assert torch.equal(m2.shapedirs, sd['shapedirs'])
    m3 = pickle.loads(pickle.dumps(m2))
    assert m3._pack is None and torch.equal(m3.v_template, sd['v_template'])


def test_refused_configurations_and_cpu_inputs():
    from stylegan_directions_face_reenactment_amd import flame as FL
    with pytest.raises(NotImplementedError, match='n_shape'):
        FL.FLAME(n_shape=300)
    with pytest.raises(NotImplementedError, match='vertices'):
        FL.FLAME(n_vertices=1000)
    m = FL.FLAME()
    m.load_state_dict(flame_state(3))
    c = S.synthetic_flame_coeffs(3, 'cpu', 2)
    with pytest.raises(RuntimeError, match='no CPU path'):
        m(c['shape'], c['exp'], c['pose'])
    with pytest.raises(RuntimeError, match='no CPU path'):
        FL.decode(m, c)
    with pytest.raises(RuntimeError, match='no CPU path'):
        FL.ShapeLoss(m)(c, c)
    with pytest.raises(NotImplementedError, match='224'):
        FL.decode(m, c, image_size=256)
    with torch.no_grad():
        m.neck_pose[0, 1] = 0.1
    with pytest.raises(ValueError, match='neck_pose'):
        m.folded()


def test_folded_tables_restate_the_joint_regressor_and_the_landmark_index():
    from stylegan_directions_face_reenactment_amd import flame as FL
    sd = flame_state(3)
    m = FL.FLAME()
    m.load_state_dict(sd)
    ps = m.folded()
    assert len(ps) == 15
    betas = S.counter_tensor(3, 'fold.betas', (150,)).double()
    v_shaped = sd['v_template'].double() + torch.einsum('vkl,l->vk', sd['shapedirs'].double(), betas)
    J = sd['J_regressor'].double() @ v_shaped
    Jf = ps[4].double().view(5, 3) + (ps[5].double() @ betas).view(5, 3)
    assert float((J - Jf).abs().max()) <= 1e-6 * float(J.abs().max())
    # inverse landmark index: every (slot, corner) appears once under its vertex, in slot order
    off, slots, w = ps[12].long(), ps[13].long(), ps[14]
    assert off[0] == 0 and off[-1] == FL.N_CSR == slots.numel() and bool((off[1:] >= off[:-1]).all())
    corners = torch.cat([ps[6], ps[8], ps[10]]).long().view(-1, 3)
    bary = torch.cat([ps[7], ps[9], ps[11]]).view(-1, 3)
    vert_of_entry = torch.repeat_interleave(torch.arange(FL.V), off[1:] - off[:-1])
    assert bool((corners[slots] == vert_of_entry[:, None]).any(1).all())
    assert float(w.sum()) == pytest.approx(float(bary.sum()), rel=1e-5)
    assert torch.equal(torch.bincount(slots, minlength=corners.shape[0]), torch.full((corners.shape[0],), 3))


def test_entry_points_are_declared_exported_and_validate():
    from stylegan_directions_face_reenactment_amd import _native
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    declared = set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header))
    names = {'sgdfr_flame_pack_elems', 'sgdfr_flame_saved_elems', 'sgdfr_flame_workspace_bytes', 'sgdfr_flame_prepack_f32',
             'sgdfr_flame_decode_f32', 'sgdfr_flame_decode_backward_f32', 'sgdfr_shape_loss_f32'}
    assert names <= declared
    lib = _native.load()
    for n in names:
        assert hasattr(lib, n), n
    assert names - {'sgdfr_flame_pack_elems', 'sgdfr_flame_saved_elems', 'sgdfr_flame_workspace_bytes'} <= set(_native.SIGNATURES)
    assert lib.sgdfr_flame_pack_elems() > 2 * 47 * 15069 * 4
    assert lib.sgdfr_flame_saved_elems(3) == 3 * (256 + 2 * 15069) and lib.sgdfr_flame_saved_elems(0) < 0
    assert lib.sgdfr_flame_workspace_bytes(16) > 0 and lib.sgdfr_flame_workspace_bytes(-1) < 0
    one = ctypes.c_void_p(64)                                  # a non-NULL pointer that is never dereferenced: validation fails first
    arr = (ctypes.c_void_p * _native.FLAME_PARAMS)(*[64] * _native.FLAME_PARAMS)
    assert lib.sgdfr_flame_prepack_f32(arr, 5023, 150, 36, 5, 79, 4386, None, None) != 0 and b'NULL' in lib.sgdfr_last_error()
    assert lib.sgdfr_flame_prepack_f32(arr, 1000, 150, 36, 5, 79, 4386, one, None) != 0 and b'sizes' in lib.sgdfr_last_error()
    arr[3] = None
    assert lib.sgdfr_flame_prepack_f32(arr, 5023, 150, 36, 5, 79, 4386, one, None) != 0 and b'table 3' in lib.sgdfr_last_error()
    rc = lib.sgdfr_flame_decode_f32(one, one, one, 0, None, None, None, 0, one, one, 1, one, one, one, one, None)
    assert rc != 0 and b'rows=0' in lib.sgdfr_last_error()
    rc = lib.sgdfr_flame_decode_f32(one, one, None, 2, None, None, None, 0, one, one, 1, one, one, one, one, None)
    assert rc != 0 and b'NULL' in lib.sgdfr_last_error()
    rc = lib.sgdfr_flame_decode_f32(one, one, one, 2, None, None, None, 0, None, one, 1, one, one, one, one, None)
    assert rc != 0 and b'cam' in lib.sgdfr_last_error()
    rc = lib.sgdfr_flame_decode_backward_f32(None, None, None, None, 2, one, 1, one, one, one, one, None, one, 16, None)
    assert rc != 0 and b'workspace' in lib.sgdfr_last_error()
    rc = lib.sgdfr_shape_loss_f32(one, one, -3, 1.0, 1.0, 1.0, one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'rows=-3' in lib.sgdfr_last_error()
    rc = lib.sgdfr_shape_loss_f32(None, one, 2, 1.0, 1.0, 1.0, one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'NULL' in lib.sgdfr_last_error()

"""GPU: the ground-truth coefficients of the `disentanglement_50` step built on the device (csrc/shift.hip gt_reenacted_kernel through
ShiftVectors.get_params_gt_reenacted) against the fixture kat18, written from the reference's own get_params_gt_reenacted on CPU
tensors (scripts/make_golden_gt_coeffs.py).

Bars (test_cpu_gt_coeffs.check_against_fixture).  Rows of the first half, untouched entries, jaw and expression entries: bit-identical
to the reference's float32.  The three rotated pose entries of a row whose direction is a pose angle: |HIP - ref32| <= 4 * d_ref with
d_ref = the reference's own max |float32 - float64| on those entries, read from the fixture.  The margin of 4: both sides carry their
own rounding through six sin / cos calls and an atan2, and the device's and the host's libm differ by an ulp or two in each; a wrong
branch or a wrong swap is off by 1e-1 or more.  Every test prints the figure it asserts on.
"""
import numpy as np
import pytest
import torch

from util import golden
from test_cpu_gt_coeffs import KAT, SETTINGS, builder, case, check_against_fixture, tag_of

pytestmark = pytest.mark.gpu


def _cuda(par_s, par_t, shift, which, ang_s):
    cu = lambda d: {k: v.cuda() for k, v in d.items()}
    return cu(par_s), cu(par_t), shift.cuda(), which, ang_s.cuda()


@pytest.mark.parametrize('dataset,D,sc', SETTINGS)
def test_kernel_against_the_reference(dataset, D, sc):
    g = golden(KAT)
    tag = tag_of(dataset, D, sc)
    sv = builder(dataset, D, sc)
    par_s, par_t, shift, which, ang_s = _cuda(*case(g, tag))
    keep = {id(v): v.clone() for v in list(par_s.values()) + list(par_t.values())}
    out = sv.get_params_gt_reenacted(par_s, par_t, shift, which, ang_s)
    assert sorted(out) == ['exp', 'pose'] and out['pose'].is_cuda and out['pose'].shape == (16, 6) and out['exp'].shape == (16, 50)
    check_against_fixture(g, tag, out['pose'].cpu().numpy(), out['exp'].cpu().numpy(), 'HIP')
    zero = out['pose'][8, :3].cpu()
    assert (zero == 0).all()                                               # (0, 0, 0) with no shift: the k = 2 branch, no NaN
    # the source and target dicts are left alone, bit for bit
    for v in list(par_s.values()) + list(par_t.values()):
        assert torch.equal(v.view(torch.int32), keep[id(v)].view(torch.int32))
    # target_indices as a device tensor (int32 and int64), a numpy array and a list: the same output
    for idx in (torch.from_numpy(which).cuda(), torch.from_numpy(which).to(torch.int32).cuda(), which.astype(np.int32), which.tolist()):
        again = sv.get_params_gt_reenacted(par_s, par_t, shift, idx, ang_s)
        assert torch.equal(again['pose'].view(torch.int32), out['pose'].view(torch.int32))
        assert torch.equal(again['exp'].view(torch.int32), out['exp'].view(torch.int32))
    # ... and the indices make_shift_vector_50 hands back feed it directly
    sv50, idx = sv.make_shift_vector_50(par_s, par_t, ang_s, t_ang(g, tag), target_indices=which, u=torch.from_numpy(g[tag + '.u']).cuda())
    assert (sv50.cpu().numpy() == g[tag + '.shift']).all() and idx.dtype == torch.int32 and idx.is_cuda
    chained = sv.get_params_gt_reenacted(par_s, par_t, sv50, idx, ang_s)
    assert torch.equal(chained['pose'], out['pose']) and torch.equal(chained['exp'], out['exp'])


def t_ang(g, tag):
    return torch.from_numpy(g[tag + '.ang_t']).cuda()


def test_smallest_batch_and_undriven_indices():
    """B = 2, one row per half: row 0 is the target's, row 1 the source's moved along its direction -- the fixture's rows 0 and 9
    (injected angles (170, 150, 20), the cos_theta < 0 branch).  An index outside the table leaves the source copy, as the
    reference's chain of ifs does."""
    g = golden(KAT)
    dataset, D, sc = SETTINGS[0]
    tag = tag_of(dataset, D, sc)
    sv = builder(dataset, D, sc)
    par_s, par_t, shift, which, ang_s = case(g, tag)
    rows = [0, 9]
    pick = lambda d: {k: v[rows].contiguous().cuda() for k, v in d.items()}
    ps, pt = pick(par_s), pick(par_t)
    out = sv.get_params_gt_reenacted(ps, pt, shift[rows].contiguous().cuda(), which[1:2], ang_s[rows].contiguous().cuda())
    pose, exp = out['pose'].cpu().numpy(), out['exp'].cpu().numpy()
    assert pose.shape == (2, 6) and exp.shape == (2, 50)
    assert (pose[0] == g[tag + '.pose'][0]).all() and (exp == g[tag + '.exp'][rows]).all() and (pose[1, 3:] == g[tag + '.pose'][9, 3:]).all()
    err = float(np.abs(pose[1, :3].astype(np.float64) - g[tag + '.pose'][9, :3]).max())
    print('B=2: rotated entries max |HIP - ref32| %.3e   bar %.3e' % (err, 4 * float(g['d_ref'])))
    assert err <= 4 * float(g['d_ref'])
    for outside in (-1, D, 63, 1 << 20):
        same = sv.get_params_gt_reenacted(ps, pt, shift[rows].contiguous().cuda(), [outside], ang_s[rows].contiguous().cuda())
        assert torch.equal(same['pose'][1], ps['pose'][1]) and torch.equal(same['exp'][1], ps['alpha_exp'][1])
        assert torch.equal(same['pose'][0], pt['pose'][0])
    with pytest.raises(RuntimeError):
        sv.get_params_gt_reenacted(ps, pt, shift[rows][:, :5].contiguous().cuda(), which[1:2], ang_s[rows].contiguous().cuda())


def test_direction_losses_ground_truth_set():
    """DirectionLosses.coefficients_gt: with disentanglement_50 the set of get_params_gt_reenacted, without it the target's pose and
    expression themselves (utils_train.py:387-391); the shape is the source's alpha_shp either way (:395)."""
    from stylegan_directions_face_reenactment_amd.train_step import DirectionLosses
    g = golden(KAT)
    dataset, D, sc = SETTINGS[0]
    tag = tag_of(dataset, D, sc)
    sv = builder(dataset, D, sc)
    par_s, par_t, shift, which, ang_s = _cuda(*case(g, tag))
    par_s['alpha_shp'] = torch.arange(1600, dtype=torch.float32).view(16, 100).cuda()
    par_t['alpha_shp'] = -par_s['alpha_shp']
    none = {'lambda_shape': 0.0}
    off = DirectionLosses(None, None, None, sv, none, disentanglement_50=False).coefficients_gt(par_s, par_t, shift, which, ang_s)
    assert off['pose'] is par_t['pose'] and off['exp'] is par_t['alpha_exp'] and off['shape'] is par_s['alpha_shp']
    on = DirectionLosses(None, None, None, sv, none).coefficients_gt(par_s, par_t, shift, which, ang_s)
    want = sv.get_params_gt_reenacted(par_s, par_t, shift, which, ang_s)
    assert torch.equal(on['pose'], want['pose']) and torch.equal(on['exp'], want['exp']) and on['shape'] is par_s['alpha_shp']
    assert not torch.equal(on['pose'], off['pose'])

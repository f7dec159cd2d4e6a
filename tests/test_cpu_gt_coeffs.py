"""CPU: the ground-truth coefficients of the `disentanglement_50` step.  The fixture kat18 (scripts/make_golden_gt_coeffs.py: the
reference's own make_shift_vector_50 and get_params_gt_reenacted on CPU tensors) against the torch restatement
tests/gt_coeffs_restatement.py, and the host contract of ShiftVectors.get_params_gt_reenacted.

Bars.  Copied rows, untouched entries, jaw and expression entries: bit-identical to the reference's float32 (+0 and -0 compare
equal).  The three rotated pose entries of a row whose direction is a pose angle: |restatement - ref32| <= 4 * d_ref, d_ref = the
reference's own max |float32 - float64| over those entries, read from the fixture (4.19e-7 on values up to 2.98); on this side both
run torch's CPU sin / cos / atan2, so the figure printed is 0 on the host that wrote the fixture and an ulp (2.4e-7 was seen) on a
host whose vector width or libm differs."""
import os
import re

import numpy as np
import pytest
import torch

from util import ROOT, golden, t
import gt_coeffs_restatement as R

KAT = 'kat18_gt_coeffs.npz'
SETTINGS = (('voxceleb', 15, 6), ('ffhq', 12, 6.0), ('voxceleb', 15, 4.5))
MARGIN = 4.0


def tag_of(dataset, D, sc):
    return '%s_%d_%s' % (dataset, D, str(sc).replace('.', 'p'))


def builder(dataset, D, sc):
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    return ShiftVectors(dataset, D, sc, ranges=golden('kat8_shift.npz')['ranges_' + dataset])


def case(g, tag, dtype=torch.float32):
    """(source params, target params, shift vector, target_indices, source angles) of one setting as CPU tensors."""
    f = lambda k: t(g[tag + '.' + k]).to(dtype)
    return ({'pose': f('pose_s'), 'alpha_exp': f('exp_s')}, {'pose': f('pose_t'), 'alpha_exp': f('exp_t')}, f('shift'),
            g[tag + '.which'], f('ang_s'))


def rotated_mask(g, tag):
    m = np.zeros(g[tag + '.pose'].shape, dtype=bool)
    m[g[tag + '.rotated_rows'], :3] = True
    return m


def check_against_fixture(g, tag, pose, exp, label):
    """The bars of this module's docstring for one setting; returns the largest deviation on the rotated entries."""
    pose, exp = np.asarray(pose), np.asarray(exp)
    rot = rotated_mask(g, tag)
    assert pose.dtype == np.float32 and exp.dtype == np.float32
    assert (exp == g[tag + '.exp']).all(), '%s %s: expression entries differ' % (label, tag)            # (== : -0 equals +0)
    assert (pose[~rot] == g[tag + '.pose'][~rot]).all(), '%s %s: copied / jaw pose entries differ' % (label, tag)
    err = float(np.abs(pose[rot].astype(np.float64) - g[tag + '.pose'][rot].astype(np.float64)).max())
    bar = MARGIN * float(g['d_ref'])
    print('%s %-18s rotated entries: max |. - ref32| %.3e   bar %.0f x d_ref = %.3e' % (label, tag, err, MARGIN, bar))
    assert err <= bar, (label, tag, err, bar)
    return err


def test_fixture_covers_what_it_claims():
    g = golden(KAT)
    assert abs(float(g['d_ref']) - 4.19e-7) < 0.01e-7 and int(g['rows']) == 16
    angles = set()
    for dataset, D, sc in SETTINGS:
        tag = tag_of(dataset, D, sc)
        sv = builder(dataset, D, sc)
        table = R.directions(sv)
        which = g[tag + '.which'].tolist()
        kinds = [table[w][0] for w in which]
        assert set(kinds) == {'angle', 'jaw', 'exp'} and len(set(which)) < len(which) and D - 1 in which
        assert kinds[:3] == ['angle'] * 3                                  # the three injected rows are rotated
        assert g[tag + '.rotated_rows'].tolist() == [8 + i for i, k in enumerate(kinds) if k == 'angle']
        if dataset == 'voxceleb':
            angles |= {table[w][1] for w in which if table[w][0] == 'angle'}
        else:
            assert table[2][0] == 'jaw' and 2 in which and all(table[w][1] != 2 for w in which if table[w][0] == 'angle')
        assert g[tag + '.ang_s'][8:11].tolist() == [[0, 0, 0], [170, 150, 20], [100, -160, 175]]
        assert float(g[tag + '.u'][0]) == 0.5 and float(g[tag + '.shift'][8, which[0]]) == 0.0
        zero = g[tag + '.pose'][8, :3]
        assert (zero == 0).all() and np.signbit(zero).tolist() == [False, True, False]                 # sin^2 == 0: [0, -0, 0]
        # first half = the target's rows, second half = the source's except what the row's direction moved
        assert (g[tag + '.pose'][:8] == g[tag + '.pose_t'][:8]).all() and (g[tag + '.exp'][:8] == g[tag + '.exp_t'][:8]).all()
        moved = (g[tag + '.pose'][8:] != g[tag + '.pose_s'][8:]).sum() + (g[tag + '.exp'][8:] != g[tag + '.exp_s'][8:]).sum()
        assert 8 <= int(moved) <= 3 * len(g[tag + '.rotated_rows']) + (8 - len(g[tag + '.rotated_rows']))
        assert np.isfinite(g[tag + '.pose']).all() and np.isfinite(g[tag + '.pose64']).all()
    assert angles == {0, 1, 2}                                               # yaw, pitch and roll over the voxceleb settings


@pytest.mark.parametrize('dataset,D,sc', SETTINGS)
def test_restatement_equals_the_reference(dataset, D, sc):
    g = golden(KAT)
    tag = tag_of(dataset, D, sc)
    sv = builder(dataset, D, sc)
    par_s, par_t, shift, which, ang_s = case(g, tag)
    keep = [v.clone() for v in list(par_s.values()) + list(par_t.values())]
    out = R.gt_reenacted(sv, par_s, par_t, shift, which, ang_s)
    check_against_fixture(g, tag, out['pose'].numpy(), out['exp'].numpy(), 'restatement')
    assert all(torch.equal(a, b) for a, b in zip(keep, list(par_s.values()) + list(par_t.values())))
    # ... and in float64, fed the float32 shift vector, it stays within d_ref-sized distance of the reference's float64 run (whose
    # own shift vector was float64: the two differ by that rounding, carried through the rotation)
    par_s, par_t, shift, which, ang_s = case(g, tag, torch.float64)
    out64 = R.gt_reenacted(sv, par_s, par_t, shift, which, ang_s)
    e64 = float(np.abs(out64['pose'].numpy() - g[tag + '.pose64']).max())
    print('restatement float64 %-18s max |. - ref64| over pose %.3e' % (tag, e64))
    assert e64 <= MARGIN * float(g['d_ref'])


def test_host_contract():
    """CPU tensors, an odd batch and a wrong number of target_indices are refused before any launch; the symbol is declared."""
    from stylegan_directions_face_reenactment_amd import _native
    sv = builder('voxceleb', 15, 6)
    g = golden(KAT)
    par_s, par_t, shift, which, ang_s = case(g, tag_of('voxceleb', 15, 6))
    with pytest.raises(RuntimeError, match='no CPU path'):
        sv.get_params_gt_reenacted(par_s, par_t, shift, which, ang_s)
    cut = lambda d, n: {k: v[:n] for k, v in d.items()}
    with pytest.raises(RuntimeError, match='even'):
        sv.get_params_gt_reenacted(cut(par_s, 15), cut(par_t, 15), shift[:15], which[:7], ang_s[:15])
    for bad in (which[:7], list(which) + [0], which.reshape(2, 4)):
        with pytest.raises(RuntimeError, match='target_indices'):
            sv.get_params_gt_reenacted(par_s, par_t, shift, bad, ang_s)
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    assert 'sgdfr_gt_reenacted_f32' in set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header))
    assert 'sgdfr_gt_reenacted_f32' in _native.SIGNATURES and len(_native.SIGNATURES['sgdfr_gt_reenacted_f32']) == 16
    assert hasattr(_native.load(), 'sgdfr_gt_reenacted_f32')
    # argument validation happens before any launch
    lib = _native.load()
    rc = lib.sgdfr_gt_reenacted_f32(None, None, None, None, None, 6, 50, None, None, 6.0, sv._table_train, 15, None, None, 3, None)
    assert rc != 0 and b'even' in lib.sgdfr_last_error()
    rc = lib.sgdfr_gt_reenacted_f32(None, None, None, None, None, 6, 50, None, None, 6.0, sv._table_train, 15, None, None, 4, None)
    assert rc != 0 and b'null' in lib.sgdfr_last_error()
    assert lib.sgdfr_gt_reenacted_f32(None, None, None, None, None, 6, 50, None, None, 6.0, sv._table_train, 15, None, None, 0, None) == 0

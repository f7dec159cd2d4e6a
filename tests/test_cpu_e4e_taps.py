"""CPU: the restatement of the e4e encoder (tests/e4e_restatement.py) against the fixture written from the reference's own module
(tests/golden/kat15_e4e_taps.npz, scripts/make_golden_e4e_taps.py), and the host side of the HIP path: the C ABI's declarations, the
documented parameter layout, and what `encode` refuses."""
import copy
import os
import pickle
import re

import pytest
import torch

from util import ROOT, S, golden
import e4e_restatement as R

BAR = 8.0


@pytest.fixture(scope='module')
def kat():
    return golden(R.KAT)


_ENCODERS = {}


def make_encoder(name):
    """(module, state) of a fixture case, built once per process: the seeded state of 10 heads is 150 M values."""
    if name not in _ENCODERS:
        _ENCODERS[name] = _make_encoder(name)
    return _ENCODERS[name]


def _make_encoder(name):
    from stylegan_directions_face_reenactment_amd.encoder import Encoder4Editing
    enc = Encoder4Editing(50, 'ir_se', R.case(name)[1]).eval()
    state = R.fixture_state(S, name, enc.state_dict())
    enc.load_state_dict(state, strict=True)
    return enc, state


@pytest.fixture(scope='module')
def small():
    return make_encoder('a')


@pytest.mark.parametrize('name', ['a', 'b'])
def test_restatement_against_the_reference_fixture(kat, name):
    """fp64 within 1e-10 max|w| of the reference's fp64 codes (reordering noise); fp32 within 8 x the reference's own
    max |fp32 - fp64|."""
    enc, state = make_encoder(name)
    x = R.fixture_inputs(S, name)
    want = torch.from_numpy(kat['w_' + name])
    top = float(want.abs().max())
    assert abs(top - float(kat['max_w_' + name])) == 0.0
    with torch.no_grad():
        t64 = R.forward(state, x.double())
        t32 = R.forward(state, x)
    e64 = float((t64['w'] - want).abs().max())
    e32 = float((t32['w'].double() - want).abs().max())
    dev = float(kat['dev_w_' + name])
    print('case %s: fp64 restatement %.3e (bar %.3e), fp32 restatement %.3e = %.2f x dev_w %.3e (bar %.0f x)' % (
        name, e64, 1e-10 * top, e32, e32 / dev, dev, BAR))
    assert tuple(t64['w'].shape) == tuple(want.shape) == (R.CASES[name][0], enc.style_count, 512)
    assert e64 <= 1e-10 * top and e32 <= BAR * dev
    side = R.CASES[name][1]
    assert [tuple(t64[k].shape[1:]) for k in ('stem', 'u0', 'u3', 'c1', 'c2', 'c3', 'p2', 'p1')] == [
        (64, side, side), (64, side // 2, side // 2), (128, side // 4, side // 4), (128, side // 4, side // 4), (256, side // 8, side // 8),
        (512, side // 16, side // 16), (512, side // 8, side // 8), (512, side // 4, side // 4)]
    assert all(('dev_%s_%s' % (k, name)) in kat.files for k in R.TAPS)


def test_fixture_holds_case_c_as_one_scalar(kat):
    assert 'dev_w_c' in kat.files and float(kat['dev_w_c']) > 0
    assert not [k for k in kat.files if k.endswith('_c') and k not in ('dev_w_c', 'max_w_c')]
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', R.KAT)) < 1 << 20


def test_c_abi_declares_the_e4e_functions():
    from stylegan_directions_face_reenactment_amd import _native
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    declared = set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header))
    names = {'sgdfr_e4e_style_count', 'sgdfr_e4e_param_count', 'sgdfr_e4e_pack_elems', 'sgdfr_e4e_debug_elems',
             'sgdfr_e4e_workspace_bytes', 'sgdfr_e4e_prepack_f32', 'sgdfr_e4e_forward_f32'}
    assert names <= declared
    assert {'sgdfr_e4e_prepack_f32', 'sgdfr_e4e_forward_f32'} <= set(_native.SIGNATURES)
    lib = _native.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.sgdfr_abi_version() == _native.ABI_VERSION == 23
    # sizes out of range are refused by every entry point, before any launch
    for bad in (16, 40, 272, 512):
        assert lib.sgdfr_e4e_style_count(bad) == -1 and lib.sgdfr_e4e_pack_elems(bad) == -1
        assert lib.sgdfr_e4e_workspace_bytes(1, bad) == -1
        assert lib.sgdfr_e4e_forward_f32(None, 1, bad, None, None, None, None, 0, None) != 0
        assert b'resolution' in lib.sgdfr_last_error()
    assert lib.sgdfr_e4e_workspace_bytes(0, 64) == -1 and lib.sgdfr_e4e_workspace_bytes(257, 64) == -1
    assert lib.sgdfr_e4e_forward_f32(None, 0, 64, None, None, None, None, 0, None) != 0 and b'rows' in lib.sgdfr_last_error()
    assert lib.sgdfr_e4e_prepack_f32(None, 64, None, None) != 0 and b'null' in lib.sgdfr_last_error()
    assert [lib.sgdfr_e4e_style_count(r) for r in (32, 64, 96, 128, 256)] == [8, 10, 10, 12, 14]


def test_parameter_count_matches_the_documented_layout(small):
    """3 for the stem, 10 per unit, 4 for the lateral convs, per head two per conv (4 / 5 / 6 convs by group) and two for its
    EqualLinear; the shortcut pair is None exactly for the 21 units whose input width equals their depth."""
    from stylegan_directions_face_reenactment_amd import _native, encoder as E
    lib = _native.load()
    for res, heads in ((64, 10), (256, 14)):
        convs = sum(4 if j < 3 else 5 if j < 7 else 6 for j in range(heads))
        assert lib.sgdfr_e4e_param_count(res) == 3 + 10 * 24 + 4 + 2 * convs + 2 * heads
    assert lib.sgdfr_e4e_param_count(256) == _native.E4E_PARAMS_256 == 423
    enc, _ = small
    ps = E.folded(enc)
    assert len(ps) == lib.sgdfr_e4e_param_count(64)
    assert sum(p is None for p in ps) == 2 * 21 and all(p is None or p.dtype == torch.float32 for p in ps)
    assert tuple(ps[0].shape) == (64, 3, 3, 3) and tuple(ps[3 + 10 * 3 + 8].shape) == (128, 64) and tuple(ps[-2].shape) == (512, 512)
    total = sum(p.numel() for p in ps if p is not None)
    assert total <= lib.sgdfr_e4e_pack_elems(64) <= total + 64 * len(ps)        # the pack: the same values, 64-float aligned


def test_encode_refuses_cpu_tensors_train_mode_wrong_sizes_and_other_trunks(small):
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _ = small
    with pytest.raises(RuntimeError, match='no CPU path'):
        E.encode(enc, torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match='built for 64x64'):
        E.encode(enc, torch.zeros(1, 3, 64, 96))
    with pytest.raises(ValueError, match='built for 64x64'):
        E.encode(enc, torch.zeros(1, 3, 128, 128))
    with pytest.raises(ValueError, match=r'\[B,3,64,64\]'):
        E.encode(enc, torch.zeros(3, 64, 64))
    enc.train()
    try:
        with pytest.raises(RuntimeError, match=r'train\(\) mode'):
            E.encode(enc, torch.zeros(1, 3, 64, 64))
    finally:
        enc.eval()
    with pytest.raises(ValueError, match="'ir_se'"):
        E.encode(E.Encoder4Editing(50, 'ir', 64).eval(), torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match='multiple of 16'):
        E.encode(E.Encoder4Editing(50, 'ir_se', 512).eval(), torch.zeros(1, 3, 512, 512))


def test_pack_stays_out_of_the_state_dict_copies_and_pickles(small):
    enc, state = small
    enc._pack = ('key', torch.zeros(1), [])
    try:
        assert set(enc.state_dict().keys()) == set(state.keys())
        assert copy.deepcopy(enc)._pack is None
        assert pickle.loads(pickle.dumps(enc))._pack is None
        enc.invalidate_packs()
        assert enc._pack is None
        enc._pack = ('key', torch.zeros(1), [])
        enc.load_state_dict(state, strict=True)
        assert enc._pack is None
        enc._pack = ('key', torch.zeros(1), [])
        enc.float()
        assert enc._pack is None
    finally:
        enc._pack = None


# ---------------------------------------------------------------------------------------------------------------- the plan rules
def test_plan_rule_geometry_matches_the_c_abi():
    """tests/plan_rules.py restates the geometry csrc/e4e.hip plans from: the head count at every resolution the ABI admits, the
    live taps of the head convs, and the launch total the GPU tests assert."""
    import plan_rules as P
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    for res in range(32, 257, 16):
        assert P.e4e_style_count(res) == lib.sgdfr_e4e_style_count(res), res
        groups = P.e4e_groups(res)
        assert [hi - lo for lo, hi, _, _ in groups] == [3, 4, P.e4e_style_count(res) - 7]
        for lo, hi, depth, side in groups:                  # every head ends at 1 x 1 after its 4 / 5 / 6 convs
            for _ in range(depth):
                side = (side - 1) // 2 + 1
            assert side == 1, res
    assert all(res in R.SWEEP for res, _ in P.E4E_SMALL + P.E4E_LARGE)
    assert [R.case(R.SWEEP[res])[:2] for res, _ in P.E4E_SMALL] == [(B, res) for res, B in P.E4E_SMALL]
    # one tap of a 1 x 1 map, four of 2 x 2, all nine from 3 x 3 on (an odd map reaches its last row through tap 0 of the next output)
    assert [len(P.live_taps(s)) for s in (1, 2, 3, 4, 5, 7, 8)] == [1, 4, 9, 9, 9, 9, 9]
    assert P.live_taps(1) == [4] and P.live_taps(2) == [4, 5, 7, 8]
    # R = 80: 5 -> 3 -> 2 -> 1 -> 1; R = 112: 7 -> 4 -> 2 -> 1 -> 1 (K = 512 x taps of the input map)
    assert [l.K // 512 for l in P.e4e_launches(80) if l.name.startswith('g0.')] == [9, 9, 4, 1]
    assert [l.K // 512 for l in P.e4e_launches(112) if l.name.startswith('g0.')] == [9, 9, 4, 1]
    assert [l.K // 512 for l in P.e4e_launches(64) if l.name.startswith('g0.')] == [9, 4, 1, 1]
    for res in range(32, 257, 16):
        assert len(P.e4e_launches(res)) == 1 + 48 + 3 + 2 + 15 + 1 == 70
    assert P.e4e_counts(3, 64)[0] == 70
    # what the existing GPU test observes at R = 64: fewer sliced convs as the batch grows, one fewer at B = 3 (unit 0's conv1)
    f = [P.e4e_counts(B, 64)[1] for B in (1, 2, 3)]
    assert f[0] >= f[1] >= f[2] > 0 and f[0] > f[2], f


def test_sweep_cases_cover_every_launch_class_sliced_and_whole():
    """The coverage condition: over the GPU cases of test_gpu_s3fd_e4e_plans every launch class of csrc/e4e.hip runs at least once
    sliced over K (epilogue in e4e_finish_kernel) and at least once whole (epilogue in e4e_conv_kernel).  The exceptions are named
    in plan_rules.E4E_EXCEPTIONS and proven here over every size the ABI admits."""
    import plan_rules as P
    cases = P.E4E_SMALL + P.E4E_LARGE
    assert all(1 <= B <= P.E4E_MAX_ROWS and B * res * res <= 1 << 24 for res, B in cases)
    seen = P.coverage([P.e4e_plan(B, res) for res, B in cases], P.E4E_CLASSES)
    want = {(c, how) for c in P.E4E_CLASSES for how in ('sliced', 'whole')}
    for res, B in cases:
        plan = P.e4e_plan(B, res)
        sliced, whole = [l.name for l, S in plan if S > 1], [l.name for l, S in plan if S == 1]
        print('R = %3d B = %3d: %d convs, %d sliced; %s' % (res, B, len(plan), len(sliced), 'whole: ' + ' '.join(whole)
                                                            if len(whole) <= len(sliced) else 'sliced: ' + ' '.join(sliced)))
    print('exceptions: %s' % '; '.join('%s never %s (%s)' % (c, how, why) for (c, how), why in P.E4E_EXCEPTIONS.items()))
    assert want - seen == set(P.E4E_EXCEPTIONS), sorted(want - seen)
    assert list(P.E4E_EXCEPTIONS) == [('stem', 'sliced')]
    reach = P.coverage([P.e4e_plan(B, res) for res in range(32, 257, 16) for B in range(1, P.E4E_MAX_ROWS + 1) if B * res * res <= 1 << 24],
                       P.E4E_CLASSES)
    assert not (set(P.E4E_EXCEPTIONS) & reach)              # no admitted size reaches an exception ...
    assert reach == seen                                    # ... and the cases reach everything an admitted size can
    # the paths the small fixtures never ran, by name: unit 21's SE-gated shortcut and the grouped launches run whole
    whole = {(res, B): {l.name for l, S in P.e4e_plan(B, res) if S == 1} for res, B in cases}
    assert 'u21.shortcut' not in whole[(64, 3)] and 'u21.shortcut' in whole[(64, 96)]
    assert 'linear' not in whole[(64, 96)] and 'linear' in whole[(64, 192)]
    assert {'g1.k1', 'g2.k1'} <= whole[(64, 96)] and 'g2.k1' in whole[(48, 192)] and {'g0.k3', 'g1.k4'} & whole[(256, 194)] == set()
    assert 'g2.k5' in whole[(256, 194)]

"""CPU: the direction sweeps' ladder arithmetic and host contract (csrc/sweep.hip, sweep.py) -- no GPU needed.

The fixture tests/golden/kat20_sweeps.npz holds what the REAL get_direction_info + np.arange + one_hot chain gives on CPU tensors
(scripts/make_golden_sweep.py).  Bars: bit for bit -- the restatement (tests/sweep_restatement.py) and the library's host entries
sgdfr_sweep_plan_host / sgdfr_sweep_rows_host, which run the very function the device kernels run."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import sweep_restatement as R
from util import ROOT, golden

SETTINGS = (('voxceleb', 15, 6), ('ffhq', 12, 6.0), ('voxceleb', 15, 4.5))
COUNTS = (10, 4)
BASE_ROWS = 8


def tag_of(dataset, D, sc):
    return '%s_%d_%s' % (dataset, D, str(sc).replace('.', 'p'))


def builder(dataset, D, sc):
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    return ShiftVectors(dataset, D, sc, ranges=golden('kat8_shift.npz')['ranges_' + dataset])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_values(a, b):
    """equal with +0 == -0 (float arrays of the same dtype and shape, no NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())


def test_fixture_covers_what_it_claims():
    g = golden('kat20_sweeps.npz')
    assert any(v.startswith('numpy 2') or int(v.split()[1].split('.')[0]) >= 2 for v in g['versions'] if v.startswith('numpy'))
    for dataset, D, sc in SETTINGS:
        tag = tag_of(dataset, D, sc)
        kinds, types = g[tag + '.kinds'], list(g[tag + '.types'])
        assert set(kinds.tolist()) == {1, 2, 3} and len(types) == D
        assert types[:2] == ['yaw', 'pitch'] and 'jaw' in types and (('roll' in types) == (dataset == 'voxceleb'))
        N = g[tag + '.ang'].shape[0]
        assert N in (BASE_ROWS + 4, BASE_ROWS + 5) and (N == BASE_ROWS + 5) == bool(g[tag + '.near_integer'][:, 0].any())
        ang_k = np.nonzero(kinds == 1)[0]
        for c in COUNTS:
            key = '%s.c%d' % (tag, c)
            n_lo, n_hi, start = g[key + '.n_lo'], g[key + '.n_hi'], g[key + '.start']
            assert n_lo.dtype == n_hi.dtype == np.int32 and start.dtype == np.float64 and g[key + '.rows'].dtype == np.float32
            assert (n_lo == 0).any() and (n_hi == 0).any() and ((n_lo > 0) & (n_hi > 0)).any()
            assert list(g[key + '.start_dtype']) == ['float64' if k == 1 else 'float32' for k in kinds]
            # the zero-angle row: start exactly 0, shifts_count + (shifts_count + 1) rows -- the +1e-5 endpoint is in
            assert (start[BASE_ROWS, ang_k] == 0).all() and (n_lo[BASE_ROWS, ang_k] == c).all() and (n_hi[BASE_ROWS, ang_k] == c + 1).all()
            assert (start[BASE_ROWS + 1, ang_k] > sc / 2).all() and (n_hi[BASE_ROWS + 1, ang_k] == 0).all()
            assert (start[BASE_ROWS + 2, ang_k] < -sc / 2).all() and (n_lo[BASE_ROWS + 2, ang_k] == 0).all()
            assert (start[BASE_ROWS + 3, kinds != 1] > sc).all() and (n_hi[BASE_ROWS + 3, kinds != 1] == 0).all()
            rows = g[key + '.rows']
            assert rows.shape == (int(n_lo.sum() + n_hi.sum()), D) and ((rows != 0).sum(1) <= 1).all()
            assert g[key + '.step'] == sc / c


def test_restatement_equals_the_fixture_bit_for_bit():
    g = golden('kat20_sweeps.npz')
    for dataset, D, sc in SETTINGS:
        tag = tag_of(dataset, D, sc)
        table = R.table_of(builder(dataset, D, sc))
        assert [t[0] for t in table] == g[tag + '.kinds'].tolist()
        for c in COUNTS:
            key = '%s.c%d' % (tag, c)
            rec, step, n_lo, n_hi, rows, row_k, is_start = R.plan_rows(table, g[tag + '.ang'], g[tag + '.pose'], g[tag + '.exp'], sc, c)
            for f in ('start', 'min', 'max'):
                assert same_bits(rec[f], g[key + '.' + f]), (key, f)
            assert step == g[key + '.step'] and same_bits(n_lo, g[key + '.n_lo']) and same_bits(n_hi, g[key + '.n_hi'])
            assert same_bits(rows, g[key + '.rows']), key
            assert int(is_start.sum()) == int((n_hi > 0).sum())


def host_plan(sv, ang, pose, exp, dirs, sc, c):
    from stylegan_directions_face_reenactment_amd import _native as N
    from stylegan_directions_face_reenactment_amd.sweep import RECORD
    ang, pose, exp = (np.ascontiguousarray(a, dtype=np.float32) for a in (ang, pose, exp))
    n, K = ang.shape[0], len(dirs)
    arr = (ctypes.c_int * K)(*dirs)
    rec = np.zeros(n * K, dtype=RECORD)
    N.call('sgdfr_sweep_plan_host', ang.ctypes.data, pose.ctypes.data, exp.ctypes.data, pose.shape[1], exp.shape[1], sv._table_train,
           sv.learned_directions, arr, K, float(sc), c, rec.ctypes.data, n)
    return rec, arr


def test_host_entry_equals_the_fixture_bit_for_bit():
    """sgdfr_sweep_plan_host / sgdfr_sweep_rows_host run the function the device kernels run: records, lengths and rows of every setting."""
    from stylegan_directions_face_reenactment_amd import _native as N
    g = golden('kat20_sweeps.npz')
    for dataset, D, sc in SETTINGS:
        tag = tag_of(dataset, D, sc)
        sv = builder(dataset, D, sc)
        for c in COUNTS:
            key = '%s.c%d' % (tag, c)
            rec, arr = host_plan(sv, g[tag + '.ang'], g[tag + '.pose'], g[tag + '.exp'], list(range(D)), sc, c)
            r = rec.reshape(-1, D)
            for f, name in (('start', 'start'), ('min_shift', 'min'), ('max_shift', 'max')):
                assert same_bits(np.ascontiguousarray(r[f]), g[key + '.' + name]), (key, f)
            assert (r['step'] == g[key + '.step']).all()
            assert same_bits(np.ascontiguousarray(r['n_lo']), g[key + '.n_lo']) and same_bits(np.ascontiguousarray(r['n_hi']), g[key + '.n_hi'])
            total = int(r['n_lo'].sum() + r['n_hi'].sum())
            rows = np.full((total, D), 7.0, dtype=np.float32)
            row_k, is_start = np.full(total, -7, dtype=np.int32), np.full(total, -7, dtype=np.int32)
            N.call('sgdfr_sweep_rows_host', rec.ctypes.data, sv._table_train, D, arr, D, r.shape[0], rows.ctypes.data, row_k.ctypes.data,
                   is_start.ctypes.data, total)
            assert same_values(rows, g[key + '.rows']), key
            _, _, _, _, _, want_k, want_start = R.plan_rows(R.table_of(sv), g[tag + '.ang'], g[tag + '.pose'], g[tag + '.exp'], sc, c)
            assert (row_k == want_k).all() and (is_start == want_start).all()


def test_host_entry_on_a_subset_of_directions_in_another_order():
    g = golden('kat20_sweeps.npz')
    dataset, D, sc = SETTINGS[0]
    tag, sv = tag_of(dataset, D, sc), builder(dataset, D, sc)
    dirs = [9, 0, 3]
    rec, _ = host_plan(sv, g[tag + '.ang'], g[tag + '.pose'], g[tag + '.exp'], dirs, sc, 10)
    r = rec.reshape(-1, 3)
    for j, k in enumerate(dirs):
        assert (r['start'][:, j] == g[tag + '.c10.start'][:, k]).all() and (r['n_lo'][:, j] == g[tag + '.c10.n_lo'][:, k]).all()
        assert (r['n_hi'][:, j] == g[tag + '.c10.n_hi'][:, k]).all()


def test_native_entries_refuse_bad_arguments_before_any_launch():
    from stylegan_directions_face_reenactment_amd import _native as N
    lib = N.load()
    fake = ctypes.c_void_p(64)                                           # never dereferenced: every case is refused first
    rc = lib.sgdfr_sweep_frames_f32(fake, 1, 8, 3, None, None, 0, fake, None, None, 1, None)
    assert rc != 0 and b'1, 2 or 4' in lib.sgdfr_last_error()
    rc = lib.sgdfr_sweep_frames_f32(fake, 1, 6, 1, fake, None, 0, None, fake, None, 1, None)
    assert rc != 0 and b'border' in lib.sgdfr_last_error()
    rc = lib.sgdfr_sweep_frames_f32(fake, 1, 8, 1, None, None, 0, None, None, fake, 2, None)
    assert rc != 0 and b'source' in lib.sgdfr_last_error()
    # a direction the table marks absent (SGDFR_DIR_ZERO): the reference dies with UnboundLocalError there
    table = (N.Direction * 4)()
    for k in range(4):
        table[k].kind, table[k].col, table[k].a, table[k].b = N.DIR_ANGLE, 0, 6.0, 40.0
    table[2].kind = N.DIR_ZERO
    dirs = (ctypes.c_int * 2)(0, 2)
    for name, extra in (('sgdfr_sweep_plan_f32', (None,)), ('sgdfr_sweep_plan_host', ())):
        rc = getattr(lib, name)(fake, fake, fake, 6, 50, table, 4, dirs, 2, 6.0, 10, fake, 1, *extra)
        assert rc != 0 and b'direction 2 is absent' in lib.sgdfr_last_error(), name
    dirs = (ctypes.c_int * 1)(4)
    assert lib.sgdfr_sweep_plan_host(fake, fake, fake, 6, 50, table, 4, dirs, 1, 6.0, 10, fake, 1) != 0 and b'outside' in lib.sgdfr_last_error()
    dirs = (ctypes.c_int * 1)(0)
    assert lib.sgdfr_sweep_plan_host(fake, fake, fake, 6, 50, table, 4, dirs, 1, 6.0, 0, fake, 1) != 0 and b'shifts_count' in lib.sgdfr_last_error()


def test_python_entries_refuse_cpu_tensors_and_bad_shapes():
    from stylegan_directions_face_reenactment_amd import sweep as SW
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.model import Generator
    with pytest.raises(RuntimeError, match='no CPU path'):
        SW.pool_frames(torch.zeros(1, 3, 8, 8))
    G = Generator(32, 512, 8, channel_multiplier=1)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    sv = builder('voxceleb', 15, 6)
    sw = SW.DirectionSweep(G, A, sv, truncation=1.0)
    assert sw.types_all == ['yaw', 'pitch', 'roll', 'jaw'] + ['exp_%02d' % i for i in range(11)]
    with pytest.raises(RuntimeError, match='no CPU path'):
        sw.plan({'pose': torch.zeros(1, 6), 'alpha_exp': torch.zeros(1, 50)}, torch.zeros(1, 3), [0, 1])
    with pytest.raises(RuntimeError, match='truncation'):
        SW.DirectionSweep(G, A, sv)
    with pytest.raises(RuntimeError, match='DirectionMatrix'):
        SW.DirectionSweep(G, A, sv, truncation=1.0, w_plus=False)
    with pytest.raises(RuntimeError, match='directions'):
        SW.DirectionSweep(G, A, builder('ffhq', 12, 6.0), truncation=1.0)
    # the table built from get_direction_info's own arguments is the trainer's table
    mine = SW.direction_table(15, 6, sv.angle_scales, sv.angle_directions, sv.count_pose, sv.a_jaw, sv.b_jaw, sv.directions_exp)
    for k in range(15):
        assert (mine[k].kind, mine[k].col, mine[k].a, mine[k].b) == tuple(getattr(sv._table_train[k], f) for f in ('kind', 'col', 'a', 'b'))
    ff = builder('ffhq', 12, 6.0)
    assert SW.direction_types(ff._table_train, 12) == ['yaw', 'pitch', 'jaw'] + ['exp_%02d' % i for i in range(9)]


def test_symbols_are_declared_exported_and_abi_is_23():
    from stylegan_directions_face_reenactment_amd import _native as N
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    declared = set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header))
    lib = N.load()
    for name in ('sgdfr_sweep_plan_f32', 'sgdfr_sweep_plan_host', 'sgdfr_sweep_rows_f32', 'sgdfr_sweep_rows_host', 'sgdfr_sweep_frames_f32'):
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert N.ABI_VERSION == 23 and lib.sgdfr_abi_version() == 23
    assert 'struct sgdfr_sweep_record' in header and ctypes.sizeof(N.SweepRecord) == 40


def test_install_visualization_mounts_and_unmounts():
    from stylegan_directions_face_reenactment_amd import compat, sweep as SW
    before = {k: sys.modules.get(k) for k in list(sys.modules) if k == 'libs' or k.startswith('libs.')}
    names = set(sys.modules)
    assert compat.VISUALIZATION_ALIAS not in compat.ALIASES                 # install() stays as it was
    try:
        assert compat.install_visualization() == 'libs.utilities.visualization'
        from libs.utilities.visualization import make_interpolation_chart, get_shifted_image    # noqa: F401
        assert make_interpolation_chart is SW.make_interpolation_chart
    finally:
        assert compat.uninstall_visualization()
    assert set(sys.modules) - names == set() and all(sys.modules.get(k) is v for k, v in before.items())
    assert not compat.uninstall_visualization()


def test_frame_restatement_under_image_tolerance_noise():
    """Two renderings IMG_TOL = 2e-4 apart give uint8 frames at most one count apart.  How many bytes differ: a boundary is crossed
    with probability 127.5 * |delta| per byte, 2.55 % at |delta| = IMG_TOL everywhere and half of that, ~1.3 %, for deltas uniform in
    +-IMG_TOL (measured here: 1.38 %) -- so the GPU test's 1 % cap asks the batched frames to agree with the loop's to better than
    ~1.5e-4 on average, which batches of one arithmetic do by orders of magnitude."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.0, 1.0, (4, 3, 64, 64)).astype(np.float32)
    for amp, cap in ((2e-4, 0.0255), (2e-5, 0.01)):
        y = (x + rng.uniform(-amp, amp, x.shape)).astype(np.float32)
        a, b = R.frame_u8(x), R.frame_u8(y)
        d = np.abs(a.astype(np.int16) - b.astype(np.int16))
        assert d.max() <= 1
        share = float((d != 0).mean())
        print('noise +-%g: %.3f %% of the bytes differ' % (amp, 100 * share))
        assert share <= cap
    # the pieces the GPU test leans on
    p = R.pool64(x, 4)
    assert p.shape == (4, 3, 16, 16) and np.allclose(p, torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(x).double(), (16, 16)).numpy())
    bd = R.border64(p, [0, 1, 0, 0])
    m = R.border_mask(16)
    assert (bd[1, 0][m] == 1).all() and (bd[1, 1:][:, m] == -1).all() and (bd[1][:, ~m] == p[1][:, ~m]).all() and (bd[0] == p[0]).all()
    assert R.frames_u8(x[:, :, :16, :16], x[:1, :, :16, :16]).shape == (4, 16, 32, 3)

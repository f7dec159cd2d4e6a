"""GPU: direction sweeps (csrc/sweep.hip through sweep.py) against the fixture captured from the real get_direction_info + np.arange +
one_hot chain (tests/golden/kat20_sweeps.npz), the float64 restatements of tests/sweep_restatement.py and the written-out B=1 loop.

Bars: ladder records, lengths and one-hot rows BIT-exact; the pooled mean within the sequential-sum bound
(f^2 - 1) * 2^-24 * max|x| + 2^-24 * max|x| of the float64 mean; border and uint8 frames exact functions of the kernel's own pooled
values; sweep images equal to ReenactmentSession.render of the same rows bit for bit and within IMG_TOL of the B=1 loop."""
import itertools

import numpy as np
import pytest
import torch

import sweep_restatement as R
from test_cpu_sweeps import COUNTS, SETTINGS, builder, same_bits, same_values, tag_of
from util import S, SEED, golden, hip_generator, maxabs

pytestmark = pytest.mark.gpu

IMG_TOL = 2e-4          # the bar of tests/test_gpu_generator.py
U = 2.0 ** -24


def direction_matrix(D=15):
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    A = DirectionMatrix(512, input_dim=D, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(5, input_dim=D))
    return A.cuda()


def source_params(g, tag, rows):
    ang = torch.from_numpy(g[tag + '.ang'][rows]).cuda()
    return {'pose': torch.from_numpy(g[tag + '.pose'][rows]).cuda(), 'alpha_exp': torch.from_numpy(g[tag + '.exp'][rows]).cuda()}, ang


# ------------------------------------------------------------------ plan and rows
@pytest.mark.parametrize('dataset,D,sc', SETTINGS)
def test_plan_and_rows_equal_the_fixture_bit_for_bit(dataset, D, sc):
    from stylegan_directions_face_reenactment_amd.sweep import DirectionSweep
    g = golden('kat20_sweeps.npz')
    tag = tag_of(dataset, D, sc)
    sv = builder(dataset, D, sc)
    sw = DirectionSweep(None, direction_matrix(D), sv, truncation=1.0)
    assert sw.types_all == list(g[tag + '.types'])
    n = g[tag + '.ang'].shape[0]
    params, ang = source_params(g, tag, slice(0, n))
    for c in COUNTS:
        key = '%s.c%d' % (tag, c)
        rec = sw.plan(params, ang, range(D), c)
        assert rec.is_cuda and rec.shape == (n, D, 5)
        host = sw.records_to_host(rec)
        for f, name in (('start', 'start'), ('min_shift', 'min'), ('max_shift', 'max')):
            assert same_bits(np.ascontiguousarray(host[f]), g[key + '.' + name]), (key, f)
        assert (host['step'] == g[key + '.step']).all()
        assert same_bits(np.ascontiguousarray(host['n_lo']), g[key + '.n_lo']) and same_bits(np.ascontiguousarray(host['n_hi']), g[key + '.n_hi'])
        total = int(host['n_lo'].sum() + host['n_hi'].sum())
        rows, row_k, is_start = sw.rows(rec, range(D), total)
        assert same_values(rows.cpu().numpy(), g[key + '.rows']), key               # +0 / -0 compare equal
        _, _, _, _, _, want_k, want_start = R.plan_rows(R.table_of(sv), g[tag + '.ang'], g[tag + '.pose'], g[tag + '.exp'], sc, c)
        assert (row_k.cpu().numpy() == want_k).all() and (is_start.cpu().numpy() == want_start).all()


# ------------------------------------------------------------------ frames kernel
def frames_input(R_, S_, key):
    x = S.counter_tensor(SEED, key, (R_, 3, S_, S_), 0.0, 0.9).clamp_(-1.5, 1.5)      # a sixth of the values beyond +-1: the clamp acts
    assert float(x.abs().max()) > 1.0
    return x


def check_frames_kernel(P, f, R_, flagged, key):
    from stylegan_directions_face_reenactment_amd.sweep import pool_frames
    x = frames_input(R_, P * f, key)
    src = frames_input(1, P, key + '.src')
    flags = torch.zeros(R_, dtype=torch.int32)
    flags[list(flagged)] = 1
    xc, sc_, fc = x.cuda(), src.cuda(), flags.cuda()
    full = pool_frames(xc, P, fc, sc_, ('images', 'bordered', 'frames'))
    pooled, bordered, frames2 = (full[k].cpu().numpy() for k in ('images', 'bordered', 'frames'))
    # pooled: the sequential-sum bound against the float64 mean
    bound = ((f * f - 1) * U + U) * float(x.abs().max())
    err = float(np.abs(pooled.astype(np.float64) - R.pool64(x.numpy(), f)).max())
    print('P=%d f=%d: max |pooled - mean64| = %.3e (bound %.3e)' % (P, f, err, bound))
    assert pooled.shape == (R_, 3, P, P) and err <= bound
    # bordered: add_border on the flagged rows only, applied to the kernel's own pooled values
    assert same_values(bordered, R.border64(pooled, flags.numpy()).astype(np.float32))
    m = R.border_mask(P)
    for r in range(R_):
        if r in flagged:
            assert (bordered[r, 0][m] == 1).all() and (bordered[r, 1:][:, m] == -1).all() and (bordered[r][:, ~m] == pooled[r][:, ~m]).all()
        else:
            assert (bordered[r] == pooled[r]).all()
    # frames: the reference scaling of the kernel's own pooled values, byte for byte, in both layouts; never bordered
    assert frames2.shape == (R_, P, 2 * P, 3) and (frames2 == R.frames_u8(pooled, src.numpy())).all()
    one = pool_frames(xc, P, None, None, ('frames',))['frames'].cpu().numpy()
    assert one.shape == (R_, P, P, 3) and (one == R.frames_u8(pooled)).all()
    per_row = pool_frames(xc, P, None, xc[:, :, :P, :P].contiguous(), ('frames',))['frames'].cpu().numpy()
    assert (per_row == R.frames_u8(pooled, x[:, :, :P, :P].numpy())).all()
    # every subset of the outputs leaves the others as they were
    for k in (1, 2):
        for want in itertools.combinations(('images', 'bordered', 'frames'), k):
            part = pool_frames(xc, P, fc, sc_, want)
            assert set(part) == set(want) and all(torch.equal(part[n], full[n]) for n in want), want
    # a view that is only 4-byte aligned takes the dword path: the same bits
    shifted = torch.empty(x.numel() + 1, device='cuda')[1:].view(x.shape).copy_(xc)
    assert shifted.data_ptr() % 16 != 0
    off = pool_frames(shifted, P, fc, sc_, ('images', 'bordered', 'frames'))
    assert all(torch.equal(off[n], full[n]) for n in full)
    return full


@pytest.mark.parametrize('P,f', [(8, 1), (8, 2), (8, 4), (10, 1)])
def test_frames_kernel_small(P, f):
    check_frames_kernel(P, f, 5, (1, 3), 'sweep.frames.%d.%d' % (P, f))


def test_frames_kernel_real_shape():
    check_frames_kernel(256, 4, 2, (1,), 'sweep.frames.real')


def test_frames_at_f1_equal_the_reenactment_converters():
    from stylegan_directions_face_reenactment_amd.reenact import grid_frames_uint8, images_to_uint8
    from stylegan_directions_face_reenactment_amd.sweep import pool_frames
    x, src = frames_input(5, 16, 'sweep.f1').cuda(), frames_input(1, 16, 'sweep.f1.src').cuda()
    assert torch.equal(pool_frames(x, 16, None, src, ('frames',))['frames'], grid_frames_uint8([src, x]))
    assert torch.equal(pool_frames(x, 16, None, None, ('frames',))['frames'], images_to_uint8(x))
    assert torch.equal(pool_frames(x, 16, None, None, ('images',))['images'], x)
    with pytest.raises(RuntimeError, match='1, 2 or 4'):
        pool_frames(frames_input(1, 24, 'sweep.f3').cuda(), 8)
    with pytest.raises(RuntimeError, match='border'):
        pool_frames(frames_input(1, 6, 'sweep.p6').cuda(), 6, torch.zeros(1, dtype=torch.int32).cuda(), None, ('bordered',))


# ------------------------------------------------------------------ the sweep
_SWEEP = {}


def sweep_setup():
    """One 32^2 generator, DirectionMatrix, W+ source and truncation latent for the sweep tests (built once)."""
    if not _SWEEP:
        G = hip_generator(32, 1)
        _SWEEP.update(G=G, A=direction_matrix(15), w=S.synthetic_latents(5, 1, n_latent=G.n_latent).cuda(),
                      trunc=S.counter_tensor(5, 'trunc', (1, 512)).cuda(), z=S.synthetic_z(5, 1).cuda())
    return _SWEEP


def test_sweep_equals_session_render_and_the_b1_loop():
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.reenact import ReenactmentSession
    from stylegan_directions_face_reenactment_amd.sweep import DirectionSweep
    g = golden('kat20_sweeps.npz')
    dataset, D, sc = SETTINGS[0]
    tag, key = tag_of(dataset, D, sc), tag_of(dataset, D, sc) + '.c10'
    s = sweep_setup()
    G, A, w, trunc = s['G'], s['A'], s['w'], s['trunc']
    dirs = [0, 3, 5]                                                    # yaw, jaw, an expression
    assert [int(g[tag + '.kinds'][k]) for k in dirs] == [1, 2, 3]
    params, ang = source_params(g, tag, slice(0, 1))
    sw = DirectionSweep(G, A, builder(dataset, D, sc), 0.7, trunc, True, 8, batch=8)
    res = sw.run(w, dirs, params, ang, input_is_latent=True, shifts_count=10, want=('images', 'bordered', 'frames'))
    # the fixture's rows of source 0 along these directions, in run order
    n_lo, n_hi = g[key + '.n_lo'], g[key + '.n_hi']
    lens = (n_lo + n_hi).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(lens.reshape(-1))])[:-1].reshape(lens.shape)
    want_rows = np.concatenate([g[key + '.rows'][first[0, k]:first[0, k] + lens[0, k]] for k in dirs])
    total = want_rows.shape[0]
    assert total > 3 * 8 and total % 8 != 0                              # several chunks and a ragged tail
    assert [sl.stop - sl.start for sl in res.slices] == [int(lens[0, k]) for k in dirs] and res.slices[-1].stop == total
    assert res.types == ['yaw', 'jaw', 'exp_01'] and list(res.n_lo) == [int(n_lo[0, k]) for k in dirs]
    assert (res.start == g[key + '.start'][0, dirs]).all() and (res.min_shift == g[key + '.min'][0, dirs]).all()
    assert (res.max_shift == g[key + '.max'][0, dirs]).all() and res.step == float(g[key + '.step'])
    assert same_values(res.rows.cpu().numpy(), want_rows)
    assert res.images.shape == (total, 3, 32, 32) and res.frames.shape == (total, 32, 32, 3)
    # == ReenactmentSession.render of the same rows, bit for bit
    sess = ReenactmentSession(G, A, w, 0.7, trunc, batch=8)
    assert torch.equal(res.images, sess.render(torch.from_numpy(want_rows).cuda()))
    # within IMG_TOL of the written-out reference loop: one B=1 generate_image per fixture row
    with torch.no_grad():                                                # run_facial_editing.py:145 get_shifted_image
        loop = torch.cat([generate_image(G, w, 0.7, trunc, True, 8, shift_code=A(torch.from_numpy(row).cuda().unsqueeze(0)), input_is_latent=True)
                          for row in want_rows])
    err = maxabs(res.images, loop)
    print('sweep vs B=1 loop: max |diff| = %.3e over %d rows' % (err, total))
    assert err <= IMG_TOL
    # the start frame of each direction carries the red box, the others and the gif frames do not
    start_rows = [sl.start + int(n_lo[0, k]) for sl, k in zip(res.slices, dirs)]
    assert res.is_start.cpu().nonzero().flatten().tolist() == start_rows
    assert same_values(res.bordered.cpu().numpy(), R.border64(res.images.cpu().numpy(), res.is_start.cpu().numpy()).astype(np.float32))
    assert (res.frames.cpu().numpy() == R.frames_u8(res.images.cpu().numpy())).all()
    # a z source goes through the mapping network once; a W source is broadcast
    z = s['z']
    via_z = sw.run(z, [0], params, ang, input_is_latent=False, want=('images',))
    via_w = sw.run(G.get_latent(z), [0], params, ang, input_is_latent=True, want=('images',))
    assert torch.equal(via_z.images, via_w.images) and via_z.images.shape[0] == int(lens[0, 0])


def test_sweep_empty_ladder_gives_an_empty_slice():
    from stylegan_directions_face_reenactment_amd.sweep import DirectionSweep
    g = golden('kat20_sweeps.npz')
    dataset, D, sc = SETTINGS[0]
    tag = tag_of(dataset, D, sc)
    s = sweep_setup()
    params, ang = source_params(g, tag, slice(0, 1))
    params['pose'][0, 3] = float('nan')                                  # nothing to walk along the jaw (np.arange itself raises on it)
    sw = DirectionSweep(s['G'], s['A'], builder(dataset, D, sc), 0.7, s['trunc'], True, 8, batch=8)
    res = sw.run(s['w'], [3, 0], params, ang, want=('images', 'frames'))
    assert res.slices[0] == slice(0, 0) and res.n_lo[0] == 0 and res.n_hi[0] == 0
    n0 = int(g[tag + '.c10.n_lo'][0, 0] + g[tag + '.c10.n_hi'][0, 0])
    assert res.slices[1] == slice(0, n0) and res.images.shape[0] == n0 and res.frames.shape[0] == n0
    # a half-empty ladder: row 10 has no `lo` part on the angle directions, its first row is the start frame
    params, ang = source_params(g, tag, slice(10, 11))
    res = sw.run(s['w'], [0], params, ang, want=('images',))
    assert res.n_lo[0] == 0 and res.n_hi[0] == int(g[tag + '.c10.n_hi'][10, 0]) and int(res.is_start[0]) == 1
    with pytest.raises(RuntimeError, match='outside'):
        sw.run(s['w'], [15], params, ang)


def test_make_interpolation_chart_structure_and_frames(monkeypatch):
    """Reference structure (grids: per direction a list of uint8 HWC arrays; types), frames within one count of the B=1 loop's
    tensor_to_image(...).astype(uint8), at most 1 % of the bytes different (printed)."""
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.sweep import make_interpolation_chart
    g = golden('kat20_sweeps.npz')
    dataset, D, sc = SETTINGS[0]
    tag = tag_of(dataset, D, sc)
    s = sweep_setup()
    G, A, z, trunc = s['G'], s['A'], s['z'], s['trunc']
    sv = builder(dataset, D, sc)
    params, ang = source_params(g, tag, slice(0, 1))
    monkeypatch.setattr(G, 'mean_latent', lambda n: trunc.clone())
    seen = []

    def shape_model(images):
        seen.append(tuple(images.shape))
        return params, ang

    info = {'input_is_latent': False, 'learned_dims': D, 'count_pose': sv.count_pose, 'a_jaw': sv.a_jaw, 'b_jaw': sv.b_jaw, 'shift_scale': sc,
            'shifts_count': 4, 'w_plus': True, 'num_layers_shift': 8}
    grids, types = make_interpolation_chart(G, A, shape_model, z, sv.directions_exp, sv.angle_scales, sv.angle_directions, info,
                                            max_directions=4)
    assert seen == [(1, 3, 32, 32)] and types == ['yaw', 'pitch', 'roll', 'jaw'] and len(grids) == 4
    key = tag + '.c4'
    assert [len(gr) for gr in grids] == [int(g[key + '.n_lo'][0, k] + g[key + '.n_hi'][0, k]) for k in range(4)]
    assert all(isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.shape == (32, 32, 3) for gr in grids for f in gr)
    # the written-out loop of visualization.py:46-71 on the restated ladders
    table = R.table_of(sv)
    diff, count = 0, 0
    for k in range(4):
        kind, col, a, b = table[k]
        x = g[tag + '.ang'][0, col] if kind == R.ANGLE else g[tag + '.pose'][0, col]
        _, _, _, _, lo, hi = R.plan_ladder(kind, x, a, b, sc, 4)
        for j, shift in enumerate(list(lo) + list(hi)):
            vec = torch.zeros(D)
            vec[k] = shift
            with torch.no_grad():                                        # visualization.py:20
                img = generate_image(G, z, 0.7, trunc, True, 8, shift_code=A(vec.cuda()), input_is_latent=False)
            ref = R.frame_u8(img.cpu().numpy())[0]
            d = np.abs(ref.astype(np.int16) - grids[k][j].astype(np.int16))
            assert d.max() <= 1, (k, j)
            diff, count = diff + int((d != 0).sum()), count + d.size
    print('chart vs loop: %d of %d bytes differ (%.4f %%)' % (diff, count, 100.0 * diff / count))
    assert diff <= 0.01 * count


def test_extract_statistics_columns_ranges_and_used_rows():
    from stylegan_directions_face_reenactment_amd.sweep import extract_statistics
    s = sweep_setup()
    G, trunc = s['G'], s['trunc']
    n = 10
    ang, par = S.synthetic_shape_params(SEED, 'sweep.stats', n)
    ang, pose, exp = ang.clone(), par['pose'].clone(), par['alpha_exp'].clone()
    failed = [2, 7]
    for r in failed:                                                     # estimate_DECA.py:48-51: what a failed detection leaves
        ang[r], pose[r], exp[r] = -180.0, 0.0, 0.0
    calls = []

    def shape_fn(images):
        lo = sum(calls)
        calls.append(images.shape[0])
        assert images.shape[1:] == (3, 32, 32) and images.is_cuda
        sl = slice(lo, lo + images.shape[0])
        return {'pose': pose[sl].cuda(), 'alpha_exp': exp[sl].cuda()}, ang[sl].cuda()

    stats, ranges, used = extract_statistics(G, shape_fn, n, batch=4, truncation=0.7, trunc=trunc, z=S.synthetic_z(6, n).cuda())
    assert calls == [4, 4, 2] and stats.shape == (n, 54) and ranges.shape == (54, 2) and used.dtype == np.bool_
    assert stats.dtype == np.float64 and ranges.dtype == np.float64
    want = np.concatenate([ang.numpy(), pose.numpy()[:, 3:4], exp.numpy()], 1).astype(np.float64)      # yaw, pitch, roll, jaw, exp 0..49
    assert (stats == want).all()
    assert used.tolist() == [r not in failed for r in range(n)]
    assert (ranges[:, 0] == want[used].min(0)).all() and (ranges[:, 1] == want[used].max(0)).all()
    assert (ranges[:3, 0] > -180).all()                                  # the failed rows did not set the minima

"""GPU: the face detector on the HIP kernels of csrc/s3fd.hip against the fixture kat14 (written from the reference's own s3fd,
batch_detect, nms and detect_from_batch) and against the fp64 restatement on the CPU (tests/s3fd_restatement.py, itself pinned to
the fixture by test_cpu_s3fd).  Never against another run of the HIP code, except where two HIP runs must agree.

Bars: every debug tap and each of the twelve maps within 8 x the reference's own max |fp32 - fp64| on that tensor (dev_* of the
fixture: the same fp32 accumulation in another order); candidate and final boxes within 8 x the reference's own fp32 - fp64
deviation on its final boxes; candidate counts and order, kept indices and their order exactly equal (the fixture's script asserts
margins of 16 x dev on every score decision and 1e-3 on every IoU decision).  Every test prints the figures it asserts on.
"""
import copy

import numpy as np
import pytest
import torch

from util import S, golden
import s3fd_restatement as R
from test_cpu_s3fd import KAT, check_decisions

pytestmark = pytest.mark.gpu

BAR = 8.0
EPS32 = 2.0 ** -24


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def state(kat):
    return S.synthetic_s3fd_state(int(kat['seed']))


@pytest.fixture(scope='module')
def det(state):
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    m = FD.S3FD()
    m.load_state_dict(state, strict=True)
    return m.cuda()


@pytest.fixture(scope='module')
def ref64(kat, state):
    """Per case: images, subtract_mean and the fp64 taps of the restatement on the CPU."""
    out = {}
    for name in R.CASES:
        x, sub = R.fixture_inputs(S, int(kat['seed']), name)
        with torch.no_grad():
            out[name] = (x, sub, R.network(state, x.double(), sub))
    return out


def _check_image(kat, tag, r, b, bar, label):
    n, k = int(r['count'][b]), int(r['kept'][b])
    assert int(r['valid'][b]) == 1
    dets = r['cand'][b, :n].cpu().numpy()
    assert not r['cand'][b, n:].any()
    check_decisions(kat, tag, dets, None, None, r['index'][b, :k].cpu().tolist(), r['boxes'][b, :k].cpu().numpy(), bar, label)
    assert not r['boxes'][b, k:].any() and bool((r['index'][b, k:] == -1).all())
    scores = r['boxes'][b, :k, 4]
    assert bool((scores[:-1] > scores[1:]).all()) and bool((scores > 0.5).all())


@pytest.mark.parametrize('name', list(R.CASES))
def test_taps_maps_and_decisions_against_the_fixture(kat, det, ref64, name):
    """72 x 104 (cases a, m): M = 2*72*104 is no multiple of the 64-pixel tile, 9 x 13 pools to 4 x 6, fc6 makes 2 x 3 into 6 x 7, the
    last level is 2 x 2.  K runs from 27 (conv1_1) to 9216 (the fc7 head)."""
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    x, sub, taps64 = ref64[name]
    B, H, W, _ = R.CASES[name]
    r = FD.run_debug(det, x.cuda(), subtract_mean=sub)
    torch.cuda.synchronize()
    assert [tuple(m.shape[2:]) for m in r['maps'][::2]] == R.LEVEL_DIMS[(H, W)] == FD.level_dims(H, W)
    figures = []
    for k in R.TAPS:
        dev = float(kat['dev_%s_%s' % (k, name)])
        err = float((r['debug'][k].double().cpu() - taps64[k]).abs().max())
        figures.append((k, err, dev))
        print('case %s tap %-8s max |HIP - fp64| %.3e = %.2f x the reference fp32 deviation %.3e   bar %.0f x' % (name, k, err, err / dev, dev,
                                                                                                                 BAR))
    for i, m in enumerate(r['maps']):
        dev = float(kat['dev_map%d_%s' % (i, name)])
        err = float((m.double().cpu() - taps64['maps'][i]).abs().max())
        e_fix = float((m.double().cpu() - torch.from_numpy(kat['map%d_%s' % (i, name)])).abs().max())
        figures.append(('map%d' % i, max(err, e_fix), dev))
        print('case %s map %2d %-12s max |HIP - fp64| %.3e (fixture %.3e) = %.2f x the reference fp32 deviation %.3e   bar %.0f x' % (
            name, i, tuple(m.shape), err, e_fix, err / dev, dev, BAR))
    first = next(((k, err / dev) for k, err, dev in figures if err > BAR * dev), None)
    assert first is None, 'first tensor beyond the bar: %s at %.2f x' % first
    bar = BAR * float(kat['dev_boxes_' + name])
    for b in range(B):
        _check_image(kat, '%s_%d' % (name, b), r, b, bar, 'HIP')
    # the short path (0.5 in front of the NMS) and the reference-shaped lists give the same boxes
    boxes, kept, valid = FD.detect(det, x.cuda(), subtract_mean=sub)
    assert torch.equal(kept, r['kept']) and torch.equal(boxes, r['boxes']) and bool(valid.all())
    lists = FD.detect_from_batch(det, x.cuda(), subtract_mean=sub)
    assert [len(v) for v in lists] == kept.tolist()
    assert all(np.array_equal(np.stack(v), boxes[b, :len(v)].cpu().numpy()) for b, v in enumerate(lists))
    cand, count, _ = FD.candidates(det, x.cuda(), subtract_mean=sub)
    assert torch.equal(cand, r['cand']) and torch.equal(count, r['count'])


def _finish_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return sum('s3fd_conv_kernel' in n for n in names), sum('s3fd_finish_kernel' in n for n in names)


def test_rows_are_independent_across_batch_sizes_and_plans(kat, det, ref64):
    """B = 1, 2 and 3 from the rows of case a, permuted: per row the maps stay within the bar and the decisions equal the fixture's.
    The split-K plan follows the row count, so fewer convs are sliced over K as the batch grows."""
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    x, sub, taps64 = ref64['a']
    counts = {}
    for rows in ([1], [1, 0], [1, 0, 1]):
        B = len(rows)
        xb = x[rows].cuda()
        r = FD.run_debug(det, xb)
        worst = 0.0
        for i, m in enumerate(r['maps']):
            err = float((m.double().cpu() - taps64['maps'][i][rows]).abs().max())
            worst = max(worst, err / float(kat['dev_map%d_a' % i]))
        counts[B] = _finish_launches(lambda: FD.detect(det, xb))
        print('B = %d rows %s: worst map at %.2f x the reference fp32 deviation   bar %.0f x; %d convs, %d of them sliced over K' % (
            B, rows, worst, BAR, counts[B][0], counts[B][1]))
        assert worst <= BAR
        for b, row in enumerate(rows):
            _check_image(kat, 'a_%d' % row, r, b, BAR * float(kat['dev_boxes_a']), 'HIP B=%d' % B)
    assert all(c[0] == 25 for c in counts.values()), counts       # 19 trunk convs and six heads
    assert counts[1][1] >= counts[2][1] >= counts[3][1] > 0 and counts[1][1] > counts[3][1], counts


def _box_bar(want):
    """A decoded box is a handful of float32 operations on values up to its own size, with two exp calls accurate to 2 ulp."""
    return 16 * EPS32 * max(1.0, float(np.abs(want).max()))


def test_candidates_kernel_alone_on_handmade_heads():
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    heads = R.handmade_heads()
    maps = R.maps_of_heads(heads)
    cand, count, valid = FD.candidates_from_heads([h.cuda() for h in heads], threshold=0.05, capacity=32)
    assert count.tolist() == [15, 5] and valid.tolist() == [1, 1]
    for b in range(2):
        want = R.decode_image(maps, b)['dets']
        got = cand[b, :len(want)].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        print('hand-made image %d: %d candidates, max |HIP - restatement| %.3e   bar %.3e' % (b, len(want), err, _box_bar(want)))
        assert err <= _box_bar(want) and not cand[b, len(want):].any()
        # the maximum of the background channels decides, wherever it sits: the same score as with the three channels swapped round
    swapped = [heads[0][:, [2, 0, 1, 3, 4, 5, 6, 7]].contiguous()] + heads[1:]
    again, _, _ = FD.candidates_from_heads([h.cuda() for h in swapped], threshold=0.05, capacity=32)
    assert torch.equal(again, cand)
    # a list longer than the capacity: the true count, the first `capacity` rows, and the row marked
    short, count8, valid8 = FD.candidates_from_heads([h.cuda() for h in heads], threshold=0.05, capacity=8)
    assert count8.tolist() == [15, 5] and valid8.tolist() == [0, 1]
    assert torch.equal(short[0], cand[0, :8]) and torch.equal(short[1], cand[1, :8])
    # a higher threshold drops the weakest; nothing passes at all when every face logit is low
    _, count_high, _ = FD.candidates_from_heads([h.cuda() for h in heads], threshold=0.6, capacity=32)
    want_high = [int((R.decode_image(maps, b)['dets'][:, 4] > 0.6).sum()) for b in range(2)]
    assert count_high.tolist() == want_high == [13, 3]
    none = [torch.cat([torch.full_like(h[:, :-4], 3.0), h[:, -4:]], 1) for h in heads]
    for h in none:
        h[:, h.shape[1] - 5] = -3.0
    empty, count0, valid0 = FD.candidates_from_heads([h.cuda() for h in none], capacity=4)
    assert count0.tolist() == [0, 0] and valid0.tolist() == [1, 1] and not empty.any()
    boxes, index, kept = FD.nms(empty, count0)
    assert kept.tolist() == [0, 0] and not boxes.any() and bool((index == -1).all())


def test_nms_kernel_alone_on_handmade_lists():
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    # row 0: A; B overlaps A at IoU 47/153 = 0.307 (suppressed); C at 45/155 = 0.290 (kept, then suppresses nothing); a duplicate of A
    # (tie: the lower index wins); two boxes at or below 0.5 that overlap nothing; D far away with the top score; E tied with D, apart
    a = [0., 0, 99, 99]
    row0 = np.array([a + [0.9], [53., 0, 152, 99, 0.8], [0., 55, 99, 154, 0.7], a + [0.9], [300., 300, 310, 310, 0.5], [400., 0, 420, 30, 0.2],
                     [600., 600, 700, 700, 0.95], [800., 800, 900, 900, 0.95]], dtype=np.float32)
    row1 = np.array([[10., 10, 50, 50, 0.6], [12., 12, 52, 52, 0.99], [200., 10, 240, 50, 0.51]], dtype=np.float32)
    cap = 12
    cand = np.zeros((3, cap, 5), dtype=np.float32)
    cand[0, :len(row0)], cand[1, :len(row1)] = row0, row1
    cand[2] = np.array([5., 5, 25, 25, 0.75], dtype=np.float32) + np.arange(cap, dtype=np.float32)[:, None] * np.array([40., 0, 40, 0, 0.01],
                                                                                                                  dtype=np.float32)
    count = [len(row0), len(row1), cap + 5]                  # row 2: more were found than the list holds
    assert abs(float(R.iou_plus_one(row0[0], row0[1])) - 47 / 153) < 1e-6 and abs(float(R.iou_plus_one(row0[0], row0[2])) - 45 / 155) < 1e-6
    boxes, index, kept = FD.nms(torch.from_numpy(cand).cuda(), torch.tensor(count, dtype=torch.int32).cuda())
    for b in range(3):
        dets = cand[b, :min(count[b], cap)]
        want_idx, want = R.select(dets, floor=0.5)
        k = int(kept[b])
        print('hand-made row %d: %d candidates -> kept %s (restatement %s)' % (b, len(dets), index[b, :k].tolist(), want_idx))
        assert index[b, :k].tolist() == want_idx and np.array_equal(boxes[b, :k].cpu().numpy(), want)
        assert not boxes[b, k:].any() and bool((index[b, k:] == -1).all())
    assert index[0, :int(kept[0])].tolist() == [6, 7, 0, 2]
    assert index[1, :int(kept[1])].tolist() == [1, 2]


def test_two_runs_are_bitwise_equal(kat, det):
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    x, _ = R.fixture_inputs(S, int(kat['seed']), 'b')
    xc = x.cuda()
    one, two = FD.run_debug(det, xc), FD.run_debug(det, xc)
    for k in ('cand', 'count', 'valid', 'boxes', 'index', 'kept'):
        assert torch.equal(one[k], two[k]), k
    assert all(torch.equal(p, q) for p, q in zip(one['maps'], two['maps']))
    assert all(torch.equal(one['debug'][k], two['debug'][k]) for k in one['debug'])
    assert int(one['kept'].min()) >= 3


def test_detect_landmarks_end_to_end(kat, det):
    """detect -> select_face -> get_landmarks -> kpt68_boxes on one stream equals get_landmarks fed the fixture's first box."""
    from stylegan_directions_face_reenactment_amd import face_detector as FD, landmarks as L
    fan = L.FAN(4)
    fan.load_state_dict(S.synthetic_fan_state(20261208), strict=True)
    fan = fan.cuda().eval()
    x, _ = R.fixture_inputs(S, int(kat['seed']), 'b')
    xc = x.cuda()
    faces = torch.from_numpy(np.stack([kat['boxes_b_%d' % b][0] for b in range(2)])).float()
    pts_img, boxes, has = FD.detect_landmarks(det, fan, xc, rule='first')
    want_pts, _, _ = L.get_landmarks(fan, xc, faces.cuda())
    n = int((pts_img != want_pts).sum())
    print('detect_landmarks: %d of %d coordinates differ from get_landmarks fed the fixture boxes' % (n, pts_img.numel()))
    assert has.tolist() == [True, True] and n == 0
    assert torch.equal(boxes, L.kpt68_boxes(want_pts))
    # 'last_above_0.99': the mask says which rows hold such a face; those rows equal get_landmarks fed that box
    top = [kat['boxes_b_%d' % b] for b in range(2)]
    want_has = [bool((t[:, 4] > 0.99).any()) for t in top]
    pts99, _, has99 = FD.detect_landmarks(det, fan, xc, rule='last_above_0.99')
    assert has99.tolist() == want_has
    for b in range(2):
        if want_has[b]:
            f = torch.from_numpy(top[b][top[b][:, 4] > 0.99][-1]).float().view(1, 5)
            assert torch.equal(pts99[b:b + 1], L.get_landmarks(fan, xc[b:b + 1], f.cuda())[0])


def test_pack_is_rebuilt_after_an_in_place_edit_and_only_then(kat, det):
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    d = copy.deepcopy(det)
    assert d._pack is None
    x = R.images(S, 5, 's3fd.pack.image', 1, 40, 56).cuda()
    m0 = d(x)
    p0 = d.packed()
    assert d.packed() is p0
    d(x)
    assert d.packed() is p0                                  # no change, no rebuild
    with torch.no_grad():
        d.conv7_2_mbox_loc.bias.add_(1.0)                    # bumps the version counter
    m1 = d(x)
    assert d.packed() is not p0
    shift = (m1[11] - m0[11]).double()
    print('pack: reg6 moved by %.6f .. %.6f after conv7_2_mbox_loc.bias += 1' % (float(shift.min()), float(shift.max())))
    assert float((shift - 1.0).abs().max()) <= 1e-5 and all(torch.equal(m1[i], m0[i]) for i in range(11))
    p1 = d.packed()
    d.conv7_2_mbox_loc.bias.data.sub_(1.0)                   # through .data: no version bump, the pack is stale until invalidated
    assert d.packed() is p1
    d.invalidate_packs()
    m2 = d(x)
    assert d.packed() is not p1 and float((m2[11] - m0[11]).abs().max()) <= 1e-5

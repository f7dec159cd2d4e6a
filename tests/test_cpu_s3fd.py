"""CPU: the face detector without a GPU -- the restatement (tests/s3fd_restatement.py) against the fixture kat14 written from the
reference's own s3fd, batch_detect, nms and detect_from_batch (scripts/make_golden_s3fd.py), the two facts the device path rests on
(thresholding at 0.5 in front of the NMS changes nothing; the reference's mixed lists at B > 1 give the per-image result), the
module's key list, select_face, the refused arguments, the C ABI of csrc/s3fd.hip and compat.install_face_detector."""
import copy
import ctypes
import pickle
import sys

import numpy as np
import pytest
import torch

from util import S, golden
import s3fd_restatement as R

from stylegan_directions_face_reenactment_amd import _native as N, compat, face_detector as FD

KAT = 'kat14_s3fd.npz'
BAR = 8.0


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def state(kat):
    return S.synthetic_s3fd_state(int(kat['seed']))


@pytest.fixture(scope='module')
def ref64(kat, state):
    """Per case: images, subtract_mean and the fp64 restatement's taps on the CPU (shared with the GPU tests, never changed)."""
    out = {}
    for name in R.CASES:
        x, sub = R.fixture_inputs(S, int(kat['seed']), name)
        with torch.no_grad():
            out[name] = (x, sub, R.network(state, x.double(), sub))
    return out


def fixture_maps(kat, name):
    return [torch.from_numpy(kat['map%d_%s' % (i, name)]) for i in range(12)]


def check_decisions(kat, tag, dets, order, keep, kept, boxes, bar_boxes, label):
    """Shared with the GPU tests: one image's candidate list, sorted order, NMS survivors, those above 0.5 and final boxes against the
    fixture: the candidate boxes and final boxes within `bar_boxes`, every index list exactly.  Prints every figure."""
    want = kat['cand_' + tag]
    assert dets.shape == want.shape, '%s image %s: %d candidates, the reference has %d' % (label, tag, len(dets), len(want))
    e_cand = float(np.abs(np.asarray(dets, dtype=np.float64) - want).max())
    if order is not None:
        assert [int(i) for i in order] == kat['order_' + tag].tolist(), (label, tag, 'sorted order')
    if keep is not None:
        assert [int(i) for i in keep] == kat['keep_' + tag].tolist(), (label, tag, 'NMS survivors')
    assert [int(i) for i in kept] == kat['kept_' + tag].tolist(), (label, tag, 'kept indices')
    wb = kat['boxes_' + tag]
    assert boxes.shape == wb.shape
    e_box = float(np.abs(np.asarray(boxes, dtype=np.float64) - wb).max())
    print('%s image %s: %d candidates max |.| %.3e, %d final boxes max |.| %.3e   bar %.3e' % (label, tag, len(want), e_cand, len(wb), e_box,
                                                                                              bar_boxes))
    assert e_cand <= bar_boxes and e_box <= bar_boxes


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_matches_reference_fixture(kat, state, ref64, name):
    """fp64: maps and tap checksums to fp64 rounding (1e-9 of the tensor's scale), every decision exactly.  fp32: maps within 8 x the
    reference's own fp32 deviation, the same decisions."""
    x, sub, taps = ref64[name]
    B, H, W, _ = R.CASES[name]
    assert [tuple(m.shape[2:]) for m in taps['maps'][::2]] == R.LEVEL_DIMS[(H, W)]
    for i, m in enumerate(taps['maps']):
        want = torch.from_numpy(kat['map%d_%s' % (i, name)])
        err, bar = float((m - want).abs().max()), 1e-9 * max(1.0, float(want.abs().max()))
        print('fp64 case %s map %2d: %.3e   bar %.3e' % (name, i, err, bar))
        assert err <= bar
    for k in R.TAPS:
        want = kat['tap_%s_%s' % (k, name)]
        err, bar = float(np.abs(R.tap_checksum(taps[k]) - want).max()), 1e-9 * max(1.0, float(np.abs(want).max()))
        print('fp64 case %s tap %-8s: %.3e   bar %.3e' % (name, k, err, bar))
        assert err <= bar
    with torch.no_grad():
        taps32 = R.network(state, x, sub)
    for i, m in enumerate(taps32['maps']):
        err, dev = float((m.double() - torch.from_numpy(kat['map%d_%s' % (i, name)])).abs().max()), float(kat['dev_map%d_%s' % (i, name)])
        print('fp32 case %s map %2d: %.3e = %.2f x the reference fp32 deviation' % (name, i, err, err / dev))
        assert err <= BAR * dev
    for label, maps, bar in (('fp64', taps['maps'], 1e-9), ('fp32', taps32['maps'], BAR * float(kat['dev_boxes_' + name]))):
        for b in range(B):
            dec = R.decode_image(maps, b)
            tag = '%s_%d' % (name, b)
            for k in ('level', 'y', 'x'):
                assert np.array_equal(dec[k], kat['cand_%s_%s' % (k, tag)])
            order, keep, _ = R.greedy_nms(dec['dets'])
            kept, boxes = R.select(dec['dets'])
            check_decisions(kat, tag, dec['dets'], order, keep, kept, boxes, bar, label)


def test_threshold_in_front_of_the_nms_changes_nothing(kat):
    """A box is never suppressed by a lower-scoring one, so candidates at or below 0.5 cannot change what survives the final filter:
    on every fixture list, NMS over the candidates above 0.5 alone gives the reference's final boxes, and the survivors of the full
    pass that lie above 0.5 are exactly the survivors of the short pass."""
    n_low = 0
    for name, (B, _, _, _) in R.CASES.items():
        for b in range(B):
            tag = '%s_%d' % (name, b)
            dets = kat['cand_' + tag]
            kept, boxes = R.select(dets, floor=0.5)
            assert kept == kat['kept_' + tag].tolist() and np.array_equal(boxes, kat['boxes_' + tag])
            _, keep_full, _ = R.greedy_nms(dets)
            assert keep_full == kat['keep_' + tag].tolist()
            assert [i for i in keep_full if dets[i, 4] > 0.5] == kept
            low_kept = [i for i in keep_full if dets[i, 4] <= 0.5]
            n_low += len(low_kept)
            print('image %s: %d candidates, %d above 0.5; the full pass keeps %d, %d of them at or below 0.5' % (
                tag, len(dets), int((dets[:, 4] > 0.5).sum()), len(keep_full), len(low_kept)))
    assert n_low > 0          # the fixture does hold low boxes that survive the NMS and fall to the final filter


@pytest.mark.parametrize('name', ['a', 'b'])
def test_reference_batch_lists_give_the_per_image_result(kat, name):
    """At B = 2 batch_detect's list of image j holds every position at which ANY image passes, once per passing image.  Duplicates
    have IoU 1 with their twin and fall in the NMS, positions that pass only in the other image score at most 0.05 here and fall
    to the final filter: the final boxes are the per-image ones."""
    maps = fixture_maps(kat, name)
    lists = R.batch_quirk_lists(maps)
    for b, dets in enumerate(lists):
        tag = '%s_%d' % (name, b)
        own = kat['cand_' + tag]
        assert len(dets) > len(own)
        n_dup = len(dets) - len(np.unique(dets, axis=0))
        n_foreign = int((dets[:, 4] <= 0.05).sum())
        kept, boxes = R.select(dets)
        print('image %s: the batch list has %d rows for %d own candidates (%d repeated rows, %d rows at or below 0.05); %d final boxes' % (
            tag, len(dets), len(own), n_dup, n_foreign, len(boxes)))
        assert n_dup > 0 and n_foreign > 0
        want = kat['boxes_' + tag]
        assert boxes.shape == want.shape and float(np.abs(boxes - want).max()) <= 1e-9


def test_key_list_and_shapes_match_the_reference_module(kat, state):
    det = FD.S3FD()
    ours = ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in det.state_dict().items()]
    assert ours == [str(k) for k in kat['keys']]
    assert len(ours) == 65
    det.load_state_dict(state, strict=True)
    back = det.state_dict()
    assert all(torch.equal(back[k], state[k]) for k in state)
    convs = [m for m in det.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 31 and len([m for m in det.modules() if isinstance(m, FD.L2Norm)]) == 3
    assert [float(m.weight[0]) for m in (FD.S3FD().conv3_3_norm, FD.S3FD().conv4_3_norm, FD.S3FD().conv5_3_norm)] == [10.0, 8.0, 5.0]
    assert not any(p.requires_grad for p in det.parameters())
    with pytest.raises(RuntimeError):
        det.load_state_dict({k: v for k, v in state.items() if k != 'fc6.bias'}, strict=True)
    folded = det.folded(torch.float64)
    assert len(folded) == N.S3FD_PARAMS == 50
    assert [tuple(t.shape) for t in folded[38::2]] == [(8, 256, 3, 3), (6, 512, 3, 3), (6, 512, 3, 3), (6, 1024, 3, 3), (6, 512, 3, 3),
                                                       (6, 256, 3, 3)]
    w = torch.cat([state['conv4_3_norm_mbox_conf.weight'], state['conv4_3_norm_mbox_loc.weight']]).double()
    assert torch.equal(folded[40], w * state['conv4_3_norm.weight'].double().view(1, -1, 1, 1))
    twin = pickle.loads(pickle.dumps(copy.deepcopy(det)))
    assert twin._pack is None and torch.equal(twin.fc7.weight, det.fc7.weight)
    det.conv1_1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='forward only'):
        det.check()


def test_handmade_heads_restatement():
    """The hand-made head outputs decode to what they were built for: level 0 scores come from the maximum of the three background
    channels wherever it sits, every level passes at its first and last pixel, image 1 passes on level 0 only."""
    heads = R.handmade_heads()
    maps = R.maps_of_heads(heads)
    for b in range(2):
        dec = R.decode_image(maps, b)
        per_level = [int((dec['level'] == l).sum()) for l in range(R.LEVELS)]
        assert per_level == ([5, 2, 2, 2, 2, 2] if b == 0 else [5, 0, 0, 0, 0, 0])
        for i in np.nonzero(dec['level'] == 0)[0]:
            y, x = int(dec['y'][i]), int(dec['x'][i])
            q = heads[0][b, :, y, x].double()
            want = 1.0 / (1.0 + float(torch.exp(q[:3].max() - q[3])))
            assert abs(float(dec['dets'][i, 4]) - want) < 1e-6
        for l in range(R.LEVELS):
            h, w = heads[l].shape[2:]
            at = [(int(y), int(x)) for y, x, lv in zip(dec['y'], dec['x'], dec['level']) if lv == l]
            if b == 0 or l == 0:
                assert at[0] == (0, 0) and at[-1] == (h - 1, w - 1)
    mx = [int(heads[0][0, :3, y, x].argmax()) for y, x in ((1, 2), (2, 4), (3, 1))]
    assert mx == [0, 1, 2]


def test_select_face_rules():
    boxes = torch.zeros(4, 5, 5)
    boxes[0, :3] = torch.tensor([[1., 2, 3, 4, 0.999], [5, 6, 7, 8, 0.995], [9, 10, 11, 12, 0.7]])
    boxes[1, :2] = torch.tensor([[1., 1, 2, 2, 0.98], [3, 3, 4, 4, 0.6]])
    boxes[3, :2] = torch.tensor([[4., 4, 8, 8, 0.9999], [0, 0, 1, 1, 0.9995]])        # the second lies behind `kept`
    kept = torch.tensor([3, 2, 0, 1], dtype=torch.int32)
    faces, has = FD.select_face(boxes, kept, 'first')
    assert has.tolist() == [True, True, False, True]
    assert torch.equal(faces[0], boxes[0, 0]) and torch.equal(faces[1], boxes[1, 0]) and torch.equal(faces[3], boxes[3, 0])
    assert torch.equal(faces[2], torch.zeros(5))
    faces, has = FD.select_face(boxes, kept, 'last_above_0.99')
    assert has.tolist() == [True, False, False, True]
    assert torch.equal(faces[0], boxes[0, 1]) and torch.equal(faces[3], boxes[3, 0])
    assert torch.equal(faces[1], torch.zeros(5)) and torch.equal(faces[2], torch.zeros(5))
    # the reference's loop, literally
    for b in range(4):
        got = None
        for face in boxes[b, :int(kept[b])]:
            if face[4] > 0.99:
                got = face
        assert (got is None) == (not bool(has[b])) and (got is None or torch.equal(got, faces[b]))
    with pytest.raises(ValueError, match='rule'):
        FD.select_face(boxes, kept, 'largest')
    with pytest.raises(ValueError):
        FD.select_face(boxes[0], kept)
    with pytest.raises(ValueError):
        FD.select_face(boxes, kept[:2])


def test_arguments_are_checked():
    det = FD.S3FD()
    good = torch.zeros(1, 3, 64, 64)
    for bad in (torch.zeros(3, 64, 64), torch.zeros(1, 1, 64, 64), torch.zeros(1, 3, 31, 64), torch.zeros(1, 3, 64, 16), 'x'):
        with pytest.raises(ValueError):
            FD.detect(det, bad)
    with pytest.raises(RuntimeError, match='no CPU path'):
        FD.detect(det, good)
    with pytest.raises(RuntimeError, match='no CPU path'):
        FD.network(det, good)
    for cap in (0, -1, 16385, 2.5, True):
        with pytest.raises(ValueError, match='capacity'):
            FD._check_capacity(cap)
    for thr in (-0.1, 1.0, 'a', None):
        with pytest.raises(ValueError, match='threshold'):
            FD._check_threshold(thr)
    with pytest.raises(ValueError, match='input_range'):
        FD.detect_landmarks(det, None, good, input_range='0..1')
    with pytest.raises(ValueError, match='six'):
        FD.candidates_from_heads([good] * 5)
    with pytest.raises(ValueError, match='level 0'):
        FD.candidates_from_heads([torch.zeros(1, 6, 2, 2)] * 6)
    with pytest.raises(ValueError):
        FD.nms(torch.zeros(1, 4, 4), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU path'):
        FD.nms(torch.zeros(1, 4, 5), torch.zeros(1, dtype=torch.int32))


def test_c_abi_sizes_and_refusals():
    lib = N.load()
    assert lib.sgdfr_s3fd_pack_elems() >= sum(p.numel() for p in FD.S3FD().parameters()) - 256 - 512 - 512
    for (H, W), dims in R.LEVEL_DIMS.items():
        assert FD.level_dims(H, W) == dims
        assert lib.sgdfr_s3fd_map_elems(2, H, W) == 2 * 6 * sum(h * w for h, w in dims)
    assert FD.level_dims(32, 32) == [(8, 8), (4, 4), (2, 2), (5, 5), (3, 3), (2, 2)]
    assert FD.level_dims(256, 256)[3:] == [(12, 12), (6, 6), (3, 3)]
    for rows, H, W in ((0, 64, 64), (257, 64, 64), (1, 31, 64), (1, 64, 31), (1, 4097, 64), (256, 1024, 1024)):
        assert lib.sgdfr_s3fd_workspace_bytes(rows, H, W) == -1
        assert lib.sgdfr_s3fd_debug_elems(rows, H, W) == -1 and lib.sgdfr_s3fd_map_elems(rows, H, W) == -1
    assert lib.sgdfr_s3fd_workspace_bytes(1, 32, 32) > 0 and lib.sgdfr_s3fd_workspace_bytes(256, 256, 256) > 0
    with pytest.raises(RuntimeError, match='unsupported size 16x16'):
        FD.level_dims(16, 16)
    null = ctypes.c_void_p(None)
    rc = lib.sgdfr_s3fd_forward_f32(null, 1, 16, 64, 0, null, 0.5, 8, null, null, null, null, null, null, null, null, null, 0, null)
    assert rc == 1 and b'unsupported size' in lib.sgdfr_last_error()
    rc = lib.sgdfr_s3fd_forward_f32(null, 1, 64, 64, 0, null, 0.5, 0, null, null, null, null, null, null, null, null, null, 0, null)
    assert rc == 1 and b'capacity' in lib.sgdfr_last_error()
    rc = lib.sgdfr_s3fd_forward_f32(null, 1, 64, 64, 0, null, 0.5, 8, null, null, null, null, null, null, null, null, null, 0, null)
    assert rc == 1 and b'null pointer' in lib.sgdfr_last_error()
    rc = lib.sgdfr_s3fd_nms_f32(null, null, 1, 8, null, null, null, null)
    assert rc == 1 and b'null pointer' in lib.sgdfr_last_error()


def test_compat_install_face_detector(state):
    before = {k: sys.modules.get(k) for k in list(sys.modules) if k == 'libs' or k.startswith('libs.')}
    try:
        alias = compat.install_face_detector(state)
        assert alias == 'libs.face_models.sfd.sfd_detector'
        from libs.face_models.sfd.sfd_detector import SFDDetector, s3fd
        assert s3fd is FD.S3FD
        assert isinstance(SFDDetector.reference_scale, property)
        probe = SFDDetector.__new__(SFDDetector)
        assert (probe.reference_scale, probe.reference_x_shift, probe.reference_y_shift) == (195, 0, 0)
        assert callable(SFDDetector.detect_from_batch)
        with pytest.raises(RuntimeError):
            compat.install_face_detector({k: v for k, v in state.items() if not k.startswith('fc7.')})
        compat.install_face_detector()
        from libs.face_models.sfd.sfd_detector import SFDDetector as Bare
        with pytest.raises(ValueError, match='path_to_detector'):
            Bare('cuda')
    finally:
        for k in [k for k in sys.modules if k == 'libs' or k.startswith('libs.')]:
            if k not in before:
                del sys.modules[k]
        sys.modules.update({k: v for k, v in before.items() if v is not None})


# ---------------------------------------------------------------------------------------------------------------- the plan sweep
MARGIN = 16.0           # scripts/make_golden_s3fd.py's margin on every score decision, in units of the fp32 restatement's deviation
_PLAN_REFERENCE = {}
LONG_CAPACITY = 300     # the capacity at which R.long_heads' first image overflows in its second chunk of 256 positions


def plan_reference(state, name):
    """Shared with the GPU tests, computed once per process and never changed: the distinct images of a plan-sweep case and, per
    image, R.decisive_reference (fp64 and fp32 restatement on the CPU, one image at a time)."""
    import plan_rules as P
    _, H, W, sub, seeds = P.S3FD_CASES[name]
    key = (H, W, sub, seeds)
    if key not in _PLAN_REFERENCE:
        x = R.plan_images(S, H, W, seeds)
        _PLAN_REFERENCE[key] = (x, [R.decisive_reference(state, x[i:i + 1], sub) for i in range(len(seeds))])
    return _PLAN_REFERENCE[key]


def test_plan_rule_geometry_matches_the_c_abi():
    import plan_rules as P
    sizes = sorted({(H, W) for _, H, W, _, _ in P.S3FD_CASES.values()} | set(R.LEVEL_DIMS) | {(256, 256), (40, 56)})
    for H, W in sizes:
        assert P.s3fd_level_dims(H, W) == FD.level_dims(H, W), (H, W)
        launches = P.s3fd_launches(H, W)
        assert len(launches) == 25 and [bn for _, bn in launches] == [64] * 19 + [16] * 6
    assert P.s3fd_level_dims(32, 32) == [(8, 8), (4, 4), (2, 2), (5, 5), (3, 3), (2, 2)]
    for H in (63, 95):                                       # every pool drops a row or column: odd in front of each of the five
        h, odd = H, []
        for _ in range(5):
            odd.append(h % 2)
            h //= 2
        assert odd == [1] * 5, H
    # what the existing GPU test observes at 72 x 104: fewer sliced convs as the batch grows
    f = [P.s3fd_counts(B, 72, 104) for B in (1, 2, 3)]
    assert all(c == 25 for c, _ in f) and f[0][1] >= f[1][1] >= f[2][1] > 0 and f[0][1] > f[2][1], f
    # the workload profiles/s3fd_time.txt times runs the trunk and the level-0/1 heads whole
    whole = {l.name for l, S in P.s3fd_plan(48, 256, 256) if S == 1}
    assert {'conv1_2', 'conv3_3', 'conv4_3', 'conv5_3', 'fc6', 'fc7', 'head0', 'head1'} <= whole


def test_plan_cases_cover_every_launch_class_sliced_and_whole():
    """The coverage condition: over the GPU cases of test_gpu_s3fd_e4e_plans every launch class of csrc/s3fd.hip runs at least once
    sliced over K (epilogue in s3fd_finish_kernel) and at least once whole (epilogue in s3fd_conv_kernel): the trunk's 3 x 3 convs in
    front of a pool and not, the 1 x 1 convs, the stride-2 convs, fc6 with padding 3, the heads with the reciprocal-norm loader and
    without.  No exceptions: every class reaches both within 256 rows and 2^24 pixels."""
    import plan_rules as P
    want = {(c, how) for c in P.S3FD_CLASSES for how in ('sliced', 'whole')}
    plans = []
    for name, (B, H, W, _, seeds) in P.S3FD_CASES.items():
        assert 1 <= B <= P.S3FD_MAX_ROWS and B * H * W <= P.S3FD_MAX_PIXELS and len(seeds) <= 3
        plan = P.s3fd_plan(B, H, W)
        plans.append(plan)
        print('%-5s B = %3d %3d x %3d: %d convs, %d sliced; whole: %s' % (name, B, H, W, len(plan), sum(S > 1 for _, S in plan),
                                                                         ' '.join(l.name for l, S in plan if S == 1)))
    seen = P.coverage(plans, P.S3FD_CLASSES)
    print('exceptions: %s' % (list(P.S3FD_EXCEPTIONS) or 'none'))
    assert want - seen == set(P.S3FD_EXCEPTIONS) == set()
    whole = {name: {l.name for l, S in P.s3fd_plan(B, H, W) if S == 1} for name, (B, H, W, _, _) in P.S3FD_CASES.items()}
    assert whole['tiny'] == whole['odd'] == whole['mean'] == {'conv1_1'}                 # K = 27 again
    assert {'conv5_1', 'conv5_3', 'fc6', 'fc7', 'head0'} <= whole['b33'] and not {'head1', 'conv6_1'} & whole['b33']
    assert {'head1', 'conv6_1'} <= whole['b65'] and {'conv6_2', 'head3'} <= whole['b240']
    assert not {'conv6_2', 'head3'} & whole['b65']


def test_plan_cases_are_decisive(state):
    """Exact comparison of candidate counts, kept indices and their order on the GPU is fair only where the fp64 decisions are far
    from every cut: for exactly the images of the plan-sweep cases, every score is 16 x the fp32 restatement's score deviation away
    from 0.05 and 0.5, neighbours in the sorted list of which one is kept are as far apart, every IoU the greedy pass compares (in
    fp64 and in fp32) is 1e-3 away from 0.3, the fp32 restatement takes the same decisions, and every image has a face.
    The neighbour rule differs from scripts/make_golden_s3fd.py's, which asks the margin of every adjacent pair above 0.5: here a pair
    counts only if one of the two is kept.  Two suppressed neighbours are both suppressed by kept boxes ranked above them and suppress
    nothing themselves, so their order changes neither the kept indices nor their order, which is all the GPU test compares."""
    import plan_rules as P
    for name, (B, H, W, sub, seeds) in P.S3FD_CASES.items():
        x, refs = plan_reference(state, name)
        assert tuple(x.shape) == (len(seeds), 3, H, W) and len(set(seeds)) == len(seeds)
        for seed, r in zip(seeds, refs):
            im = r['images'][0]
            print('%-5s seed %3d: %3d candidates, %2d above 0.5, %2d kept; score gaps %.1f and %.1f x dev (bar %.0f), nearest IoU %.2e '
                  '(bar 1e-3), max |loc| %.2f, dev_boxes %.2e' % (name, seed, len(im['dets']), im['above'], len(im['kept']), r['gap_cut'],
                                                                r['gap_adjacent'], MARGIN, r['near_iou'], r['max_loc'], r['dev_boxes']))
            assert r['agree'] and r['gap_cut'] >= MARGIN and r['gap_adjacent'] >= MARGIN and r['near_iou'] >= 1e-3
            assert len(im['kept']) >= 1 and r['max_loc'] <= 5.0 and r['dev_boxes'] > 0 and np.isfinite(im['dets']).all()


def test_long_lists_are_what_the_kernel_tests_need():
    """The seeded lists of test_gpu_s3fd_e4e_plans' list-kernel tests: sizes as stated, every compared IoU 1e-3 away from 0.3 (the
    kernel and R.select do the same individually rounded float32 arithmetic, so even that margin is a courtesy)."""
    rows = R.nms_rows()
    ref = {k: R.nms_reference(d, c) for k, (d, c) in rows.items()}
    wide = R.nms_reference(R.nms_wide(), 300, 16384)
    for k, (kept, _, near, above) in list(ref.items()) + [('wide', wide)]:
        print('%-8s %4d boxes above 0.5, %3d kept, nearest IoU to 0.3 at %.2e' % (k, above, len(kept), near))
        assert near >= 1e-3
    assert all(d.dtype == np.float32 and d.shape[1] == 5 and len(d) <= R.NMS_CAPACITY for d, _ in rows.values())
    many, count = rows['many']
    assert count == len(many) == 800 and 700 <= count <= 900 and ref['many'][3] > 512 and len(ref['many'][0]) > 256
    low = np.nonzero(~(many[:, 4] > 0.5))[0]
    assert len(low) == 261 and low.min() < 64 and low.max() > 736 and bool((many[:, 4] == 0.5).any())        # interleaved
    # a later chunk of 256 sorted places lands inside an earlier one: fewer than 256 of the first 256 places survive and some survive
    # beyond place 256, so the second chunk's write base falls inside the first chunk; the same at place 512 for the third chunk
    sorted_ids = sorted(np.nonzero(many[:, 4] > 0.5)[0].tolist(), key=lambda i: (-many[i, 4], i))
    keep = np.isin(sorted_ids, ref['many'][0])
    assert [sorted_ids[p] for p in np.nonzero(keep)[0]] == ref['many'][0]
    for edge in (256, 512):
        print('many: %d of the first %d sorted places survive, %d beyond' % (keep[:edge].sum(), edge, keep[edge:].sum()))
        assert 0 < keep[:edge].sum() < edge and keep[edge:].sum() > 0
    # ... and inside a chunk a survivor's target is a place that a wave in front of its own still has to read (a survivor there)
    target = np.cumsum(keep) - 1
    crossing = [p for p in np.nonzero(keep)[0] if target[p] // 64 < p // 64 and target[p] // 256 == p // 256 and keep[target[p]]]
    print('many: %d survivors land on a surviving place of an earlier wave of their own chunk' % len(crossing))
    assert len(crossing) > 50
    # clusters: the kept box of a cluster suppresses members ranked more than 256 places (eight words of suppression bits) behind it
    cl, _ = rows['clusters']
    kept = ref['clusters'][0]
    assert len(cl) == 780 and ref['clusters'][3] == 780 and len(kept) == 33
    order = sorted(range(len(cl)), key=lambda i: (-cl[i, 4], i))
    rank = {i: p for p, i in enumerate(order)}
    far = [j for j in range(len(cl)) if j not in kept and any(R.iou_plus_one(cl[i], cl[j]) > 0.3 and rank[j] - rank[i] > 512
                                                              for i in kept[:3])]
    assert len(far) > 100
    # ties: exact copies 300 places apart lose to the lower index; equal scores elsewhere keep both, lower index first
    ti, _ = rows['ties']
    kept = ref['ties'][0]
    assert len(ti) == 600 and all(ti[i, 4] == ti[i + 300, 4] for i in range(300))
    assert set(kept) == set(range(300)) | set(range(301, 600, 2))
    assert all(kept.index(i) < kept.index(i + 300) for i in range(1, 300, 2))
    assert rows['over'][1] > R.NMS_CAPACITY == len(rows['over'][0]) and rows['none'][1] == 0 and len(rows['none'][0]) > 0
    # the hand-made heads: six chunks of 256 positions; image 0 fills chunk 0, leaves chunk 2 empty and passes in the last, partial
    # chunk and on every level; image 2 passes nowhere; every score is far from 0.05
    heads = R.long_heads()
    assert [tuple(h.shape[2:]) for h in heads] == list(R.PLAN_DIMS) == FD.level_dims(128, 128)
    maps = R.maps_of_heads(heads)
    start = np.cumsum([0] + [h * w for h, w in R.PLAN_DIMS])
    per_chunk = []
    for b in range(3):
        d = R.decode_image(maps, b)
        pos = start[d['level']] + d['y'] * np.array([R.PLAN_DIMS[l][1] for l in d['level']], dtype=np.int64) + d['x'] if len(d['dets']) else \
            np.zeros(0, dtype=np.int64)
        per_chunk.append(np.bincount(pos // 256, minlength=6).tolist())
        if b < 2:
            assert np.bincount(d['level'], minlength=6).min() >= 1
    print('passing positions per chunk of 256:', per_chunk)
    assert start[-1] == 1428 and per_chunk[0][0] == 256 and per_chunk[0][2] == 0 and per_chunk[0][5] > 0 and per_chunk[2] == [0] * 6
    assert per_chunk[0][0] < LONG_CAPACITY < per_chunk[0][0] + per_chunk[0][1]                  # the list overflows in the second chunk
    s = torch.cat([m.flatten() for m in R.scores_of(maps)])
    assert float((s - 0.05).abs().min()) > 1e-2


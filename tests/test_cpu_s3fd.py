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

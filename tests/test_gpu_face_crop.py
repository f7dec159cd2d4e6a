"""GPU: the alignment crop on the HIP kernels of csrc/facecrop.hip against the fixture kat16 (written from the reference's own
ffhq_cropping with PIL and scipy) and against the numpy restatement (tests/face_crop_restatement.py, itself pinned to the fixture and
to Pillow by test_cpu_face_crop).  Never against another run of the HIP code, except where two HIP runs must agree (batch rows,
composition).  Every test prints the figures it asserts on.

Bars: boxes, unpadded crops, the composition and the e4e tensor are exact.  The float crop of a padded row lies within PADDED_BOUND
of the reference's float32 crop on the 0..255 scale: 4 x the largest deviation measured on an MI355X over the six fixture cases.
That deviation is 0 in all six (the kernels keep scipy's summation order and numpy's float32 steps, so there is no
reordering left to absorb), hence the bound is 0: the float crop equals the reference's bit for bit.  For scale: the reference's own
float32 result lies 1.7e-5 from a float64 evaluation of its formulas, and anything above 1e-3 would be a defect.  Final bytes of a
padded row: within one level, at most 0.5 % of them different (measured: none differ).
"""
import numpy as np
import pytest
import torch

from util import S, golden
import face_crop_restatement as R
from test_cpu_face_crop import KAT, NOPAD, PADDED

pytestmark = pytest.mark.gpu

PADDED_BOUND = 4 * 0.0


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def FC():
    from stylegan_directions_face_reenactment_amd import face_crop
    return face_crop


def _case(kat, name):
    frame = kat['frame_' + str(kat['frame_of_' + name])]
    return frame, kat['lm_' + name], int(kat['size_' + name])


def _dev(frame, lm):
    return torch.from_numpy(frame).unsqueeze(0).cuda(), torch.from_numpy(lm).unsqueeze(0).cuda()


@pytest.fixture(scope='module')
def padded_runs(kat, FC):
    """One device run per padded fixture case: float crop, crop bytes, valid."""
    out = {}
    for name in PADDED:
        frame, lm, S_ = _case(kat, name)
        half = int(kat['box_' + name][2] - kat['box_' + name][0]) // 2         # all4's box is larger than the frame: beyond the default
        flt, crops, valid = FC.padded_float(*_dev(frame, lm), out_size=S_, max_size=max(half, max(frame.shape[:2]) // 2))
        out[name] = (None if flt[0] is None else flt[0].cpu().numpy(), crops[0].cpu().numpy(), valid.cpu().tolist())
    return out


def _landmarks(xr, yr):
    lm = np.empty((68, 2), np.float32)
    lm[:, 0] = np.linspace(xr[0], xr[1], 68)
    lm[:, 1] = np.linspace(yr[1], yr[0], 68)
    return lm


def test_boxes_exact(kat, FC):
    """Fixture boxes (centres on .5 both ways, size // 6, a fractional extent, negatives, an empty box) and the fixture cases' own."""
    lms = [kat['box_only_lm']] + [kat['lm_' + n][None] for n in NOPAD + PADDED]
    want = [kat['box_only_boxes']] + [kat['box_' + n][None] for n in NOPAD + PADDED]
    lms += [np.stack([_landmarks((10, 21), (10, 21)), _landmarks((10, 19), (10, 19))])]
    want += [np.array([[16 - 11, 16 - 1 - 11, 16 + 11, 16 - 1 + 11], [14 - 9, 14 - 1 - 9, 14 + 9, 14 - 1 + 9]], np.int32)]
    lm, want = np.concatenate(lms), np.concatenate(want)
    boxes, size = FC.crop_boxes(torch.from_numpy(lm).cuda())
    boxes, size = boxes.cpu().numpy(), size.cpu().numpy()
    bad = np.flatnonzero((boxes != want).any(1))
    print('boxes: %d rows, %d differ %s' % (len(want), len(bad), [(boxes[i].tolist(), want[i].tolist()) for i in bad[:4]]))
    assert len(bad) == 0
    assert np.array_equal(size, (want[:, 2] - want[:, 0]) // 2)
    for i, l in enumerate(lm):
        assert R.crop_box(l) == (tuple(int(v) for v in want[i]), int(size[i]))


@pytest.mark.parametrize('name', NOPAD)
def test_unpadded_crops_bit_exact(kat, FC, name):
    """80 -> 32, 74 -> 32 (no integer ratio), 20 -> 32 (upscale), 32 -> 32: the frame's bytes through Pillow's resampler."""
    frame, lm, S_ = _case(kat, name)
    crops, valid = FC.crop_using_landmarks(*_dev(frame, lm), out_size=S_)
    got, want = crops[0].cpu().numpy(), kat['out_' + name]
    n = int((got != want).sum())
    print('%s: side %d -> %d, %d of %d bytes differ' % (name, kat['box_' + name][2] - kat['box_' + name][0], S_, n, want.size))
    assert valid.cpu().tolist() == [1] and n == 0


def test_default_size_against_the_restatement(FC):
    """300 -> 256 on a 320 x 330 frame: the default out_size, several blocks per row, coefficients of a non-integer ratio."""
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (320, 330, 3), dtype=np.uint8)
    lm = _landmarks((165 - 75.25, 165 + 75.25), (185 - 30, 185 + 30))
    box, size = R.crop_box(lm)
    assert size == 150 and not any(R.borders(box, 320, 330))
    crops, valid = FC.crop_using_landmarks(*_dev(frame, lm))
    want = R.crop_using_landmarks(frame, lm)
    n = int((crops[0].cpu().numpy() != want).sum())
    print('300 -> 256: %d of %d bytes differ' % (n, want.size))
    assert valid.cpu().tolist() == [1] and tuple(crops.shape) == (1, 256, 256, 3) and n == 0


@pytest.mark.parametrize('name', PADDED)
def test_padded_float_stage(kat, padded_runs, name):
    """Border, mask, Gaussian, both blends and the median against the reference's float32 crop."""
    flt, _, valid = padded_runs[name]
    want = kat['float_' + name]
    assert valid == [1] and flt.shape == want.shape
    err = float(np.abs(flt.astype(np.float64) - want).max())
    print('%s: padded float crop %s max |HIP - reference| = %.3e (bound %.3e)' % (name, want.shape, err, PADDED_BOUND))
    assert err <= PADDED_BOUND


@pytest.mark.parametrize('name', PADDED)
def test_padded_composition_bit_exact(kat, padded_runs, name):
    """The device's bytes are Pillow's resampler applied to the truncation of the same run's float crop."""
    flt, got, _ = padded_runs[name]
    want = R.resize_bicubic(flt.astype(np.uint8), int(kat['size_' + name]))
    n = int((got != want).sum())
    print('%s: %d of %d bytes differ from resize(trunc(padded_float))' % (name, n, want.size))
    assert n == 0


@pytest.mark.parametrize('name', PADDED)
def test_padded_end_to_end(kat, padded_runs, name):
    _, got, _ = padded_runs[name]
    want = kat['out_' + name]
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print('%s: max level difference %d, %d of %d bytes differ (%.3f %%)' % (name, d.max(), (d > 0).sum(), d.size, 100.0 * (d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() <= 0.005


@pytest.mark.parametrize('level', [255, 0])
def test_flat_frame(FC, level):
    """A flat frame stays flat through border, Gaussian (double accumulation: 254.99998 would truncate to 254), median and resize."""
    frame = np.full((96, 128, 3), level, np.uint8)
    lm = _landmarks((-4.25, 20), (30, 50))
    box, _ = R.crop_box(lm)
    assert any(R.borders(box, 96, 128))
    crops, valid = FC.crop_using_landmarks(*_dev(frame, lm), out_size=48)
    got = crops.cpu().numpy()
    print('flat %d: min %d max %d' % (level, got.min(), got.max()))
    assert valid.cpu().tolist() == [1] and got.min() == level and got.max() == level


def test_batch_rows_independent(kat, FC):
    """B = 5: unpadded, padded, upscale, an empty box and a box beyond max_size; valid rows equal their B = 1 result bit for bit."""
    frame = kat['frame_b']
    point = np.tile(np.array([[40.0, 40.0]], np.float32), (68, 1))
    lms = np.stack([_landmarks((50, 80.5), (40, 60)), kat['lm_corner'], _landmarks((60, 70.25), (30, 35)), point, _landmarks((20, 85.5), (30, 60))])
    sizes = [R.crop_box(l)[1] for l in lms]
    assert sizes == [30, 24, 10, 0, 65] and not any(R.borders(R.crop_box(lms[0])[0], 96, 128))
    frames = torch.from_numpy(np.stack([frame] * 5)).cuda()
    (crops, x), valid = FC.crop_using_landmarks(frames, torch.from_numpy(lms).cuda(), out_size=32, as_tensor=True)
    print('batch: valid %s' % valid.cpu().tolist())
    assert valid.cpu().tolist() == [1, 1, 1, 0, 0]           # max_size defaults to 128 // 2
    assert int(crops[3:].max()) == 0 and float(x[3:].abs().max()) == 0.0
    for b in range(3):
        one, v1 = FC.crop_using_landmarks(*_dev(frame, lms[b]), out_size=32)
        n = int((one[0] != crops[b]).sum())
        print('batch row %d: %d bytes differ from its B = 1 run' % (b, n))
        assert v1.cpu().tolist() == [1] and n == 0
        if b != 1:                        # the unpadded rows are the restatement's bytes as well
            assert np.array_equal(one[0].cpu().numpy(), R.crop_using_landmarks(frame, lms[b], 32))


def test_e4e_tensor_bit_exact(kat, FC):
    frame, lm, S_ = _case(kat, 'left')
    (crops, x), _ = FC.crop_using_landmarks(*_dev(frame, lm), out_size=S_, as_tensor=True)
    want = crops.cpu().permute(0, 3, 1, 2).float().div(255.0) * 2 - 1
    assert tuple(x.shape) == (1, 3, S_, S_) and torch.equal(x.cpu(), want)


def test_input_checks(kat, FC):
    frame, lm, _ = _case(kat, 'left')
    f, l = _dev(frame, lm)
    for bad_f, bad_l in ((f.float(), l), (f[0], l), (f[..., :2], l), (f.permute(0, 2, 1, 3), l), (f, l.double()), (f, l[:, :67]),
                         (f, l.expand(2, 68, 2)), (f, l.transpose(1, 2).contiguous().transpose(1, 2)), (f.cpu(), l)):
        with pytest.raises(ValueError):
            FC.crop_using_landmarks(bad_f, bad_l)
    with pytest.raises(ValueError):
        FC.crop_using_landmarks(f, l, out_size=0)
    with pytest.raises(ValueError):
        FC.crop_using_landmarks(f, l, max_size=5000)
    with pytest.raises(ValueError):
        FC.crop_boxes(l.cpu())
    assert FC.crop_image(frame, np.tile(np.float32([[40, 40]]), (68, 1))) is None
    assert np.array_equal(FC.crop_image(frame, lm, out_size=int(kat['size_left'])), FC.crop_using_landmarks(f, l, out_size=48)[0][0].cpu().numpy())


def test_preprocess_frames_is_the_composition(FC):
    """reenact.preprocess_frames on a 96 x 128 batch with the synthetic S3FD / FAN weights equals detect_landmarks followed by
    crop_using_landmarks, bit for bit, and ok carries has_face."""
    import s3fd_restatement as R3
    from stylegan_directions_face_reenactment_amd import face_detector as FD, landmarks as L, reenact
    seed = int(golden('kat14_s3fd.npz')['seed'])
    det = FD.S3FD()
    det.load_state_dict(S.synthetic_s3fd_state(seed), strict=True)
    det = det.cuda()
    fan = L.FAN(4)
    fan.load_state_dict(S.synthetic_fan_state(20261208), strict=True)
    fan = fan.cuda().eval()
    x, _ = R3.fixture_inputs(S, seed, 'b')
    frames = x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    crops, e4e, ok = reenact.preprocess_frames(det, fan, frames, out_size=64)
    pts, _, has = FD.detect_landmarks(det, fan, frames.permute(0, 3, 1, 2).float(), rule='last_above_0.99', input_range='255')
    (want, want_x), valid = FC.crop_using_landmarks(frames, pts.contiguous(), out_size=64, as_tensor=True)
    print('preprocess_frames: has_face %s valid %s ok %s' % (has.tolist(), valid.tolist(), ok.tolist()))
    assert torch.equal(crops, want) and torch.equal(e4e, want_x)
    assert ok.dtype == torch.bool and ok.tolist() == [bool(h) and bool(v) for h, v in zip(has.tolist(), valid.tolist())]
    assert tuple(crops.shape) == (2, 64, 64, 3) and tuple(e4e.shape) == (2, 3, 64, 64)

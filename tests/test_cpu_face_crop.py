"""CPU: the numpy restatement of the alignment crop (tests/face_crop_restatement.py) against the fixture kat16 (written from the
reference's own ffhq_cropping by scripts/make_golden_face_crop.py) and against Pillow, and the host side of face_crop.

The GPU tests hold the device to the restatement and to the fixture, so this file is what ties both to the reference: boxes and final
bytes exactly, the float crop within one float32 ulp at 255 (2^-16), and a float64 evaluation of the same formulas on the same
final bytes (the condition under which the GPU end-to-end bound of one level on at most 0.5 % of the bytes is fair).
"""
import numpy as np
import pytest

from util import golden
import face_crop_restatement as R

KAT = 'kat16_face_crop.npz'
NOPAD = ('down80', 'ratio74', 'up20', 'same32')
PADDED = ('left', 'top', 'right', 'bottom', 'corner', 'all4')
PAIRS = ((100, 32), (37, 32), (20, 32), (7, 16), (64, 48), (300, 256), (513, 256))


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


def _case(kat, name):
    return kat['frame_' + str(kat['frame_of_' + name])], kat['lm_' + name], int(kat['size_' + name])


def test_fixture_layout(kat):
    assert tuple(str(n) for n in kat['names']) == NOPAD + PADDED
    layouts = {}
    for name in NOPAD + PADDED:
        frame, lm, S = _case(kat, name)
        H, W, _ = frame.shape
        layouts[name] = tuple(b > 0 for b in R.borders(tuple(kat['box_' + name]), H, W))
        assert kat['out_' + name].shape == (S, S, 3) and kat['out_' + name].dtype == np.uint8 and lm.dtype == np.float32
    assert all(layouts[n] == (False,) * 4 for n in NOPAD)
    # left, top, right, bottom alone, a corner, all four sides
    assert [layouts[n] for n in PADDED] == [(True, False, False, False), (False, True, False, False), (False, False, True, False),
                                            (False, False, False, True), (True, False, False, True), (True, True, True, True)]
    sides = {n: int(kat['box_' + n][2] - kat['box_' + n][0]) for n in NOPAD}
    assert sides == {'down80': 80, 'ratio74': 74, 'up20': 20, 'same32': 32} and all(int(kat['size_' + n]) == 32 for n in NOPAD)


def test_boxes_exact(kat):
    for lm, box in zip(kat['box_only_lm'], kat['box_only_boxes']):
        assert R.crop_box(lm)[0] == tuple(int(v) for v in box)
    for name in NOPAD + PADDED:
        assert R.crop_box(kat['lm_' + name])[0] == tuple(int(v) for v in kat['box_' + name])
    b = kat['box_only_boxes']
    assert b[0, 0] + b[0, 2] == 32 and b[1, 0] + b[1, 2] == 28           # centres 15.5 -> 16 and 14.5 -> 14
    assert R.crop_using_landmarks(kat['frame_a'], kat['box_only_lm'][5]) is None        # every landmark on one point


@pytest.mark.parametrize('name', NOPAD + PADDED)
def test_restatement_reproduces_the_fixture(kat, name):
    frame, lm, S = _case(kat, name)
    box, _ = R.crop_box(lm)
    if name in PADDED:
        mine, want = R.float_crop(frame, box), kat['float_' + name]
        err = float(np.abs(mine.astype(np.float64) - want).max())
        print('%s: float crop max |restatement - reference| = %.3e' % (name, err))
        assert mine.dtype == np.float32 and mine.shape == want.shape and err <= 2.0 ** -16
    assert np.array_equal(R.crop_using_landmarks(frame, lm, S), kat['out_' + name])


@pytest.mark.parametrize('name', PADDED)
def test_float64_evaluation_gives_the_same_bytes(kat, name):
    frame, lm, S = _case(kat, name)
    box, _ = R.crop_box(lm)
    f32, f64 = R.float_crop(frame, box), R.float_crop(frame, box, np.float64)
    print('%s: max |float32 - float64| = %.3e' % (name, float(np.abs(f32 - f64).max())))
    assert np.array_equal(f32.astype(np.uint8), f64.astype(np.uint8))
    assert np.array_equal(R.crop_using_landmarks(frame, lm, S, dtype=np.float64), kat['out_' + name])


@pytest.mark.parametrize('pair', PAIRS)
def test_resampler_equals_pillow(pair):
    Image = pytest.importorskip('PIL.Image')
    n, S = pair
    rng = np.random.default_rng(n)
    img = rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
    img[: n // 3] = (img[: n // 3] > 127) * 255                      # hard edges: the overshoot has to clip as Pillow's does
    want = np.array(Image.fromarray(img).resize((S, S), Image.BICUBIC))
    assert np.array_equal(R.resize_bicubic(img, S), want)


def test_flat_frames_stay_flat():
    for level in (0, 255):
        frame = np.full((96, 128, 3), level, np.uint8)
        crop = R.float_crop(frame, (-16, 12, 32, 60))
        assert crop.dtype == np.float32 and float(crop.min()) == level == float(crop.max())


def test_host_checks_and_none_return(monkeypatch):
    import torch
    from stylegan_directions_face_reenactment_amd import face_crop as FC
    image, lm = np.zeros((96, 128, 3), np.uint8), np.zeros((68, 2), np.float32)
    for bad in (image.astype(np.float32), image[:, :, :2], image[0], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            FC.crop_image(bad, lm)
    with pytest.raises(ValueError):
        FC.crop_image(image, lm[:67])
    f, l = torch.zeros((1, 96, 128, 3), dtype=torch.uint8), torch.zeros((1, 68, 2))
    with pytest.raises(ValueError, match='no CPU path'):
        FC.crop_using_landmarks(f, l)
    with pytest.raises(ValueError, match='no CPU path'):
        FC.crop_boxes(l)
    for bad_f, bad_l in ((f.float(), l), (f[0], l), (f.permute(0, 2, 1, 3), l), (f, l.double()), (f, l[:, :60])):
        with pytest.raises(ValueError):
            FC.crop_using_landmarks(bad_f, bad_l)
    # the numpy wrapper returns None for a row the device marks invalid, the crop otherwise
    seen = {}

    def fake(frames, landmarks, out_size=256, max_size=None, as_tensor=False):
        seen['shapes'] = (tuple(frames.shape), frames.dtype, tuple(landmarks.shape), landmarks.dtype)
        return torch.full((1, out_size, out_size, 3), 7, dtype=torch.uint8), torch.tensor([seen['valid']], dtype=torch.int32)

    monkeypatch.setattr(FC, 'crop_using_landmarks', fake)
    seen['valid'] = 0
    assert FC.crop_image(image, lm.astype(np.float64), device='cpu') is None
    assert seen['shapes'] == ((1, 96, 128, 3), torch.uint8, (1, 68, 2), torch.float32)
    seen['valid'] = 1
    out = FC.crop_image(image, lm, out_size=16, device='cpu')
    assert out.shape == (16, 16, 3) and out.dtype == np.uint8 and int(out.min()) == 7


def test_compat_mount():
    import sys
    from stylegan_directions_face_reenactment_amd import compat
    keep = {k: sys.modules.get(k) for k in ('libs', 'libs.face_models', compat.FACE_CROP_ALIAS)}
    try:
        assert compat.install_face_crop() == 'libs.face_models.ffhq_cropping'
        from libs.face_models.ffhq_cropping import crop_using_landmarks
        with pytest.raises(ValueError):
            crop_using_landmarks(np.zeros((4, 4), np.uint8), np.zeros((68, 2)))
    finally:
        for k, v in keep.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v

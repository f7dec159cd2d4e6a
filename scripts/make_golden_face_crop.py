"""Writes tests/golden/kat16_face_crop.npz from the reference's own alignment crop (libs/face_models/ffhq_cropping.py).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_face_crop.py        (CPU only, seconds; needs PIL and scipy)

ffhq_cropping imports cv2 for one call, copyMakeBorder(..., BORDER_REFLECT); a stub module supplies it as
np.pad(mode='symmetric'), which is the same border (cba|abc|cba).  crop_using_landmarks hard-codes a 256 x 256 output, so its
pieces are called: the box is captured from its own call of crop_from_bbox, the float crop is crop_from_bbox's return value
(pad_img_to_fit_bbox's image where the box leaves the frame), and the final bytes are its own two lines,
Image.fromarray(crop.astype(np.uint8)).resize((S, S), Image.BICUBIC), at S = 32 / 48 / 64.

The file holds arrays only: two frames, per case the landmarks, the box, the float crop (padded cases) and the final uint8 crop,
and a list of landmark sets with their boxes alone.  The script ASSERTS that the restatement (tests/face_crop_restatement.py)
reproduces every array and that a float64 evaluation of the same formulas gives the same final bytes, so that the GPU tests may
hold the device to a one-level, 0.5 % bound against these bytes.  If an assertion fails, change the seed, not the assertion.
No border width is a multiple of 3: at the pixel 4/3 of such a width from the edge the first blend's weight, clip(3 mask + 1),
is exactly 0 in float32 but 2e-16 in double, which moves an untouched integer pixel below its integer.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import face_crop_restatement as R                                                 # noqa: E402

SEED = 20261018
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat16_face_crop.npz')

# name, frame, out_size, box centre (x, y) after the size // 6 shift, size
NOPAD = (('down80', 'a', 32, 80, 60, 40), ('ratio74', 'a', 32, 70, 62, 37), ('up20', 'a', 32, 100, 40, 10), ('same32', 'a', 32, 50, 90, 16))
PADDED = (('left', 'b', 48, 14, 48, 24), ('top', 'b', 64, 64, 14, 24), ('right', 'b', 48, 115, 50, 24), ('bottom', 'b', 32, 60, 85, 24),
          ('corner', 'b', 48, 13, 80, 24), ('all4', 'b', 64, 64, 47, 66))
FRAMES = {'a': (120, 160), 'b': (96, 128)}
# x extent (min, max), y extent (min, max): centres on .5 both ways, size // 6, a fractional extent that truncates, negatives
BOX_ONLY = (((10, 21), (10, 21)), ((10, 19), (10, 19)), ((10, 21), (30, 43)), ((3.25, 27.24), (5, 9)), ((-8, -3), (-20.5, 4)),
            ((40, 40), (17, 17)), ((0.5, 99.75), (7.5, 60.5)), ((11, 24), (100, 101)))


def _reference():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref or not os.path.isdir(ref):
        raise SystemExit('set SGDFR_REFERENCE to a checkout of the reference')
    cv2 = types.ModuleType('cv2')
    cv2.BORDER_REFLECT = 2
    cv2.copyMakeBorder = lambda img, top, bottom, left, right, kind: np.pad(img, ((top, bottom), (left, right), (0, 0)), mode='symmetric')
    sys.modules['cv2'] = cv2
    sys.path.insert(0, ref)
    from libs.face_models import ffhq_cropping
    return ffhq_cropping


def make_frame(rng, H, W):
    """A smooth scene with blobs, edges and noise that touches 0 and 255."""
    y, x = np.mgrid[:H, :W].astype(np.float64)
    img = np.stack([120 + 100 * np.sin(x / 17.0 + c) * np.cos(y / 23.0 - c) + 40 * ((x // 16 + y // 12 + c) % 2) for c in range(3)], -1)
    img += rng.normal(0, 25, img.shape)
    return np.clip(img, 0, 255).round().astype(np.uint8)


def make_landmarks(rng, xr, yr):
    """68 points whose extremes are exactly xr and yr."""
    lm = np.stack([rng.uniform(xr[0], xr[1], 68), rng.uniform(yr[0], yr[1], 68)], 1)
    lm[0], lm[1] = (xr[0], yr[1]), (xr[1], yr[0])
    return lm.astype(np.float32)


def landmarks_for(rng, cx, cy, size):
    """Landmarks whose box has centre (cx, cy) after the shift and half side `size`."""
    e = size + 0.375
    cy = cy + size // 6
    return make_landmarks(rng, (cx - e / 2, cx + e / 2), (cy - e / 4, cy + e / 4))


def reference_box(ref, frame, lm):
    seen = []
    keep = ref.crop_from_bbox
    ref.crop_from_bbox = lambda img, bbox: (seen.append(tuple(int(v) for v in bbox)), np.zeros((4, 4, 3), np.uint8))[1]
    try:
        ref.crop_using_landmarks(frame, lm)
    finally:
        ref.crop_from_bbox = keep
    return seen[0]


def main():
    from PIL import Image
    ref = _reference()
    rng = np.random.default_rng(SEED)
    out = {'seed': np.int64(SEED)}
    frames = {k: make_frame(rng, *hw) for k, hw in FRAMES.items()}
    for k, f in frames.items():
        out['frame_' + k] = f
    names = []
    for padded, cases in ((False, NOPAD), (True, PADDED)):
        for name, fk, S, cx, cy, size in cases:
            frame = frames[fk]
            lm = landmarks_for(rng, cx, cy, size)
            box = reference_box(ref, frame, lm)
            assert box == (cx - size, cy - size, cx + size, cy + size), (name, box)
            H, W, _ = frame.shape
            assert any(R.borders(box, H, W)) == padded and all(b <= d for b, d in zip(R.borders(box, H, W), (W, H, W, H))), name
            crop = ref.crop_from_bbox(frame.copy(), box)
            final = np.array(Image.fromarray(crop.astype(np.uint8)).resize((S, S), Image.BICUBIC))
            # the restatement equals the reference, and the float64 evaluation lands on the same bytes
            assert R.crop_box(lm) == (box, size), name
            mine = R.float_crop(frame, box)
            assert mine.shape == crop.shape and float(np.abs(mine.astype(np.float64) - crop).max()) <= 255 * 2.0 ** -23, name
            assert np.array_equal(R.crop_using_landmarks(frame, lm, S), final), name
            assert np.array_equal(R.crop_using_landmarks(frame, lm, S, dtype=np.float64), final), name
            names.append(name)
            out.update({'lm_' + name: lm, 'box_' + name: np.array(box, np.int32), 'out_' + name: final, 'frame_of_' + name: np.array(fk),
                        'size_' + name: np.int32(S)})
            if padded:
                assert crop.dtype == np.float32
                out['float_' + name] = crop
    out['names'] = np.array(names)
    lms = np.stack([make_landmarks(rng, xr, yr) for xr, yr in BOX_ONLY])
    boxes = np.array([reference_box(ref, frames['a'], lm) for lm in lms], np.int32)
    for lm, b in zip(lms, boxes):
        assert R.crop_box(lm)[0] == tuple(b)
    assert boxes[0, 0] + boxes[0, 2] == 32 and boxes[1, 0] + boxes[1, 2] == 28, boxes[:2]         # 15.5 -> 16, 14.5 -> 14
    out['box_only_lm'], out['box_only_boxes'] = lms, boxes
    np.savez_compressed(OUT, **out)
    print('wrote %s: %d bytes, cases %s' % (OUT, os.path.getsize(OUT), ' '.join(names)))


if __name__ == '__main__':
    main()

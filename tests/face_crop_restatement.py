"""Plain-numpy restatement of the reference's FFHQ alignment crop (libs/face_models/ffhq_cropping.py): the box, the reflected
border, the feathered Gaussian and median blends of pad_img_to_fit_bbox, and Pillow's 8-bit bicubic resampler.  No PIL, scipy or
reference import, so a GPU test can compare any shape against it.  tests/test_cpu_face_crop.py pins it to the fixture (made from
the reference's own code) and to Pillow.

`dtype=np.float32` follows the reference's number formats step by step (scipy filters a float32 image with double weights and a
double accumulator and rounds to float32 after each axis; numpy's mask and blends are float32).  `dtype=np.float64` evaluates the
same formulas in double throughout.
"""
import numpy as np

SIGMA, RADIUS = 5.0, 20            # scipy: radius = int(4.0 * sigma + 0.5)
PRECISION_BITS = 32 - 8 - 2        # Pillow's Resample.c


def crop_box(landmarks):
    """(x1, y1, x2, y2), size of ffhq_cropping.crop_using_landmarks (:51-61) for landmarks [68,2] float32."""
    lm = np.asarray(landmarks, dtype=np.float32)
    center = ((lm.min(0) + lm.max(0)) / 2).round().astype(int)
    size = int(max(lm[:, 0].max() - lm[:, 0].min(), lm[:, 1].max() - lm[:, 1].min()))
    center[1] -= size // 6
    return (int(center[0]) - size, int(center[1]) - size, int(center[0]) + size, int(center[1]) + size), size


def borders(box, H, W):
    """(left, top, right, bottom) border widths of a box on an H x W frame."""
    x1, y1, x2, y2 = box
    return max(-x1, 0), max(-y1, 0), max(x2 - W, 0), max(y2 - H, 0)


def gaussian_weights():
    x = np.arange(-RADIUS, RADIUS + 1)
    phi = np.exp(-0.5 / (SIGMA * SIGMA) * x ** 2)
    return phi / phi.sum()


def _gauss_axis(a, axis, w):
    """scipy.ndimage.correlate1d with a symmetric kernel and mode='reflect': the centre tap first, then the pairs from the
    outermost inwards, everything in double."""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    n = a.shape[0]
    p = np.pad(a, [(RADIUS, RADIUS)] + [(0, 0)] * (a.ndim - 1), mode='symmetric')
    acc = p[RADIUS:RADIUS + n] * w[RADIUS]
    for j in range(RADIUS, 0, -1):
        acc = acc + (p[RADIUS - j:RADIUS - j + n] + p[RADIUS + j:RADIUS + j + n]) * w[RADIUS - j]
    return np.moveaxis(acc, 0, axis)


def gaussian(img, dtype=np.float32):
    w = gaussian_weights()
    t = _gauss_axis(img, 0, w).astype(dtype)
    return _gauss_axis(t, 1, w).astype(dtype)


def feather_mask(h, w, pad, dtype=np.float32):
    """pad = (left, top, right, bottom); the reference's mask [h,w,1]."""
    y, x = np.ogrid[:h, :w]
    pad = np.array(pad, dtype=dtype)
    pad[pad == 0] = 1e-10
    one = dtype(1.0)
    m = np.maximum(one - np.minimum(x.astype(dtype) / pad[0], (w - 1 - x).astype(dtype) / pad[2]),
                   one - np.minimum(y.astype(dtype) / pad[1], (h - 1 - y).astype(dtype) / pad[3]))
    return m[:, :, None].astype(dtype)


def median(img, dtype=np.float32):
    """np.median over axes (0, 1): the middle value, or the mean of the two middle values in the array's own type."""
    flat = np.sort(img.reshape(-1, img.shape[2]), axis=0)
    n = flat.shape[0]
    if n % 2:
        return flat[n // 2].astype(dtype)
    return ((flat[n // 2 - 1] + flat[n // 2]) / dtype(2)).astype(dtype)


def first_blend(frame, box, dtype=np.float32):
    """pad_img_to_fit_bbox up to its median: the padded frame after the Gaussian blend (what np.median sees), and the mask."""
    H, W, _ = frame.shape
    pl, pt, pr, pb = borders(box, H, W)
    img = np.pad(frame, ((pt, pb), (pl, pr), (0, 0)), mode='symmetric').astype(dtype)
    h, w, _ = img.shape
    mask = feather_mask(h, w, (pl, pt, pr, pb), dtype)
    img = img + (gaussian(img, dtype) - img) * np.clip(mask * dtype(3.0) + dtype(1.0), dtype(0.0), dtype(1.0))
    return img, mask


def padded_frame(frame, box, dtype=np.float32):
    """pad_img_to_fit_bbox: the whole padded frame after both blends, and the box moved into it."""
    H, W, _ = frame.shape
    pl, pt, pr, pb = borders(box, H, W)
    img, mask = first_blend(frame, box, dtype)
    img = img + (median(img, dtype) - img) * np.clip(mask, dtype(0.0), dtype(1.0))
    x1, y1, x2, y2 = box
    return img, (x1 + pl, y1 + pt, x2 + pl, y2 + pt)


def float_crop(frame, box, dtype=np.float32):
    """crop_from_bbox: the crop before astype(np.uint8); float only where the box leaves the frame (else the frame's own bytes)."""
    x1, y1, x2, y2 = box
    H, W, _ = frame.shape
    if x1 < 0 or y1 < 0 or x2 > W or y2 > H:
        img, (x1, y1, x2, y2) = padded_frame(frame, box, dtype)
        return img[y1:y2, x1:x2]
    return frame[y1:y2, x1:x2]


# ---------------------------------------------------------------------------------------------------------------- Pillow's resampler
def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def bicubic_coeffs(in_size, out_size):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc -> [(xmin, int32 coefficients)] per output index."""
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(xmax) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w:                                 # summed in index order, as the C loop does
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)   # (int): towards 0
        out.append((xmin, k.astype(np.int32)))
    return out


def _resample_axis0(a, out_size):
    """One pass along axis 0 of a uint8 array; a pass whose size does not change is skipped, as ImagingResample does."""
    n = a.shape[0]
    if n == out_size:
        return a
    out = np.empty((out_size,) + a.shape[1:], dtype=np.uint8)
    src = a.astype(np.int64)
    for xx, (xmin, k) in enumerate(bicubic_coeffs(n, out_size)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k.astype(np.int64), src[xmin:xmin + len(k)], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic(img, out_size):
    """Image.fromarray(img).resize((S, S), Image.BICUBIC) for a uint8 [h,w,3] array: horizontal pass, uint8, vertical pass."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    t = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), out_size), 0, 1)
    return np.ascontiguousarray(_resample_axis0(t, out_size))


def crop_using_landmarks(frame, landmarks, out_size=256, dtype=np.float32):
    """The reference's crop_using_landmarks with its 256 as a parameter; None where its box is empty."""
    box, size = crop_box(landmarks)
    if size < 1:
        return None
    return resize_bicubic(float_crop(frame, box, dtype).astype(np.uint8), out_size)

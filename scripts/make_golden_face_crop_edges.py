"""Writes tests/golden/kat17_face_crop_edges.npz from the reference's own alignment crop, as make_golden_face_crop.py writes kat16
(same SGDFR_REFERENCE and cv2-stub mechanism, same assertions per case: the restatement equals the reference on the box, on the
float crop within 255 * 2^-23 and on the final bytes exactly, and a float64 evaluation lands on the same bytes).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_face_crop_edges.py      (CPU only, under a minute)

The cases are the ones kat16 does not reach (tests/test_cpu_face_crop_edges.py lists them again and checks their preconditions):

  median    med_p0 .. med_p3: the lower and the upper middle value of the blended padded frame differ first in byte 0 / 1 / 2 / 3 of
            their bit patterns (the pass of the 8-bit radix select at which the two prefixes part), in every channel; med_odd: both
            padded dimensions odd, so there is one middle value.  The pair is PLACED: pixels more than 20 + ceil(4/3 border) from a
            padded side and more than 21 from an unpadded one (whose first line is fully blended, the 1e-10 quirk) keep their own
            value through the Gaussian blend and reach no blended pixel, so they are ballast: as many of them are set below the
            pair as its lower value needs to sit at rank n/2 - 1, the others above.  Pass 0 and 1 take integer pairs (1/2, 7/8,
            127/128 and 100/101, 2/3, 47/48) on a scene kept above them; pass 2 and 3 take two adjacent blended values.
  border    eq_w / eq_h: a left border exactly as wide as the frame, a bottom border exactly as high.
  short     short_top (9 x 64 frame, top border 5) and short_right (64 x 13, right border 6): the padded dimension is below the
            Gaussian's radius, so its reflection wraps more than once.
  cap       a 300 x 400 frame with max_size 200 (the workspace's padded frame is 600 x 800: more than 2^20 values), box side 300.
  resample  2 -> 5, 6 -> 1, 24 -> 1024, 400 -> 16, and side 24 with max_size 200, on padded and on unpadded rows.  The 1024 x 1024
            outputs are held as 28 full rows plus the row and column sums, to keep the file small.

If the float64 condition fails for a case its seed moves on by one (SEED + 1000 * index + attempt), never the assertion.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import face_crop_restatement as R                                                 # noqa: E402
import make_golden_face_crop as G                                                 # noqa: E402

SEED = 20261019
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat17_face_crop_edges.npz')
FLOAT_SIDE = 160                     # the float crop is stored up to this crop side
DIGEST_ROWS = tuple(range(8)) + tuple(range(506, 518)) + tuple(range(1016, 1024))

# name, (H, W), out_size, max_size (None: the default max(H, W) // 2), box centre (x, y) after the size // 6 shift, size, extra
#   extra: ('median', kind) with kind 0..3 the parting pass or 'odd'; ('shared', key) to reuse one frame; None
CASES = (
    ('med_p0', (200, 210), 48, None, 14, 100, 24, ('median', 0)),
    ('med_p1', (210, 200), 48, None, 100, 14, 24, ('median', 1)),
    ('med_p2', (96, 118), 48, None, 104, 48, 24, ('median', 2)),
    ('med_p3', (118, 96), 48, None, 48, 104, 24, ('median', 3)),
    ('med_odd', (95, 121), 48, None, 14, 47, 24, ('median', 'odd')),
    ('eq_w', (44, 25), 32, None, -5, 22, 20, None),
    ('eq_h', (25, 44), 32, None, 22, 30, 20, None),
    ('short_top', (9, 64), 16, None, 30, 2, 7, None),
    ('short_right', (64, 13), 16, None, 10, 30, 9, None),
    ('cap', (300, 400), 32, 200, 113, 121, 150, ('shared', 'c')),
    ('r400to16', (300, 400), 16, 200, 150, 156, 200, ('shared', 'c')),
    ('r2to5_in', (64, 80), 5, None, 40, 30, 1, ('shared', 'd')),
    ('r2to5_pad', (64, 80), 5, None, 0, 30, 1, ('shared', 'd')),
    ('r6to1_in', (64, 80), 1, None, 40, 30, 3, ('shared', 'd')),
    ('r6to1_pad', (64, 80), 1, None, 79, 62, 3, ('shared', 'd')),
    ('r24to1024_in', (64, 80), 1024, None, 40, 30, 12, ('shared', 'd')),
    ('r24to1024_pad', (64, 80), 1024, None, 8, 30, 12, ('shared', 'd')),
    ('m200_in', (64, 80), 32, 200, 41, 31, 12, ('shared', 'd')),
    ('m200_pad', (64, 80), 32, 200, 30, 59, 12, ('shared', 'd')),
)
INT_PAIRS = {0: ((1, 2), (7, 8), (127, 128)), 1: ((100, 101), (2, 3), (47, 48))}     # per channel; the scene stays above 140


def first_differing_byte(a, b):
    """Index (0 = most significant) of the first byte in which the bit patterns of two float32 differ; 4 if they are equal."""
    x = int(np.float32(a).view(np.uint32)) ^ int(np.float32(b).view(np.uint32))
    return 4 if x == 0 else 3 - (x.bit_length() - 1) // 8


def free_pixels(H, W, pad):
    """Frame pixels that keep their own value through the Gaussian blend and reach no blended pixel -> bool [H, W]."""
    pl, pt, pr, pb = pad
    near = lambda p: 20 + -(-4 * p // 3) if p else 21
    y, x = np.mgrid[:H, :W]
    return (x + pl > near(pl)) & (W - 1 - x + pr > near(pr)) & (y + pt > near(pt)) & (H - 1 - y + pb > near(pb))


def place_median(rng, scene, box, kind):
    """Ballast on the free pixels of `scene` so that the two middle values of the blended padded frame part at pass `kind` (or, for
    'odd', so that the single middle value is a blended one) -> frame, middle values [3,2]."""
    H, W, _ = scene.shape
    pad = R.borders(box, H, W)
    free = free_pixels(H, W, pad)
    probe = scene.copy()
    probe[free] = 255
    blend, _ = R.first_blend(probe, box)
    other = scene.copy()
    other[free] = 0
    blend0, _ = R.first_blend(other, box)
    pfree = np.zeros(blend.shape[:2], bool)
    pfree[pad[1]:pad[1] + H, pad[0]:pad[0] + W] = free
    # the ballast is ballast: it changes no value but its own
    assert np.array_equal(blend[~pfree], blend0[~pfree]) and (blend[pfree] == 255).all() and (blend0[pfree] == 0).all()
    n, nfree = blend.shape[0] * blend.shape[1], int(free.sum())
    frame, mids = scene.copy(), np.zeros((3, 2), np.float32)
    for c in range(3):
        fixed = np.sort(blend[..., c][~pfree])
        if kind in INT_PAIRS:
            a, b = (np.float32(v) for v in INT_PAIRS[kind][c])
            assert fixed[0] > b
        else:
            vals = np.unique(fixed)
            vals = vals[vals != np.floor(vals)]
            if kind == 'odd':
                a = b = vals[len(vals) // 2]
            else:
                lo, hi = vals[:-1], vals[1:]
                ok = np.array([first_differing_byte(p, q) == kind for p, q in zip(lo, hi)]) & (np.floor(lo) == np.floor(hi))
                at = np.flatnonzero(ok)
                at = at[np.argmin(np.abs(at - len(vals) // 2))]           # the candidate nearest the scene's own middle
                a, b = lo[at], hi[at]
                assert not ((fixed > a) & (fixed < b)).any()
        low = (n + 1) // 2 - int((fixed <= a).sum())                      # values <= a: n / 2 of them (odd n: rank (n - 1) / 2 is a)
        assert 0 < low < nfree, (kind, c, low, nfree)
        fill = np.empty(nfree, np.uint8)
        below, above = int(np.ceil(a)) - (a != np.floor(a)), int(np.floor(b)) + (b != np.floor(b))
        fill[:low] = rng.integers(max(below - 3, 0), below + 1, low)
        fill[low:] = rng.integers(above, min(above + 3, 255) + 1, nfree - low)
        if kind in INT_PAIRS:
            fill[0], fill[low] = below, above                             # the pair itself is present
        order = rng.permutation(nfree)
        plane = frame[..., c]
        plane[free] = fill[np.argsort(order)]
        mids[c] = a, b
    return frame, mids


def middle_values(frame, box):
    """The two middle values per channel of what np.median sees -> [3,2] float32, n."""
    blend, _ = R.first_blend(frame, box)
    flat = np.sort(blend.reshape(-1, 3), axis=0)
    n = flat.shape[0]
    return np.stack([flat[(n - 1) // 2], flat[n // 2]], 1), n


def reference_crop(ref, frame, box):
    """crop_from_bbox, and the median it took (None for a box inside the frame)."""
    seen, keep = [], np.median
    np.median = lambda *a, **k: (seen.append(keep(*a, **k)), seen[-1])[1]
    try:
        crop = ref.crop_from_bbox(frame.copy(), box)
    finally:
        np.median = keep
    return crop, (np.asarray(seen[0], np.float32) if seen else None)


def scene(rng, H, W, kind):
    f = G.make_frame(rng, H, W)
    if kind in INT_PAIRS:
        f = (140 + f.astype(np.float64) * (115.0 / 255.0)).round().astype(np.uint8)
    return f


def main():
    from PIL import Image
    ref = G._reference()
    out = {'seed': np.int64(SEED)}
    shared, names = {}, []
    for index, (name, (H, W), S, M, cx, cy, size, extra) in enumerate(CASES):
        box = (cx - size, cy - size, cx + size, cy + size)
        pad = R.borders(box, H, W)
        for attempt in range(50):
            rng = np.random.default_rng(SEED + 1000 * index + attempt)
            lm = G.landmarks_for(rng, cx, cy, size)
            mids = None
            if extra and extra[0] == 'shared':
                if extra[1] not in shared:
                    shared[extra[1]] = G.make_frame(np.random.default_rng(SEED + 500 + len(shared)), H, W)
                frame = shared[extra[1]]
            elif extra:
                frame, mids = place_median(rng, scene(rng, H, W, extra[1]), box, extra[1])
            else:
                frame = G.make_frame(rng, H, W)
            if not any(pad) or np.array_equal(R.crop_using_landmarks(frame, lm, S, dtype=np.float64), R.crop_using_landmarks(frame, lm, S)):
                break
        else:
            raise SystemExit('%s: no seed meets the float64 condition' % name)
        assert G.reference_box(ref, frame, lm) == box and R.crop_box(lm) == (box, size), name
        assert all(b <= d for b, d in zip(pad, (W, H, W, H))), name
        crop, med = reference_crop(ref, frame, box)
        final = np.array(Image.fromarray(crop.astype(np.uint8)).resize((S, S), Image.BICUBIC))
        mine = R.float_crop(frame, box)
        err = float(np.abs(mine.astype(np.float64) - crop).max())
        assert mine.shape == crop.shape == (2 * size, 2 * size, 3) and err <= 255 * 2.0 ** -23, (name, err)
        assert np.array_equal(R.crop_using_landmarks(frame, lm, S), final), name
        assert np.array_equal(R.crop_using_landmarks(frame, lm, S, dtype=np.float64), final), name
        fk = extra[1] if extra and extra[0] == 'shared' else name
        out['frame_' + fk] = frame
        out.update({'lm_' + name: lm, 'box_' + name: np.array(box, np.int32), 'frame_of_' + name: np.array(fk), 'size_' + name: np.int32(S),
                    'maxsize_' + name: np.int32(M if M else max(max(H, W) // 2, 1))})
        if S == 1024:
            rows = np.array(DIGEST_ROWS)
            out.update({'outrows_' + name: final[rows], 'rowsum_' + name: final.sum(1, dtype=np.int32), 'colsum_' + name: final.sum(0, dtype=np.int32)})
        else:
            out['out_' + name] = final
        if any(pad):
            assert crop.dtype == np.float32 and med is not None
            out['med_' + name] = med
            if 2 * size <= FLOAT_SIDE:
                out['float_' + name] = crop
        note = ''
        if mids is not None:
            got, n = middle_values(frame, box)
            assert np.array_equal(got, mids) and np.array_equal(R.median(R.first_blend(frame, box)[0]), med), (name, got, mids, med)
            parts = [first_differing_byte(a, b) for a, b in mids]
            assert (n % 2 == 1 and parts == [4] * 3) if extra[1] == 'odd' else (n % 2 == 0 and parts == [extra[1]] * 3), (name, n, parts)
            out['mid_' + name] = mids
            note = ' middle values %s median %s' % (mids.tolist(), med.tolist())
        names.append(name)
        print('%-14s frame %3d x %3d borders %-16s side %3d -> %4d attempt %d float err %.1e%s' % (name, H, W, pad, 2 * size, S, attempt, err, note))
    out['names'], out['digest_rows'] = np.array(names), np.array(DIGEST_ROWS, np.int32)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    print('wrote %s: %d bytes' % (OUT, size))


if __name__ == '__main__':
    main()

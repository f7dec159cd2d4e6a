"""CPU: the numpy restatement of the alignment crop against the fixture kat17 (written from the reference's own ffhq_cropping by
scripts/make_golden_face_crop_edges.py), and the preconditions that make each kat17 case the edge it is named for.

kat16 has six padded cases with an even pixel count whose two middle values are equal or part at pass 2 of the radix select, borders
well inside the frame, no dimension below 96, 9 k to 27 k values per histogram and resize ratios within 2.5 : 1.  kat17 adds
  MEDIAN    two middle values that first differ in byte 0, 1, 2, 3 of their bit patterns (the pass at which `select` parts the two
            prefixes and `hist` starts its second histogram) in all three channels, and an odd count (both ranks one element);
  eq_w/eq_h a border exactly as wide as the frame dimension it reflects (the widest valid one: border_src reaches the far edge);
  short_*   a padded dimension below the Gaussian's radius of 20 (reflect_any takes its modulo path, more than one period out);
  cap       a workspace whose padded frame exceeds 2^20 values, where the histogram grid is clamped to 256 blocks;
  r* / m200 crop sides 2, 6, 24 and 400 to out_size 5, 1, 1024 and 16, and side 24 under max_size 200, padded and unpadded.
As in test_cpu_face_crop: boxes and final bytes exactly, the float crop within one float32 ulp at 255 (2^-16), and a float64
evaluation of the same formulas on the same final bytes (the condition under which the GPU end-to-end bar of one level on at most
0.5 % of the bytes is fair).
"""
import os

import numpy as np
import pytest

from util import GOLDEN, golden
import face_crop_restatement as R

KAT = 'kat17_face_crop_edges.npz'
MEDIAN = {'med_p0': 0, 'med_p1': 1, 'med_p2': 2, 'med_p3': 3, 'med_odd': 'odd'}
# name: (H, W), borders (left, top, right, bottom), crop side, out_size, max_size
GEOMETRY = {
    'med_p0': ((200, 210), (10, 0, 0, 0), 48, 48, 105), 'med_p1': ((210, 200), (0, 10, 0, 0), 48, 48, 105),
    'med_p2': ((96, 118), (0, 0, 10, 0), 48, 48, 59), 'med_p3': ((118, 96), (0, 0, 0, 10), 48, 48, 59),
    'med_odd': ((95, 121), (10, 0, 0, 0), 48, 48, 60),
    'eq_w': ((44, 25), (25, 0, 0, 0), 40, 32, 22), 'eq_h': ((25, 44), (0, 0, 0, 25), 40, 32, 22),
    'short_top': ((9, 64), (0, 5, 0, 0), 14, 16, 32), 'short_right': ((64, 13), (0, 0, 6, 0), 18, 16, 32),
    'cap': ((300, 400), (37, 29, 0, 0), 300, 32, 200), 'r400to16': ((300, 400), (50, 44, 0, 56), 400, 16, 200),
    'r2to5_in': ((64, 80), (0, 0, 0, 0), 2, 5, 40), 'r2to5_pad': ((64, 80), (1, 0, 0, 0), 2, 5, 40),
    'r6to1_in': ((64, 80), (0, 0, 0, 0), 6, 1, 40), 'r6to1_pad': ((64, 80), (0, 0, 2, 1), 6, 1, 40),
    'r24to1024_in': ((64, 80), (0, 0, 0, 0), 24, 1024, 40), 'r24to1024_pad': ((64, 80), (4, 0, 0, 0), 24, 1024, 40),
    'm200_in': ((64, 80), (0, 0, 0, 0), 24, 32, 200), 'm200_pad': ((64, 80), (0, 0, 0, 7), 24, 32, 200),
}
NAMES = tuple(GEOMETRY)
PADDED = tuple(n for n in NAMES if any(GEOMETRY[n][1]))
NOPAD = tuple(n for n in NAMES if not any(GEOMETRY[n][1]))
FLOAT_SIDE = 160                          # the fixture holds the reference's float crop up to this crop side
PAIRS = ((2, 5), (6, 1), (24, 1024), (400, 16), (24, 32), (300, 32), (14, 16), (18, 16), (40, 32))


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


def case(kat, name):
    """frame, landmarks, out_size, max_size"""
    return kat['frame_' + str(kat['frame_of_' + name])], kat['lm_' + name], int(kat['size_' + name]), int(kat['maxsize_' + name])


def first_differing_byte(a, b):
    """Index (0 = most significant) of the first byte in which the bit patterns of two float32 differ; 4 if they are equal."""
    x = int(np.float32(a).view(np.uint32)) ^ int(np.float32(b).view(np.uint32))
    return 4 if x == 0 else 3 - (x.bit_length() - 1) // 8


def max_padded(n, M):
    """The largest padded dimension of a valid row on a frame dimension n with max_size M (facecrop.hip sizes the workspace by it):
    a box that leaves on one side adds a border of at most n (validity) and at most the box side 2 M; a box that leaves on both
    sides spans the padded dimension, 2 size <= 2 M."""
    return max(n + min(n, 2 * M), 2 * M)


def fixture_bytes_differ(kat, name, got):
    """Number of bytes of a [S,S,3] result that differ from the fixture's; a 1024 x 1024 output is held as full rows plus the row
    and column sums (any single wrong byte moves one of each)."""
    if 'out_' + name in kat.files:
        return int((got != kat['out_' + name]).sum())
    rows = kat['digest_rows']
    return int((got[rows] != kat['outrows_' + name]).sum() + (got.sum(1, dtype=np.int32) != kat['rowsum_' + name]).sum()
               + (got.sum(0, dtype=np.int32) != kat['colsum_' + name]).sum())


_float32 = {}


def restated_float(kat, name):
    """The restatement's float32 crop of a case, computed once."""
    if name not in _float32:
        frame, lm, _, _ = case(kat, name)
        _float32[name] = R.float_crop(frame, R.crop_box(lm)[0])
        _float32[name].setflags(write=False)
    return _float32[name]


def test_fixture_layout(kat):
    assert tuple(str(n) for n in kat['names']) == NAMES
    assert os.path.getsize(os.path.join(GOLDEN, KAT)) < 1000 * 1000
    for name, ((H, W), pad, side, S, M) in GEOMETRY.items():
        frame, lm, S_, M_ = case(kat, name)
        box = tuple(int(v) for v in kat['box_' + name])
        assert frame.shape == (H, W, 3) and frame.dtype == np.uint8 and lm.dtype == np.float32 and lm.shape == (68, 2)
        assert R.borders(box, H, W) == pad and box[2] - box[0] == side == box[3] - box[1] and (S_, M_) == (S, M)
        assert all(b <= d for b, d in zip(pad, (W, H, W, H))) and side // 2 <= M                    # every case is a valid row
        assert not any(pad) or all(b % 3 for b in pad if b) or name == 'short_right'               # see make_golden_face_crop.py
        assert ('float_' + name in kat.files) == (any(pad) and side <= FLOAT_SIDE) and ('med_' + name in kat.files) == any(pad)
        if S == 1024:
            assert kat['outrows_' + name].shape == (len(kat['digest_rows']), S, 3) and kat['rowsum_' + name].shape == (S, 3)
        else:
            assert kat['out_' + name].shape == (S, S, 3) and kat['out_' + name].dtype == np.uint8
    assert GEOMETRY['eq_w'][1][0] == GEOMETRY['eq_w'][0][1] and GEOMETRY['eq_h'][1][3] == GEOMETRY['eq_h'][0][0]
    (H, W), pad = GEOMETRY['short_top'][:2]
    assert H + pad[1] + pad[3] == 14 < R.RADIUS
    (H, W), pad = GEOMETRY['short_right'][:2]
    assert W + pad[0] + pad[2] == 19 < R.RADIUS
    assert GEOMETRY['m200_in'][4] > 16 * (GEOMETRY['m200_in'][2] // 2)


def test_cap_case_clamps_the_histogram_grid():
    """300 x 400 with max_size 200: PH = max(300 + min(300, 400), 400) = 600, PW = max(400 + min(400, 400), 400) = 800, so the
    launch is sized for 600 * 800 * 3 = 1 440 000 values > 2^20 = 1 048 576 and ceil(1 440 000 / 4096) = 352 blocks are clamped to
    256; the row itself has 329 * 437 * 3 = 431 319 values, 1 685 (1 686 as a multiple of 3) per block instead of 4 096."""
    (H, W), pad, _, _, M = GEOMETRY['cap']
    PH, PW = max_padded(H, M), max_padded(W, M)
    assert (PH, PW) == (600, 800) and PH * PW * 3 == 1440000 > 2 ** 20
    assert -(-PH * PW * 3 // 4096) == 352 > 256
    n3 = (H + pad[1] + pad[3]) * (W + pad[0] + pad[2]) * 3
    assert n3 == 329 * 437 * 3 and -(-n3 // 256) == 1685
    for name in NAMES:                                                # ... and no other case reaches the clamp
        (H, W), _, _, _, M = GEOMETRY[name]
        assert (max_padded(H, M) * max_padded(W, M) * 3 > 2 ** 20) == (name in ('cap', 'r400to16'))


@pytest.mark.parametrize('name', NAMES)
def test_restatement_reproduces_the_fixture(kat, name):
    frame, lm, S, _ = case(kat, name)
    box, size = R.crop_box(lm)
    assert box == tuple(int(v) for v in kat['box_' + name]) and 2 * size == GEOMETRY[name][2]
    mine = restated_float(kat, name)
    if 'float_' + name in kat.files:
        want = kat['float_' + name]
        err = float(np.abs(mine.astype(np.float64) - want).max())
        print('%s: float crop max |restatement - reference| = %.3e' % (name, err))
        assert mine.dtype == np.float32 and mine.shape == want.shape and err <= 2.0 ** -16
    if name in PADDED:
        med = R.median(R.first_blend(frame, box)[0])
        print('%s: median %s, the reference\'s %s' % (name, med.tolist(), kat['med_' + name].tolist()))
        assert np.array_equal(med, kat['med_' + name])
    assert fixture_bytes_differ(kat, name, R.resize_bicubic(mine.astype(np.uint8), S)) == 0


@pytest.mark.parametrize('name', PADDED)
def test_float64_evaluation_gives_the_same_bytes(kat, name):
    frame, lm, S, _ = case(kat, name)
    f32, f64 = restated_float(kat, name), R.float_crop(frame, R.crop_box(lm)[0], np.float64)
    print('%s: max |float32 - float64| = %.3e' % (name, float(np.abs(f32 - f64).max())))
    assert fixture_bytes_differ(kat, name, R.resize_bicubic(f64.astype(np.uint8), S)) == 0


@pytest.mark.parametrize('name', list(MEDIAN))
def test_median_preconditions(kat, name):
    """The two middle values of what np.median sees, re-derived from the restatement, first differ in the byte the case is named
    for in every channel (or the count is odd), they are the fixture's, and the crop holds pixels the median is blended into."""
    frame, lm, _, _ = case(kat, name)
    box, _ = R.crop_box(lm)
    blend, mask = R.first_blend(frame, box)
    flat = np.sort(blend.reshape(-1, 3), axis=0)
    n = flat.shape[0]
    mids = np.stack([flat[(n - 1) // 2], flat[n // 2]], 1)
    parts = [first_differing_byte(a, b) for a, b in mids]
    print('%s: n = %d, middle values %s part at byte %s, median %s' % (name, n, mids.tolist(), parts, kat['med_' + name].tolist()))
    assert np.array_equal(mids, kat['mid_' + name])
    if MEDIAN[name] == 'odd':
        assert n % 2 == 1 and blend.shape[0] % 2 == 1 and blend.shape[1] % 2 == 1 and parts == [4, 4, 4]
        assert np.array_equal(mids[:, 0], kat['med_' + name])
    else:
        assert n % 2 == 0 and parts == [MEDIAN[name]] * 3
        assert np.array_equal(((mids[:, 0] + mids[:, 1]) / np.float32(2)).astype(np.float32), kat['med_' + name])
    pl, pt = R.borders(box, *frame.shape[:2])[:2]
    inside = mask[box[1] + pt:box[3] + pt, box[0] + pl:box[2] + pl, 0]
    print('%s: %d of %d crop pixels have mask > 0' % (name, int((inside > 0).sum()), inside.size))
    assert inside.shape == (48, 48) and (inside > 0).sum() >= 48


def test_median_cases_part_at_every_pass_in_every_channel(kat):
    seen = {(first_differing_byte(a, b), c) for name in MEDIAN for c, (a, b) in enumerate(kat['mid_' + name])}
    assert seen == {(p, c) for p in (0, 1, 2, 3, 4) for c in range(3)}


@pytest.mark.parametrize('pair', PAIRS)
def test_resampler_equals_pillow(pair):
    """2 -> 5 (every window clipped on both sides), 6 -> 1 (one output: the whole line), 24 -> 1024 (the out_size bound), 400 -> 16
    (101 taps per output) and the other (crop side, out_size) pairs of kat17."""
    Image = pytest.importorskip('PIL.Image')
    n, S = pair
    rng = np.random.default_rng(1000 * n + S)
    img = rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
    img[: (n + 2) // 3] = (img[: (n + 2) // 3] > 127) * 255          # hard edges: the overshoot has to clip as Pillow's does
    want = np.array(Image.fromarray(img).resize((S, S), Image.BICUBIC))
    assert np.array_equal(R.resize_bicubic(img, S), want)

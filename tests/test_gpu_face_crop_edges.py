"""GPU: the alignment crop of csrc/facecrop.hip at the edges the fixture kat16 does not reach, against the fixture kat17 (written from
the reference's own ffhq_cropping; test_cpu_face_crop_edges lists the cases and proves each is the edge it is named for) and against
the numpy restatement (pinned to both fixtures and to Pillow on the CPU).  Two HIP runs are compared only where they must agree:
batch rows, a reused workspace, a side stream, a replayed graph.  Every test prints the figures it asserts on.

Bars, as in test_gpu_face_crop: boxes, unpadded rows, the composition resize(trunc(float crop)), the e4e tensor, reuse and replay
are exact.  The float crop of a padded row lies within PADDED_BOUND of the reference's float32 crop on the 0..255 scale (of the
restatement's where the fixture holds none: cap and r400to16, crop sides 300 and 400; the two agree at 0 wherever both exist):
4 x the largest deviation measured on an MI355X over the cases below.  Final bytes of a padded row: within one level, at most 0.5 %
of them different.

Measured on an MI355X, max |HIP - reference| of the float crop per padded case:
  med_p0 0  med_p1 0  med_p2 0  med_p3 0  med_odd 0  eq_w 0  eq_h 0  short_top 0  short_right 0  cap 0  r400to16 0  r2to5_pad 0
  r6to1_pad 0  r24to1024_pad 0  m200_pad 0
so the bound is 4 x 0 = 0: bit-exact, as on kat16 (the kernels keep scipy's order and numpy's float32 steps; nothing is reordered at
these edges either).  Final bytes: 0 of 135 246 compared bytes of the padded rows differ from the reference's.
"""
import numpy as np
import pytest
import torch

from util import golden
import face_crop_restatement as R
from test_cpu_face_crop_edges import GEOMETRY, KAT, MEDIAN, NAMES, NOPAD, PADDED, case, fixture_bytes_differ, max_padded, restated_float

pytestmark = pytest.mark.gpu

PADDED_BOUND = 4 * 0.0


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def FC():
    from stylegan_directions_face_reenactment_amd import face_crop
    return face_crop


def _dev(frame, lm):
    return torch.from_numpy(np.ascontiguousarray(frame)).unsqueeze(0).cuda(), torch.from_numpy(np.ascontiguousarray(lm)).unsqueeze(0).cuda()


@pytest.fixture(scope='module')
def runs(kat, FC):
    """One device run per fixture case: float crop, crop bytes, valid."""
    out = {}
    for name in NAMES:
        frame, lm, S, M = case(kat, name)
        flt, crops, valid = FC.padded_float(*_dev(frame, lm), out_size=S, max_size=M)
        out[name] = (None if flt[0] is None else flt[0].cpu().numpy(), crops[0].cpu().numpy(), valid.cpu().tolist())
    return out


def _landmarks(cx, cy, size):
    """68 points whose box has centre (cx, cy) after the size // 6 shift and half side `size`."""
    e, cy = size + 0.375, cy + size // 6
    lm = np.empty((68, 2), np.float32)
    lm[:, 0] = np.linspace(cx - e / 2, cx + e / 2, 68)
    lm[:, 1] = np.linspace(cy + e / 4, cy - e / 4, 68)
    return lm


def _level_bar(got, want):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), int((d > 0).sum()), d.size


# ---------------------------------------------------------------------------------------------------------------- fixture cases
@pytest.mark.parametrize('name', NAMES)
def test_float_stage(kat, runs, name):
    """Border, mask, Gaussian, both blends and the median against the reference's float32 crop; an unpadded row is the frame's bytes."""
    flt, _, valid = runs[name]
    stored = 'float_' + name in kat.files
    want = kat['float_' + name] if stored else restated_float(kat, name)
    assert valid == [1] and flt.shape == want.shape
    diff = np.abs(flt.astype(np.float64) - want)
    err = float(diff.max())
    print('%s: float crop %s max |HIP - %s| = %.3e (bound %.3e)' % (name, want.shape, 'reference' if stored else 'restatement', err, PADDED_BOUND))
    if name in NOPAD:
        assert want.dtype == np.uint8 and err == 0.0
        return
    frame, lm, _, _ = case(kat, name)
    box, _ = R.crop_box(lm)
    H, W, _ = frame.shape
    pad = R.borders(box, H, W)
    mask = R.feather_mask(H + pad[1] + pad[3], W + pad[0] + pad[2], pad)[box[1] + pad[1]:box[3] + pad[1], box[0] + pad[0]:box[2] + pad[0], 0]
    touched = mask > 0
    print('%s: %d of %d crop pixels carry the median (mask > 0), max deviation there %.3e; median of the reference %s' % (
        name, int(touched.sum()), touched.size, float(diff[touched].max()) if touched.any() else -1.0, kat['med_' + name].tolist()))
    if name in MEDIAN:
        print('%s: middle values %s' % (name, kat['mid_' + name].tolist()))
    # the outermost line of a padded side has mask 1: img + (median - img) there, the median within the two float32 roundings of that
    # form (2^-17 each below 256), so the device's select is also looked at directly
    full = mask >= 1
    off = float(np.abs(flt[full].astype(np.float64) - kat['med_' + name]).max()) if full.any() else -1.0
    print('%s: %d fully blended crop pixels lie within %.3e of the reference\'s median' % (name, int(full.sum()), off))
    assert touched.any() and full.any() and off <= 2.0 ** -16
    assert err <= PADDED_BOUND


@pytest.mark.parametrize('name', NAMES)
def test_composition_bit_exact(kat, runs, name):
    """The device's bytes are Pillow's resampler applied to the truncation of the same run's float crop."""
    flt, got, _ = runs[name]
    want = R.resize_bicubic(flt.astype(np.uint8), GEOMETRY[name][3])
    n = int((got != want).sum())
    print('%s: side %d -> %d, %d of %d bytes differ from resize(trunc(float crop))' % (name, GEOMETRY[name][2], GEOMETRY[name][3], n, want.size))
    assert got.shape == want.shape and n == 0


@pytest.mark.parametrize('name', NAMES)
def test_end_to_end(kat, runs, name):
    """Against the reference's final bytes: exact for a row inside the frame, one level on at most 0.5 % of the bytes for a padded
    one.  The 1024 x 1024 outputs are held as 28 full rows plus row and column sums: the rows meet the same bar, and since a byte one
    level off moves its row's and its column's sum by one, the sums may be off by no more than 0.5 % of the bytes in total."""
    _, got, _ = runs[name]
    if name in NOPAD:
        n = fixture_bytes_differ(kat, name, got)
        print('%s: %d bytes (or sums) differ from the reference' % (name, n))
        assert n == 0
        return
    if 'out_' + name in kat.files:
        worst, n, of = _level_bar(got, kat['out_' + name])
    else:
        worst, n, of = _level_bar(got[kat['digest_rows']], kat['outrows_' + name])
        for axis in (0, 1):
            off = int(np.abs(got.sum(axis, dtype=np.int64) - kat[('colsum_', 'rowsum_')[axis] + name]).sum())
            print('%s: sums along axis %d off by %d in total' % (name, axis, off))
            assert off <= 0.005 * got.size
    print('%s: max level difference %d, %d of %d bytes differ (%.3f %%)' % (name, worst, n, of, 100.0 * n / of))
    assert worst <= 1 and n <= 0.005 * of


# ---------------------------------------------------------------------------------------------------------------- validity
def contract_valid(lm, H, W, M):
    """`valid` as include/sgdfr.h states it: landmarks finite and within 1e6 (centre and extent), 1 <= size <= max_size, no border
    wider than the frame dimension it reflects, the padded frame within the workspace."""
    lm = np.asarray(lm, np.float32)
    if not np.isfinite(lm).all():
        return 0
    ext = max(lm[:, 0].max() - lm[:, 0].min(), lm[:, 1].max() - lm[:, 1].min())
    if not (np.abs(((lm.min(0) + lm.max(0)) / 2).round()).max() < 1e6 and ext < 1e6):
        return 0
    box, size = R.crop_box(lm)
    pl, pt, pr, pb = R.borders(box, H, W)
    return int(1 <= size <= M and pl <= W and pr <= W and pt <= H and pb <= H and H + pt + pb <= max_padded(H, M)
               and W + pl + pr <= max_padded(W, M))


def test_validity_table(kat, FC, runs):
    """One batch on the 44 x 25 frame with max_size 20: a left border of exactly W (valid) and of W + 1, size == max_size (valid)
    and max_size + 1, a NaN and an Inf landmark, an extent and a centre at the 1e6 bound, an ordinary row (valid)."""
    frame, lm_eq, S, _ = case(kat, 'eq_w')
    H, W, M = 44, 25, 20
    nan, inf, wide, far = (_landmarks(12, 22, 8) for _ in range(4))
    nan[5, 0], inf[7, 1] = np.nan, np.inf
    wide[:, 0] = np.linspace(0.0, 1e6, 68)
    far[:, 0] += np.float32(1e6 - 12)
    lms = np.stack([lm_eq, lm_eq - np.float32([1, 0]), _landmarks(12, 22, 20), _landmarks(12, 22, 21), nan, inf, wide, far, _landmarks(12, 22, 8)])
    what = ('pl == W', 'pl == W + 1', 'size == max_size', 'size == max_size + 1', 'NaN', 'Inf', 'extent 1e6', 'centre 1e6', 'ordinary')
    assert [R.borders(R.crop_box(l)[0], H, W)[0] for l in lms[:2]] == [W, W + 1] and [R.crop_box(l)[1] for l in lms[:4]] == [20, 20, 20, 21]
    assert float(wide[:, 0].max() - wide[:, 0].min()) == 1e6 and float((far[:, 0].min() + far[:, 0].max()) / 2) == 1e6
    want = [contract_valid(l, H, W, M) for l in lms]
    assert want == [1, 0, 1, 0, 0, 0, 0, 0, 1]
    frames = torch.from_numpy(np.stack([frame] * len(lms))).cuda()
    dl = torch.from_numpy(lms).cuda()
    (crops, x), valid = FC.crop_using_landmarks(frames, dl, out_size=S, max_size=M, as_tensor=True)
    boxes, sizes = FC.crop_boxes(dl)
    valid, boxes, sizes = valid.cpu().tolist(), boxes.cpu().numpy(), sizes.cpu().tolist()
    for i, w in enumerate(what):
        print('%-22s valid %d (contract %d) box %s size %d' % (w, valid[i], want[i], boxes[i].tolist(), sizes[i]))
    assert valid == want
    for i in range(len(lms)):
        if 4 <= i <= 7:                                               # not finite or beyond 1e6: the box is zeros
            assert not boxes[i].any() and sizes[i] == 0
        else:
            assert (tuple(int(v) for v in boxes[i]), sizes[i]) == R.crop_box(lms[i])
        if not want[i]:
            assert int(crops[i].max()) == 0 and float(x[i].abs().max()) == 0.0
            continue
        (one, x1), v1 = FC.crop_using_landmarks(*_dev(frame, lms[i]), out_size=S, max_size=M, as_tensor=True)
        n = int((one[0] != crops[i]).sum())
        print('%-22s %d bytes differ from its B = 1 run' % (what[i], n))
        assert v1.cpu().tolist() == [1] and n == 0 and torch.equal(x1[0], x[i]) and int(one.max()) > 0
    assert np.array_equal(crops[0].cpu().numpy(), runs['eq_w'][1])      # ... and max_size 20 or 22 makes no difference to a row


@pytest.mark.parametrize('name', ['eq_w', 'eq_h'])
def test_one_pixel_beyond_the_widest_border_is_invalid(kat, FC, name):
    frame, lm, S, M = case(kat, name)
    H, W, _ = frame.shape
    lm = lm + np.float32([-1, 0] if name == 'eq_w' else [0, 1])
    pad = R.borders(R.crop_box(lm)[0], H, W)
    assert pad == ((W + 1, 0, 0, 0) if name == 'eq_w' else (0, 0, 0, H + 1)) and contract_valid(lm, H, W, M) == 0
    (crops, x), valid = FC.crop_using_landmarks(*_dev(frame, lm), out_size=S, max_size=M, as_tensor=True)
    print('%s + 1: borders %s valid %s' % (name, pad, valid.cpu().tolist()))
    assert valid.cpu().tolist() == [0] and int(crops.max()) == 0 and float(x.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- state between calls
def _reuse_inputs(kat):
    """96 x 118 frames; call A: padded (right) / a box of max_size that leaves top and bottom / unpadded; call B: unpadded / an empty
    box / padded (top, another width)."""
    f = kat['frame_med_p2']
    frames = np.ascontiguousarray(np.stack([f, f[::-1], f[:, ::-1]]))
    H, W, M = 96, 118, 59
    a = np.stack([kat['lm_med_p2'], _landmarks(59, 48, 59), _landmarks(50, 50, 20)])
    b = np.stack([_landmarks(70, 40, 15), np.tile(np.float32([[40, 40]]), (68, 1)), _landmarks(60, 10, 24)])
    assert [R.borders(R.crop_box(l)[0], H, W) for l in a] == [(0, 0, 10, 0), (0, 11, 0, 11), (0, 0, 0, 0)]
    assert [R.borders(R.crop_box(l)[0], H, W) for l in b[::2]] == [(0, 0, 0, 0), (0, 14, 0, 0)] and R.crop_box(b[1])[1] == 0
    return frames, a, b, M


def test_workspace_reuse(kat, FC):
    """Call B on the workspace call A left behind equals call B on a workspace that was dropped and refilled with 0xFF (NaN in the
    float areas) or 0x00: nothing but the cleared state survives a call."""
    frames, a, b, M = _reuse_inputs(kat)
    dev = torch.from_numpy(frames).cuda()
    la, lb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    FC.clear_workspaces()
    (ca, xa), va = FC.crop_using_landmarks(dev, la, out_size=32, max_size=M, as_tensor=True)
    (cb, xb), vb = FC.crop_using_landmarks(dev, lb, out_size=32, max_size=M, as_tensor=True)
    print('reuse: valid A %s B %s' % (va.cpu().tolist(), vb.cpu().tolist()))
    assert va.cpu().tolist() == [1, 1, 1] and vb.cpu().tolist() == [1, 0, 1]
    for fill in (None, 0xFF, 0x00):
        FC.clear_workspaces()
        if fill is not None:
            FC._workspace(3, 96, 118, M, dev.device)[0].fill_(fill)
        (c, x), v = FC.crop_using_landmarks(dev, lb, out_size=32, max_size=M, as_tensor=True)
        n = int((c != cb).sum())
        print('reuse: after A vs a new workspace filled with %s: %d bytes differ, e4e equal %s' % (fill, n, torch.equal(x, xb)))
        assert n == 0 and torch.equal(x, xb) and torch.equal(v, vb)
    got = cb.cpu().numpy()
    assert np.array_equal(got[0], R.crop_using_landmarks(frames[0], b[0], 32)) and not got[1].any()
    worst, n, of = _level_bar(got[2], R.crop_using_landmarks(frames[2], b[2], 32))
    print('reuse: padded row of B against the restatement: max level difference %d, %d of %d bytes' % (worst, n, of))
    assert worst <= 1 and n <= 0.005 * of


def test_side_stream_and_graph_replay(kat, FC):
    """The crop on a non-default stream, and one captured graph replayed with landmarks that make its row padded, unpadded, invalid
    and padded again: each replay equals the eager run for those landmarks (every decision is taken on the device)."""
    frames, a, b, M = _reuse_inputs(kat)
    frame = torch.from_numpy(frames[:1]).cuda()
    lms = [torch.from_numpy(l[None]).cuda() for l in (a[0], a[2], b[1], b[2])]
    want_valid = [1, 1, 0, 1]
    eager = [FC.crop_using_landmarks(frame, l, out_size=32, max_size=M, as_tensor=True) for l in lms]
    torch.cuda.synchronize()
    assert [int(v[0]) for _, v in eager] == want_valid
    assert np.array_equal(eager[1][0][0][0].cpu().numpy(), R.crop_using_landmarks(frames[0], a[2], 32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = [FC.crop_using_landmarks(frame, l, out_size=32, max_size=M, as_tensor=True) for l in lms]
    side.synchronize()
    for k, (((c, x), v), ((c0, x0), v0)) in enumerate(zip(other, eager)):
        print('side stream, landmarks %d: %d bytes differ' % (k, int((c != c0).sum())))
        assert torch.equal(c, c0) and torch.equal(x, x0) and torch.equal(v, v0)
    lm = lms[0].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        (c, x), v = FC.crop_using_landmarks(frame, lm, out_size=32, max_size=M, as_tensor=True)
    for k in range(len(lms)):
        lm.copy_(lms[k])
        c.fill_(7), x.fill_(7.0), v.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        (c0, x0), v0 = eager[k]
        print('replay %d: valid %s, %d bytes differ from the eager run' % (k, v.cpu().tolist(), int((c != c0).sum())))
        assert torch.equal(c, c0) and torch.equal(x, x0) and torch.equal(v, v0)

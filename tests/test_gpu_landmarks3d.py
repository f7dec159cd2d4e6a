"""GPU: flip_input, the Gaussian draw and the 3D landmark type on the HIP kernels of csrc/fan.hip and csrc/fandepth.hip against the
fixture kat21 (written from the reference's own flip, draw_gaussian and ResNetDepth) and against the restatement on the CPU
(tests/fan3d_restatement.py, itself pinned to the fixture by test_cpu_landmarks3d).  Never against another run of the HIP code,
except where two HIP runs must agree (the default argument, rows).

Bars: the flip sum and the drawn maps bit for bit; heatmaps, every ResNetDepth tap and the depths within 8 x the reference's own
max |fp32 - fp64| on that tensor (dev_* of the fixture: the same fp32 accumulation in another order), z within that bar times the
row's factor; arg-max, pts, pts_img (x, y) and boxes exactly equal (the fixture's script asserts margins of 16 x dev on every
decision and 1e-3 pixels on every truncation).  Every test prints the figures it asserts on.
"""
import copy

import numpy as np
import pytest
import torch

from util import S, golden
import fan_restatement as R
import fan3d_restatement as R3
from test_cpu_landmarks3d import CASES, KAT, MODES

pytestmark = pytest.mark.gpu

BAR = 8.0


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def fan(kat):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    m = L.FAN(4)
    m.load_state_dict(S.synthetic_fan_state(int(kat['seed'])), strict=True)
    return m.cuda().eval()


@pytest.fixture(scope='module')
def state(kat):
    return S.synthetic_fan_depth_state(int(kat['depth_seed']))


@pytest.fixture(scope='module')
def depth_net(state):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    m = L.ResNetDepth()
    m.load_state_dict(state, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope='module')
def ref_b(kat, state):
    """Case b (two rows): images, faces, the fp64 crop, the reference's maps (restated) and the fp64 taps of the restatement on the CPU."""
    x, faces = R3.case_inputs(S, int(kat['seed']), 'b')
    crop = R.crop(x.double(), faces)
    maps = R3.draw(torch.from_numpy(kat['pts_plain_b']))
    with torch.no_grad():
        taps = R3.depth_network(state, crop, maps.double())
    return x, faces, crop, maps, taps


def _taps_of(depth, views):
    return {'stem': views['stem'], 'pool': views['pool'], 'layer': views['layer'], 'feat': views['feat'], 'depth': depth}


@pytest.mark.parametrize('B', [1, 3])
def test_flip_add_is_the_reference_sum_bit_for_bit(kat, B):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    hm2 = S.counter_tensor(int(kat['seed']), 'fan3d.flip.hm2', (2, 68, 64, 64)) if B == 1 else S.counter_tensor(7, 'fan3d.flip.B3', (6, 68, 64, 64))
    got = L.flip_add(hm2.cuda()).cpu()
    n = int((got != R3.flip_add(hm2)).sum())
    print('flip_add B = %d: %d of %d values differ from the restatement' % (B, n, got.numel()))
    assert n == 0 and tuple(got.shape) == (B, 68, 64, 64)
    if B == 1:
        assert np.array_equal(got[0, :, ::8, ::8].numpy(), kat['flipadd_sub']) and np.array_equal(got[0].double().sum(2).numpy(), kat['flipadd_rowsum'])


def test_draw_is_draw_gaussian_bit_for_bit(kat):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    edge = R3.edge_points()
    R3.check_maps(kat, 'edge', L.draw(edge.cuda()), 'HIP B = 4')
    one = L.draw(edge[2:3].cuda()).cpu()                                            # B = 1
    assert torch.equal(one, R3.draw(edge[2:3]))
    R3.check_maps(kat, 'plain_a', L.draw(torch.from_numpy(kat['pts_plain_a']).cuda()), 'HIP B = 1')
    three = torch.cat([torch.from_numpy(kat['pts_flip_b']), torch.from_numpy(kat['pts_flip_a'])])
    got = L.draw(three.cuda())                                                      # B = 3
    R3.check_maps(kat, 'flip_b', got[:2], 'HIP B = 3')
    R3.check_maps(kat, 'flip_a', got[2:], 'HIP B = 3')
    wild = torch.tensor([[float('nan'), 5.0], [5.0, float('nan')], [float('inf'), 5.0], [5.0, -float('inf')], [3e9, 3e9], [-3e9, 7.0],
                         [7.0, 1e30]]).repeat(10, 1)[:68].view(1, 68, 2)
    assert float(L.draw(wild.cuda()).abs().max()) == 0.0                            # nothing drawn, nothing written out of bounds


def test_depth_network_taps_within_the_reference_fp32_deviation(kat, depth_net, ref_b):
    """B = 1 (row 0 of case b) with the debug taps: every tap against the fixture's checksums and, element by element, against the
    fp64 restatement.  The stem is the conv whose last K chunk has 7 valid rows (K = 3479) and which gathers from two tensors; the
    depths come from the linear layer whose second channel tile has 4 valid columns (N = 68)."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces, crop, maps, taps64 = ref_b
    depth, views = L.depth_network(depth_net, crop[:1].float().cuda(), maps[:1].cuda(), debug=True)
    torch.cuda.synchronize()
    fails = []
    for (tap, t), (_, want) in zip(R3.tap_list(_taps_of(depth, views)), R3.tap_list(taps64)):
        dev = float(kat['dev_%s_plain_b' % tap])
        err = float((t.double().cpu() - want[:1]).abs().max())
        got_sum, want_sum = R3.tap_checksum(t), kat['tap_%s_plain_b' % tap]
        e_win = float(np.abs(got_sum[2:] - want_sum[2:]).max())                  # the 64 stored values are row 0's
        print('tap %-7s max |HIP - fp64| %.3e = %.2f x the reference fp32 deviation %.3e; stored window %.2f x   bar %.0f x' % (
            tap, err, err / dev, dev, e_win / dev, BAR))
        if max(err, e_win) > BAR * dev:
            fails.append((tap, err / dev, e_win / dev))
    assert not fails, fails
    assert float(views['stem'].abs().max()) > 0.1 and float(depth.abs().max()) > 1.0


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return sum('fandepth_conv_kernel' in n for n in names), sum('fandepth_finish_kernel' in n for n in names)


def test_depth_rows_are_independent_across_batch_sizes_and_plans(kat, depth_net, ref_b):
    """B = 1, 2, 3 and 17 from the two rows of case b, repeated and permuted: per row the depths stay within the bar.  The split-K
    plan follows the row count: the number of convs sliced over K (a finish launch follows each) falls as B grows."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces, crop, maps, taps64 = ref_b
    want = taps64['depth']
    bar = BAR * float(kat['dev_depth_plain_b'])
    c32, m32 = crop.float().cuda(), maps.cuda()
    counts = {}
    for B in (1, 2, 3, 17):
        rows = {1: [1], 2: [0, 1], 3: [1, 0, 1]}.get(B) or [(3 * i + 1) % 2 for i in range(B)]
        cb, mb = c32[rows].contiguous(), m32[rows].contiguous()
        depth = L.depth_network(depth_net, cb, mb)
        err = float((depth.double().cpu() - want[rows]).abs().max())
        counts[B] = _launches(lambda: L.depth_network(depth_net, cb, mb))
        print('B = %2d rows %s...: max |HIP - fp64| %.3e = %.2f x dev   bar %.0f x; %d convs, %d of them sliced over K' % (
            B, rows[:4], err, err / float(kat['dev_depth_plain_b']), BAR, counts[B][0], counts[B][1]))
        assert err <= bar
    assert all(c[0] == 156 for c in counts.values()), counts      # 155 convs and the linear layer
    assert counts[1][1] > counts[3][1] > counts[17][1] > 0, counts


@pytest.mark.parametrize('name', ['a', 'b'])
def test_flip_input_landmarks_equal_the_fixture(kat, fan, name):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces = R3.case_inputs(S, int(kat['seed']), name)
    pts_img, pts, hm = L.get_landmarks(fan, x.cuda(), faces.cuda(), flip_input=True)
    tag = 'flip_' + name
    dev = float(kat['dev_heatmaps_' + tag])
    h = hm.double().cpu()
    B = h.shape[0]
    idx = torch.from_numpy(kat['argmax_' + tag])
    flat = h.reshape(B, 68, -1)
    e_full = float((h[0, [int(j) for j in kat['full']]] - torch.from_numpy(kat['heatmaps_full_' + tag])).abs().max())
    e_top = float((flat.gather(2, idx.unsqueeze(2)).squeeze(2) - torch.from_numpy(kat['top2_' + tag])[..., 0]).abs().max())
    nbh = torch.from_numpy(kat['nbh_' + tag])
    pad = torch.nn.functional.pad(h, (1, 1, 1, 1), value=float('nan'))
    e_nbh = 0.0
    for b in range(B):
        for j in range(68):
            py, px = int(idx[b, j]) // 64, int(idx[b, j]) % 64
            d = (pad[b, j, py:py + 3, px:px + 3] - nbh[b, j]).abs()
            e_nbh = max(e_nbh, float(d[~torch.isnan(nbh[b, j])].max()))
    print('flip case %s: full maps %.2f x, maxima %.2f x, neighbourhoods %.2f x the reference fp32 deviation %.3e   bar %.0f x' % (
        name, e_full / dev, e_top / dev, e_nbh / dev, dev, BAR))
    assert max(e_full, e_top, e_nbh) <= BAR * dev
    assert torch.equal(flat.argmax(2), idx)
    for what, got in (('pts', pts), ('pts_img', pts_img), ('boxes', L.kpt68_boxes(pts_img))):
        n = int((got.cpu() != torch.from_numpy(kat['%s_%s' % (what, tag)])).sum())
        print('flip case %s: %s differ in %d of %d values' % (name, what, n, got.numel()))
        assert n == 0


def test_flip_input_false_is_the_call_without_the_argument(kat, fan):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces = R3.case_inputs(S, int(kat['seed']), 'b')
    a = L.get_landmarks(fan, x.cuda(), faces.cuda())
    b = L.get_landmarks(fan, x.cuda(), faces.cuda(), flip_input=False)
    c = L.get_landmarks(fan, x.cuda(), faces.cuda(), '255', False)
    assert all(torch.equal(u, v) and torch.equal(u, w) for u, v, w in zip(a, b, c))
    assert np.array_equal(a[0].cpu().numpy(), kat['pts_img_plain_b']) and np.array_equal(a[1].cpu().numpy(), kat['pts_plain_b'])


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('name', ['a', 'c'])
def test_landmarks_3d_end_to_end(kat, fan, depth_net, name, flip):
    """B = 1 (case a) and the B = 2 case c whose scales differ by two, with and without flip, under the sync debug mode: x and y
    exactly the fixture's, z within the depth bar times the row's factor."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces = R3.case_inputs(S, int(kat['seed']), name)
    xd, fd = x.cuda(), faces.cuda()
    fan.packed(), depth_net.packed()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        pts_img3, pts, hm = L.get_landmarks_3d(fan, depth_net, xd, fd, flip_input=flip)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    tag = '%s_%s' % ('flip' if flip else 'plain', name)
    want = torch.from_numpy(kat['pts_img3_' + tag])
    got = pts_img3.double().cpu()
    assert tuple(pts_img3.shape) == (x.shape[0], 68, 3) and pts_img3.dtype == torch.float32
    n_xy = int((got[..., :2] != want[..., :2]).sum())
    zf = torch.from_numpy(kat['zfac_' + name]).double().view(-1, 1)
    dev = float(kat['dev_depth_' + tag])
    ez = float(((got[..., 2] - want[..., 2]).abs() / zf).max())
    print('3D case %s: x, y differ in %d values; z / factor off by %.3e = %.2f x the reference fp32 deviation %.3e   bar %.0f x' % (
        tag, n_xy, ez, ez / dev, dev, BAR))
    assert n_xy == 0 and np.array_equal(pts.cpu().numpy(), kat['pts_' + tag])
    assert ez <= BAR * dev and float(want[..., 2].abs().max()) > 1.0
    two = L.get_landmarks(fan, xd, fd, flip_input=flip)
    assert torch.equal(two[0], pts_img3[..., :2]) and torch.equal(two[2], hm)


def test_detect_landmarks_with_the_depth_network(kat, fan, depth_net):
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    det = FD.S3FD()
    det.load_state_dict(S.synthetic_s3fd_state(20261018), strict=True)
    det = det.cuda().eval()
    x, _ = R3.case_inputs(S, int(kat['seed']), 'c')
    p2, b2, has2 = FD.detect_landmarks(det, fan, x.cuda())
    p3, b3, has3 = FD.detect_landmarks(det, fan, x.cuda(), depth_net=depth_net)
    assert tuple(p3.shape) == (x.shape[0], 68, 3) and tuple(p2.shape) == (x.shape[0], 68, 2)
    assert torch.equal(p3[..., :2], p2) and torch.equal(b3, b2) and torch.equal(has3, has2)


def test_pack_cache_and_refused_modes(kat, fan, depth_net, ref_b):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces, crop, maps, _ = ref_b
    c, m = crop[:1].float().cuda(), maps[:1].cuda()
    d = copy.deepcopy(depth_net)
    assert d._pack is None
    h0 = d(c, m)
    p0 = d.packed()
    d(c, m)
    assert d.packed() is p0                                  # no change, no rebuild
    with torch.no_grad():
        d.fc.bias.add_(1.0)                                  # bumps the version counter
    h1 = d(c, m)
    assert d.packed() is not p0
    shift = (h1 - h0).double()
    print('pack: depths moved by %.6f .. %.6f after fc.bias += 1' % (float(shift.min()), float(shift.max())))
    assert float((shift - 1.0).abs().max()) <= 1e-4
    d.train()
    with pytest.raises(RuntimeError, match='eval mode only'):
        d(c, m)
    d.eval()
    d.conv1.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='forward only'):
        d(c, m)
    with pytest.raises(ValueError, match='unsupported batch'):
        L.get_landmarks(fan, torch.zeros(129, 3, 8, 8).cuda(), torch.zeros(129, 4), flip_input=True)      # 258 rows in the network

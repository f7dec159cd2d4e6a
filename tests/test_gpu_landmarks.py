"""GPU: the landmark head on the HIP kernels of csrc/fan.hip against the fixture kat13 (written from the reference's own FAN(4),
get_preds_fromhm and transform) and against the fp64 restatement on the CPU (tests/fan_restatement.py, itself pinned to the fixture
by test_cpu_landmarks).  Never against another run of the HIP code, except where two HIP runs must agree (rows, replays).

Bars: heatmaps and every debug tap within 8 x the reference's own max |fp32 - fp64| on that tensor (dev_* of the fixture: the same
fp32 accumulation in another order); the front within 8 x the deviation of torch's own fp32 F.interpolate from fp64; arg-max, pts,
pts_img and boxes exactly equal (the fixture's script asserts margins of 16 x dev_heatmaps on every decision and 1e-3 pixels on
every truncation).  Every test prints the figures it asserts on.
"""
import copy

import numpy as np
import pytest
import torch

from util import S, golden
import fan_restatement as R
from test_cpu_landmarks import KAT, check_against_fixture

pytestmark = pytest.mark.gpu

BAR = 8.0


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def state(kat):
    return S.synthetic_fan_state(int(kat['seed']))


@pytest.fixture(scope='module')
def fan(state):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    m = L.FAN(4)
    m.load_state_dict(state, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope='module')
def ref64(kat, state):
    """Per case: images, faces, the fp64 crop and the fp64 taps of the restatement on the CPU."""
    out = {}
    for name in R.CASES:
        x, faces = R.fixture_inputs(S, int(kat['seed']), name)
        crop = R.crop(x.double(), faces)
        with torch.no_grad():
            taps = R.network(state, crop)
        out[name] = (x, faces, crop, taps)
    return out


def _views_as_taps(v):
    return {'stem': v['stem'], 'conv4': v['conv4'], 'hg': v['hg'], 'heatmaps': v['heatmaps']}


@pytest.mark.parametrize('name', list(R.CASES))
def test_heatmaps_and_every_tap_within_the_reference_fp32_deviation(kat, fan, ref64, name):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces, _, taps64 = ref64[name]
    pts_img, pts, hm, boxes, views = L.run_debug(fan, x.cuda(), faces.cuda())
    torch.cuda.synchronize()
    assert torch.equal(views['heatmaps'][-1], hm)
    figures = []
    for (tap, t), (_, want) in zip(R.tap_list(_views_as_taps(views)), R.tap_list(taps64)):
        dev = float(kat['dev_%s_%s' % (tap, name)])
        err = float((t.double().cpu() - want).abs().max())
        figures.append((tap, err, dev))
        print('case %s tap %-10s max |HIP - fp64| %.3e = %.2f x the reference fp32 deviation %.3e   bar %.0f x' % (name, tap, err, err / dev,
                                                                                                                  dev, BAR))
    first = next(((tap, err / dev) for tap, err, dev in figures if err > BAR * dev), None)
    assert first is None, 'first tap beyond the bar: %s at %.2f x' % first
    dec = {'idx': hm.reshape(hm.shape[0], 68, -1).argmax(2), 'pts': pts, 'pts_img': pts_img, 'boxes': boxes}
    check_against_fixture(kat, name, _views_as_taps(views), dec, BAR * float(kat['dev_heatmaps_' + name]), None, 'HIP')


def test_decode_kernel_is_exact(kat, ref64):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    for name in R.CASES:
        _, faces, _, taps64 = ref64[name]
        hm32 = taps64['heatmaps'][-1].float()
        assert torch.equal(hm32.reshape(hm32.shape[0], 68, -1).argmax(2), torch.from_numpy(kat['argmax_' + name]))
        pts_img, pts, boxes = L.decode(hm32.cuda(), faces.cuda())
        for what, got in (('pts', pts), ('pts_img', pts_img), ('boxes', boxes)):
            n = int((got.cpu() != torch.from_numpy(kat['%s_%s' % (what, name)])).sum())
            print('decode case %s: %s differ in %d values' % (name, what, n))
            assert n == 0
        assert torch.equal(L.kpt68_boxes(pts_img), boxes)
    hm, faces = R.handmade_heatmaps()
    want = R.decode(hm, faces)
    pts_img, pts, boxes = L.decode(hm.cuda(), faces.tolist())          # numbers are accepted as well
    for what, got in (('pts', pts), ('pts_img', pts_img), ('boxes', boxes)):
        n = int((got.cpu() != want[what]).sum())
        print('decode hand-made: %s differ in %d values' % (what, n))
        assert n == 0


@pytest.mark.parametrize('input_range', ['255', 'gan'])
@pytest.mark.parametrize('name', list(R.CASES))
def test_front_kernel_against_interpolate(kat, name, input_range):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces = R.fixture_inputs(S, int(kat['seed']), name)
    if input_range == 'gan':
        x = R.to_gan(x)
    want = R.crop(x.double(), faces, input_range)
    stock = R.crop(x.cuda(), faces, input_range).double().cpu()          # torch's own fp32 on the device
    got = L.crop(x.cuda(), faces.cuda(), input_range).double().cpu()
    dev, err = float((stock - want).abs().max()), float((got - want).abs().max())
    print('front case %s range %s: max |HIP - fp64| %.3e, torch fp32 %.3e (%.2f x)   bar %.0f x' % (name, input_range, err, dev, err / dev, BAR))
    assert dev > 0 and float(want.max()) > 0.5
    assert err <= BAR * dev


@pytest.mark.parametrize('name', list(R.CASES))
def test_end_to_end_landmarks_equal_the_fixture(kat, fan, name):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces = R.fixture_inputs(S, int(kat['seed']), name)
    pts_img, pts, hm = L.get_landmarks(fan, x.cuda(), faces.cuda(), input_range='255')
    boxes = L.kpt68_boxes(pts_img)
    assert tuple(hm.shape) == (x.shape[0], 68, 64, 64) and pts_img.dtype == torch.float32
    for what, got in (('pts_img', pts_img), ('pts', pts), ('boxes', boxes)):
        n = int((got.cpu() != torch.from_numpy(kat['%s_%s' % (what, name)])).sum())
        print('end to end case %s: %s differ in %d of %d values' % (name, what, n, got.numel()))
        assert n == 0
    # a score column and host numbers change nothing
    five = torch.cat([faces, torch.full((faces.shape[0], 1), 0.999)], 1)
    again = L.get_landmarks(fan, x.cuda(), five.tolist())
    assert torch.equal(again[0], pts_img) and torch.equal(again[2], hm)


def _finish_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return sum('fan_conv_kernel' in n for n in names), sum('fan_finish_kernel' in n for n in names)


def test_rows_are_independent_across_batch_sizes_and_plans(kat, fan, ref64):
    """B = 1, 3, 16, 17 from the rows of case b, repeated and permuted: per row the heatmaps stay within the bar of the first test and
    the landmarks equal the fixture's.  The split-K plan follows the row count: at B = 1 most convs are sliced over K (a finish
    launch follows each), at B = 16 / 17 the 64 x 64 and 128 x 128 layers keep K in one slice and apply their epilogue themselves."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    x, faces, _, taps64 = ref64['b']
    want = taps64['heatmaps'][-1]
    bar = BAR * float(kat['dev_heatmaps_b'])
    counts = {}
    for B in (1, 3, 16, 17):
        rows = [(3 * i + 1) % 2 if B > 1 else 1 for i in range(B)]
        if B == 3:
            rows = [1, 0, 1]
        xb, fb = x[rows].cuda(), faces[rows].cuda()
        pts_img, pts, hm = L.get_landmarks(fan, xb, fb)
        err = float((hm.double().cpu() - want[rows]).abs().max())
        counts[B] = _finish_launches(lambda: L.get_landmarks(fan, xb, fb))
        print('B = %2d rows %s...: max |HIP - fp64| %.3e   bar %.3e; %d convs, %d of them sliced over K' % (
            B, rows[:4], err, bar, counts[B][0], counts[B][1]))
        assert err <= bar
        assert np.array_equal(pts_img.cpu().numpy(), kat['pts_img_b'][rows]) and np.array_equal(pts.cpu().numpy(), kat['pts_b'][rows])
        assert np.array_equal(L.kpt68_boxes(pts_img).cpu().numpy(), kat['boxes_b'][rows])
    assert all(c[0] == 191 for c in counts.values()), counts      # 194 convs, bl + al in one launch
    assert counts[1][1] > counts[3][1] > counts[17][1] > 0, counts
    assert counts[1][1] >= 150 and counts[17][1] <= 120, counts


def test_chain_into_deca_encode_and_graph_capture(kat, fan):
    """get_landmarks('gan') -> kpt68_boxes -> deca.crop_matrix -> deca.encode equals deca.encode fed with the fixture's boxes; the
    chain is then captured on one stream (nothing in it synchronises) and two replays give identical output."""
    from stylegan_directions_face_reenactment_amd import deca as D, landmarks as L
    x, faces = R.fixture_inputs(S, int(kat['seed']), 'b')
    xg = R.to_gan(x).cuda()
    fd = faces.cuda()
    E = D.ResnetEncoder()
    E.load_state_dict(S.synthetic_deca_encoder_state(20261101), strict=True)
    E = E.cuda().eval()

    def chain():
        pts_img, _, _ = L.get_landmarks(fan, xg, fd, input_range='gan')
        boxes = L.kpt68_boxes(pts_img)
        code = D.encode(E, xg, D.crop_matrix(boxes, xg.shape[2:]))
        return boxes, torch.cat([code[k].flatten(1) for k in ('shape', 'tex', 'exp', 'pose', 'cam', 'light')], 1)

    with torch.no_grad():
        boxes, params = chain()                                       # eager warm-up: both packs are built here
        want_boxes = torch.from_numpy(kat['boxes_b'])
        print('chain: boxes differ from the fixture in %d values' % int((boxes.cpu() != want_boxes).sum()))
        assert torch.equal(boxes.cpu(), want_boxes)
        code = D.encode(E, xg, D.crop_matrix(want_boxes.cuda(), xg.shape[2:]))
        direct = torch.cat([code[k].flatten(1) for k in ('shape', 'tex', 'exp', 'pose', 'cam', 'light')], 1)
        assert torch.equal(params, direct) and float(params.abs().max()) > 0.05
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gb, gp = chain()
        outs = []
        for _ in range(2):
            gb.zero_(), gp.zero_()
            g.replay()
            torch.cuda.synchronize()
            outs.append((gb.clone(), gp.clone()))
    print('chain: replay 1 against eager differs in %d parameters, replay 2 against replay 1 in %d' % (
        int((outs[0][1] != params).sum()), int((outs[1][1] != outs[0][1]).sum())))
    assert torch.equal(outs[0][0], boxes) and torch.equal(outs[0][1], params)
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])


def test_pack_is_rebuilt_after_an_in_place_edit_and_only_then(kat, fan):
    from stylegan_directions_face_reenactment_amd import landmarks as L
    f = copy.deepcopy(fan)
    assert f._pack is None
    crop = S.counter_tensor(5, 'fan.pack.crop', (1, 3, 256, 256), 0.5, 0.25).clamp(0, 1).cuda()
    h0 = f(crop)
    p0 = f.packed()
    assert f.packed() is p0
    f(crop)
    assert f.packed() is p0                                  # no change, no rebuild
    with torch.no_grad():
        f.l3.bias.add_(1.0)                                  # bumps the version counter
    h1 = f(crop)
    assert f.packed() is not p0
    shift = (h1 - h0).double()
    print('pack: heatmaps moved by %.6f .. %.6f after l3.bias += 1' % (float(shift.min()), float(shift.max())))
    assert float((shift - 1.0).abs().max()) <= 1e-5
    p1 = f.packed()
    f.l3.bias.data.sub_(1.0)                                 # through .data: no version bump, the pack is stale until invalidated
    assert f.packed() is p1
    f.invalidate_packs()
    h2 = f(crop)
    assert f.packed() is not p1 and float((h2 - h0).abs().max()) <= 1e-5

"""GPU: the DECA coefficient encoder (csrc/deca.hip) and the FAN landmark detector (csrc/fan.hip) on the sides that their own
modules (test_gpu_deca, test_gpu_landmarks) do not reach: crop matrices with rotation, shear, mirroring, strong scaling and no
inverse (an exactly singular one enters the adjoint's all-candidates fallback); the |R20| > 0.998 and zero-pose branches of the
angle kernel on the device; 48 rows in one launch, where most convs keep K in one slice and apply their epilogue themselves, with
copies of a row landing in different 64-pixel tiles; FAN windows wholly inside a large image, far smaller than 256, wholly
outside, on a strip, many times the image, and a box without extent.  Every figure is taken against the fp64 restatements on the
CPU (deca_restatement, fan_restatement), never against another run of the HIP code, except where two HIP results must be
bit-equal (copies of one row in one launch).

Bars are those of the two modules for the same quantities.  DECA front and adjoint: 8 x the deviation of torch's own fp32
grid_sample from fp64 (floor 1e-6 / 1e-6 of the largest gradient element), exactly zero where |x| > 1.  Angles 1e-2 degrees, the
zero pose and the z of the two gimbal rows exactly zero.  DECA stages 1e-4 of the maximum, at most 1e-5 of the decisions differing,
dL/dx under the HIP decisions 1e-4.  FAN front 8 x the deviation of torch's fp32 F.interpolate from fp64; heatmaps 8 x the larger
of kat13's two dev_heatmaps; arg-max, pts, pts_img and boxes equal to the decode of the fp64 heatmaps on every landmark the
fixture script's rule calls safe (margins of 16 x that bar, coordinates 1e-3 from an integer), at most 8 of 68 unsafe per row.

Which plan ran is proven by counting `*_conv_kernel` / `*_finish_kernel` launches with torch.profiler against the plan rule written
once below in plain Python (`slices`); test_cpu_deca checks without a GPU that it reproduces DESIGN 4.15's and 4.16's counts.

Not yet run on an MI355X: no figure of this module and no wall time has been recorded (the fp64 side was checked on the CPU: the
windows of GEO_WINDOWS, 3, 3 + 3, 0, 3, 7 and 4 unsafe landmarks for the six FAN geometries, crop maxima >= 0.9 and gradient
maxima of 1.4 .. 47 for the DECA front geometries; the fp64 work is 3 DECA rows and 9 FAN rows, about 10 s).
"""
import copy

import pytest
import torch

from util import S, SEED, golden
import deca_restatement as RD
import fan_restatement as RF
import test_gpu_deca as TD
from test_cpu_landmarks import KAT

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 3, 16, 17, 48)


# ---------------------------------------------------------------------------------------------------------------- the plan rule
def slices(R, N, Ho, Wo, K):
    """K slices of one conv launch: 64 x 64 output tiles over (R Ho Wo pixels, N channels), K in chunks of 16;
    S = clamp(min(512 // tiles, chunks // 8), 1, 32), then re-derived through the chunks per slice."""
    tiles = -(-(R * Ho * Wo) // 64) * -(-N // 64)
    chunks = -(-K // 16)
    S_ = max(1, min(min(512 // tiles, chunks // 8), 32))
    per_slice = -(-chunks // S_)
    return -(-chunks // per_slice)


def deca_layers():
    """(forward, backward) conv launches of deca.hip as (N, Ho, K): stem, per bottleneck conv1, conv2, [projection], conv3, the two
    regressor layers; backward: the regressor transposed, per bottleneck conv3^T, conv2^T, conv1^T (+ the projection^T in K)."""
    fwd, bwd = [(64, 112, 147)], [(1024, 1, 236), (2048, 1, 1024)]
    blocks, cin, h = [], 64, 56
    for s, (planes, count) in enumerate(RD.LAYERS):
        for k in range(count):
            ho = h // 2 if (k == 0 and s > 0) else h
            blocks.append((cin, planes, h, ho, k == 0))
            cin, h = 4 * planes, ho
    for cin, p, h, ho, ds in blocks:
        fwd += [(p, h, cin), (p, ho, 9 * p)] + ([(4 * p, ho, cin)] if ds else []) + [(4 * p, ho, p)]
    for cin, p, h, ho, ds in reversed(blocks):
        bwd += [(p, ho, 4 * p), (p, h, 9 * p), (cin, h, p + (4 * p if ds else 0))]
    return fwd + [(1024, 1, 2048), (236, 1, 1024)], bwd


def fan_layers():
    """The 191 conv launches of fan.hip as (N, Ho, K)."""
    out = [(64, 128, 147)]

    def block(cin, cout, h):
        if cin != cout:
            out.append((cout, h, cin))
        out.extend([(cout // 2, h, 9 * cin), (cout // 4, h, 9 * cout // 2), (cout // 4, h, 9 * cout // 4)])

    def hourglass(level, h):
        block(256, 256, h // 2)                      # b2
        if level > 1:
            hourglass(level - 1, h // 2)
        else:
            block(256, 256, h // 2)                  # b2_plus
        block(256, 256, h // 2)                      # b3
        block(256, 256, h)                           # b1, after the lower branch

    block(64, 128, 128), block(128, 128, 64), block(128, 256, 64)
    for s in range(RF.STACKS):
        hourglass(RF.DEPTH, 64)
        block(256, 256, 64)
        out.extend([(256, 64, 256), (68, 64, 256)])
        if s + 1 < RF.STACKS:
            out.append((256, 64, 256 + 68))
    return out


def planned_finishes(layers, B):
    return sum(slices(B, n, ho, ho, k) > 1 for n, ho, k in layers)


def _launches(fn, stem):
    """(conv launches, finish launches) of fn(), profiled after the caller's warm-up."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return sum(stem + '_conv_kernel' in n for n in names), sum(stem + '_finish_kernel' in n for n in names)


# ---------------------------------------------------------------------------------------------------------------- DECA front
def _check_front(x, M, tag, cot_key):
    """deca.crop and its adjoint on images x [B,3,H,W] and float32 matrices M [B,2,3] against F.grid_sample in fp64, per row, with
    the assertions and bars of test_gpu_deca.test_front_and_its_adjoint_match_fp64_grid_sample."""
    from stylegan_directions_face_reenactment_amd import deca as D
    B = x.shape[0]
    cot = S.counter_tensor(SEED, cot_key, (B, 3, 224, 224), 0.0, 1.0)
    x64 = x.double().requires_grad_(True)
    ref = RD.front(x64, M.double())
    ref.backward(cot.double())
    x32 = x.cuda().requires_grad_(True)
    stock = RD.front(x32, M.cuda())
    stock.backward(cot.cuda())
    xh = x.cuda().requires_grad_(True)
    out = D.crop(xh, M.cuda())
    out.backward(cot.cuda())
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(xh.grad[xh.detach().abs() > 1])) == 0 and int((x.abs() > 1).sum()) > 0
    for b in range(B):
        r, g = ref[b].detach(), x64.grad[b]
        dev = float((stock[b].detach().double().cpu() - r).abs().max())
        err = float((out[b].detach().double().cpu() - r).abs().max())
        gmax = float(g.abs().max())
        gdev = float((x32.grad[b].double().cpu() - g).abs().max())
        gerr = float((xh.grad[b].double().cpu() - g).abs().max())
        share = float((g.abs().sum(0) > 0).double().mean())
        print('front %-16s row %d crop: hip %.3e, torch fp32 %.3e (ratio %.2f); adjoint: hip %.3e, torch fp32 %.3e (ratio %.2f), '
              'max |grad| %.3e on %.1f %% of the pixels, crop max %.3f' % (tag, b, err, dev, err / max(dev, 1e-30), gerr, gdev,
                                                                         gerr / max(gdev, 1e-30), gmax, 100 * share, float(r.max())))
        assert err <= max(8 * dev, 1e-6)
        assert gerr <= max(8 * gdev, 1e-6 * gmax)
        assert float(out[b].max()) > 0.5 and gmax > 0


@pytest.mark.parametrize('name', list(RD.FRONT_GEOMETRIES))
def test_deca_front_and_adjoint_at_unusual_matrices(name):
    """One row per geometry of deca_restatement.FRONT_GEOMETRIES: down-scaling by 4.6 from 1024^2, up-scaling by 8 from 64 x 48,
    rotation + shear + anisotropy, a mirrored matrix, and the three without a usable inverse: 'singular_exact' (determinant exactly
    0: the adjoint's all-candidates fallback), 'singular' (the issue's matrix: with the fused multiply-add of the build its
    determinant is rounding noise of 4e-11, above the 1e-12 switch, so the inverse branch runs with a box clamped to the whole
    crop) and 'near_singular'."""
    from stylegan_directions_face_reenactment_amd import deca as D
    H, W, _ = RD.FRONT_GEOMETRIES[name]
    x = TD._images(1, H, W, 'deca.geo.' + name)
    _check_front(x, RD.front_matrix(name, D.crop_matrix), name, 'deca.geo.g.' + name)


def test_deca_front_batched_rows_take_their_own_matrix():
    """The four non-singular geometries in one call, their images resized to a common 256^2 (the matrices with them)."""
    from stylegan_directions_face_reenactment_amd import deca as D
    xs, Ms = [], []
    for name in RD.NON_SINGULAR:
        H, W, _ = RD.FRONT_GEOMETRIES[name]
        x = TD._images(1, H, W, 'deca.geo.' + name)
        xs.append(torch.nn.functional.interpolate(x, size=(256, 256), mode='bilinear', align_corners=False))
        Ms.append(RD.resized_matrix(RD.front_matrix(name, D.crop_matrix), (H, W), (256, 256)))
    _check_front(torch.cat(xs), torch.cat(Ms), 'batched', 'deca.geo.g.batched')


# ---------------------------------------------------------------------------------------------------------------- DECA angles
def test_deca_angle_branches_on_the_device():
    """The regressor's last layer with a zero weight and the wanted pose[:3] as bias gives that pose exactly, whatever the image.
    The bias is shared by the rows of a call, so each of deca_restatement.ANGLE_ROWS is a call of its own (five rows of different
    images, all of which must come out alike); the pack is rebuilt after every in-place edit of the bias."""
    from stylegan_directions_face_reenactment_amd import deca as D
    E0, _ = TD._module(SEED)
    E = copy.deepcopy(E0)
    B, H, W = 5, 256, 256
    x = TD._images(B, H, W, 'deca.angles').cuda()
    M = D.crop_matrix(TD._boxes(B, H, W, 'deca.angles'), (H, W)).cuda()
    rows = torch.tensor(RD.ANGLE_ROWS, dtype=torch.float64)
    r20 = RD.r20(rows)
    print('angle rows: R20 = %s' % ['%.6f' % v for v in r20.tolist()])
    assert float(r20[2]) > 0.9999 and float(r20[3]) < -0.9999 and 0.99 < float(r20[4]) < 0.9975 and abs(float(r20[1])) < 0.9
    bias = E.layers[2].bias
    keep = bias.detach().clone()
    with torch.no_grad():
        E.layers[2].weight.zero_()
    packs = []
    for i, row in enumerate(RD.ANGLE_ROWS):
        with torch.no_grad():
            bias.zero_()
            bias[200:203] = torch.tensor(row, dtype=torch.float32)
        params, angles = D.calculate_shapemodel(E, x, M)
        packs.append(E.packed())
        pose = params['pose'][:, :3]
        assert torch.equal(pose.cpu(), torch.tensor(row, dtype=torch.float32).expand(B, 3))      # 0 * h + bias, exactly
        want = RD.angles(pose.double().cpu())
        got = angles.double().cpu()
        err = float((got - want).abs().max())
        print('angles of pose %s: hip %s, fp64 %s, max difference %.3e deg (bar 1e-2)' % (row, got[0].tolist(), want[0].tolist(), err))
        assert torch.equal(angles, angles[:1].expand(B, 3))
        assert err <= 1e-2
        if i == 0:
            assert int(torch.count_nonzero(angles)) == 0
        if i in (2, 3):
            assert abs(float(got[0, 0]) - (90.0 if i == 2 else -90.0)) <= 1e-2 and int(torch.count_nonzero(angles[:, 2])) == 0
            assert abs(float(want[0, 0]) - (90.0 if i == 2 else -90.0)) <= 1e-9 and float(want[0, 2]) == 0.0
    assert all(a is not b for a, b in zip(packs, packs[1:]))
    with torch.no_grad():
        bias.copy_(keep)
    assert E.packed() is not packs[-1]


# ---------------------------------------------------------------------------------------------------------------- DECA 48 rows
DECA_PATTERN = [(5 * i + i // 7 + (i * i) // 11) % 3 for i in range(48)]


def _same_rows(t, groups):
    """Every copy of a row bit-equal to its first copy."""
    return all(torch.equal(t[idx], t[idx[:1]].expand_as(t[idx])) for idx in groups)


def test_deca_48_rows_copies_are_bit_equal_and_first_copies_match_fp64():
    """48 rows made of 3 distinct ones in a fixed irregular pattern: copies of a row are bit-equal in everything the forward and
    the backward write; the first copy of each meets the bars of test_gpu_deca.test_stages_decisions_and_gradient_match_fp64."""
    from stylegan_directions_face_reenactment_amd import deca as D
    E, sd = TD._module(SEED)
    H = W = 256
    assert sorted(set(DECA_PATTERN)) == [0, 1, 2] and DECA_PATTERN != sorted(DECA_PATTERN)
    groups = [torch.tensor([i for i, r in enumerate(DECA_PATTERN) if r == d]) for d in range(3)]
    first = torch.tensor([int(g[0]) for g in groups])
    x3 = TD._images(3, H, W, 'deca.rows48')
    M3 = D.crop_matrix(TD._boxes(3, H, W, 'deca.rows48'), (H, W))
    cot3 = S.counter_tensor(SEED, 'deca.rows48.g', (3, 236), 0.0, 1.0)
    x, M, cot = x3[DECA_PATTERN].contiguous(), M3[DECA_PATTERN].contiguous(), cot3[DECA_PATTERN].contiguous()
    params, angles, crop, saved, dbg = D.run_debug(E, x.cuda(), M.cuda(), save=True)
    dx = D.backward_from(E, cot.cuda(), x.cuda(), M.cuda(), saved)
    torch.cuda.synchronize()
    gg = [g.cuda() for g in groups]
    named = {'crop': crop, 'params': params, 'angles': angles, 'dx': dx, 'stem': dbg['stem'], 'pool': dbg['pool'], 'feat': dbg['feat']}
    for s in range(4):
        named['layer%d.first' % (s + 1)], named['layer%d.last' % (s + 1)] = dbg['first'][s], dbg['last'][s]
    sv = D.saved_views(saved, 48)
    named.update({'saved.stem': sv['stem'], 'saved.arg': sv['arg'], 'saved.fc': sv['fc']})
    for k in ('m1', 'm2', 'm3'):
        for n, m in enumerate(sv[k]):
            named['saved.%s[%d]' % (k, n)] = m
    unequal = [k for k, t in named.items() if not _same_rows(t, gg)]
    print('48 rows: %d tensors compared across the copies of 3 rows, not bit-equal: %s' % (len(named), unequal))
    assert not unequal
    # the first copies against fp64
    with torch.no_grad():
        rec = RD.run(sd, x3.double(), M3.double(), fold=True)
    sel = first.cuda()
    stages = {'crop': (crop, rec['crop']), 'stem': (dbg['stem'], rec['stem']), 'pool': (dbg['pool'], rec['pool']),
              'feat': (dbg['feat'], rec['feat']), 'params': (params, rec['params'])}
    for s, (a, b) in enumerate(zip([0, 3, 7, 13], [2, 6, 12, 15])):
        stages['layer%d.first' % (s + 1)] = (dbg['first'][s], rec['out'][a])
        stages['layer%d.last' % (s + 1)] = (dbg['last'][s], rec['out'][b])
    worst = 0.0
    for k, (a, b) in stages.items():
        r = TD._rel(a[sel], b)
        worst = max(worst, r)
        print('B=48 stage %-13s %.3e of max' % (k, r))
    assert worst <= 1e-4
    a_err = float((angles[sel].double().cpu() - rec['angles']).abs().max())
    print('angles: %.3e deg' % a_err)
    assert a_err <= 1e-2
    hm = {k: ([m[sel].cpu() for m in v] if isinstance(v, list) else v[sel].cpu()) for k, v in sv.items()}
    hm = {'stem': hm['stem'].bool(), 'arg': hm['arg'].long(), 'm1': [m.bool() for m in hm['m1']], 'm2': [m.bool() for m in hm['m2']],
          'm3': [m.bool() for m in hm['m3']], 'fc': hm['fc'].bool()}
    hip = [hm['stem']] + [m for trio in zip(hm['m1'], hm['m2'], hm['m3']) for m in trio] + [hm['fc']]
    pres = RD.relu_decisions(rec)
    assert len(hip) == len(pres) == 50
    total = sum(p.numel() for p in pres)
    diff = sum(int(((p > 0) != h).sum()) for p, h in zip(pres, hip))
    counted = rec['pool'] > 0
    pdiff = int(((rec['arg'] != hm['arg']) & counted).sum())
    print('decisions: %d of %d ReLU (%.2e), %d of %d max-pool choices' % (diff, total, diff / total, pdiff, int(counted.sum())))
    assert diff <= 1e-5 * total and pdiff <= 1e-5 * int(counted.sum())
    x64 = x3.double().requires_grad_(True)
    rec2 = RD.run(sd, x64, M3.double(), fold=True, masks=hm)
    (rec2['params'] * cot3.double()).sum().backward()
    g_err = TD._rel(dx[sel], x64.grad)
    print('dL/dx under the HIP decisions: %.3e of max (max %.3e)' % (g_err, float(x64.grad.abs().max())))
    assert float(x64.grad.abs().max()) > 0
    assert g_err <= 1e-4
    assert int(torch.count_nonzero(dx[x.cuda().abs() > 1])) == 0 and int((x3.abs() > 1).sum()) > 0


def test_deca_launch_counts_follow_the_plan_rule():
    """deca_conv_kernel / deca_finish_kernel launches of one forward and one backward at B = 1, 3, 16, 17, 48 against `slices`."""
    from stylegan_directions_face_reenactment_amd import deca as D
    E, _ = TD._module(SEED)
    H = W = 256
    fwd, bwd = deca_layers()
    x3 = TD._images(3, H, W, 'deca.rows48')
    M3 = D.crop_matrix(TD._boxes(3, H, W, 'deca.rows48'), (H, W))
    for B in ROW_COUNTS:
        rows = DECA_PATTERN[:B]
        x = x3[rows].cuda().requires_grad_(True)
        M = M3[rows].cuda()
        cot = torch.ones(B, 236, device='cuda')
        D.run(E, x, M)[0].backward(cot)                                  # warm-up
        out = []
        cf = _launches(lambda: out.append(D.run(E, x, M)[0]), 'deca')
        cb = _launches(lambda: out[0].backward(cot), 'deca')
        want = (planned_finishes(fwd, B), planned_finishes(bwd, B))
        print('deca B = %2d: forward %d convs + %d finishes, backward %d + %d; the rule gives %d / %d finishes' % (B, cf[0], cf[1], cb[0],
                                                                                                                  cb[1], want[0], want[1]))
        assert (cf[0], cb[0]) == (55, 50)
        assert (cf[1], cb[1]) == want


# ---------------------------------------------------------------------------------------------------------------- FAN
_FAN = {}


def _fan():
    from stylegan_directions_face_reenactment_amd import landmarks as L
    if not _FAN:
        kat = golden(KAT)
        state = S.synthetic_fan_state(int(kat['seed']))
        m = L.FAN(4)
        m.load_state_dict(state, strict=True)
        _FAN.update(kat=kat, state=state, fan=m.cuda().eval(), dev=max(float(kat['dev_heatmaps_a']), float(kat['dev_heatmaps_b'])))
    return _FAN['kat'], _FAN['state'], _FAN['fan'], _FAN['dev']


# the integer windows (l1x, l1y, l2x, l2y) that the float32 centre / scale / transform give for fan_restatement.GEO_CASES
GEO_WINDOWS = {
    'inside1024': [[52, 14, 951, 913]],                              # 899^2, wholly inside
    'small96': [[-6, -9, 88, 85], [-34, 0, 71, 106]],                # 94^2 and 105 x 106, leaving the 96 x 80 image
    'tiny_up': [[81, 80, 148, 147]],                                 # 67^2, up-scaled by 3.8
    'wide': [[141, -75, 389, 172]],                                  # 248 x 247, half outside the 120 x 640 strip
    'outside': [[786, 769, 1215, 1198]],                             # wholly outside: a zero crop
    'huge': [[-865, -938, 942, 869]],                                # 1807^2 around a 64^2 image
}


@pytest.mark.parametrize('input_range', ['255', 'gan'])
@pytest.mark.parametrize('name', list(RF.GEO_CASES))
def test_fan_front_geometries(name, input_range):
    """landmarks.crop against F.interpolate of the zero-padded window in fp64, within 8 x the deviation of torch's own fp32 form."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    kat, _, _, _ = _fan()
    x, faces = RF.geo_inputs(S, int(kat['seed']), name)
    B, _, H, W = x.shape
    wins = RF.windows(faces)
    print('front geometry %s: image %d x %d, windows %s' % (name, H, W, wins))
    assert wins == GEO_WINDOWS[name]
    for (l1x, l1y, l2x, l2y) in wins:
        inside = l1x >= 0 and l1y >= 0 and l2x <= W and l2y <= H
        outside = l1x >= W or l1y >= H or l2x <= 0 or l2y <= 0
        assert inside == (name in ('inside1024', 'tiny_up')) and outside == (name == 'outside')
    if input_range == 'gan':
        x = RF.to_gan(x)
    want = RF.crop(x.double(), faces, input_range)
    stock = RF.crop(x.cuda(), faces, input_range).double().cpu()          # torch's own fp32 on the device
    got = L.crop(x.cuda(), faces.cuda(), input_range).double().cpu()
    dev, err = float((stock - want).abs().max()), float((got - want).abs().max())
    print('front geometry %s range %s: max |HIP - fp64| %.3e, torch fp32 %.3e (%.2f x)   bar 8 x' % (name, input_range, err, dev,
                                                                                                    err / max(dev, 1e-30)))
    if name == 'outside':
        assert float(want.abs().max()) == 0.0 and float(stock.abs().max()) == 0.0 and float(got.abs().max()) == 0.0
    else:
        assert dev > 0 and float(want.max()) > 0.5
    assert err <= 8 * dev


@pytest.mark.parametrize('name', list(RF.GEO_CASES))
def test_fan_network_and_decode_on_the_geometries(name):
    """get_landmarks / run_debug on each geometry: the last heatmaps within 8 x dev_heatmaps of the fp64 restatement, and the decode
    equal to fan_restatement.decode of the fp64 heatmaps on every safe landmark (fan_restatement.safe_landmarks)."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    kat, state, fan, dev = _fan()
    x, faces = RF.geo_inputs(S, int(kat['seed']), name)
    B = x.shape[0]
    bar = 8 * dev
    with torch.no_grad():
        crop64 = RF.crop(x.double(), faces)
        hm64 = RF.network(state, crop64)['heatmaps'][-1]
    if name == 'outside':
        assert float(crop64.abs().max()) == 0.0
    pts_img, pts, hm, boxes, views = L.run_debug(fan, x.cuda(), faces.cuda())
    again = L.get_landmarks(fan, x.cuda(), faces.cuda())
    torch.cuda.synchronize()
    assert torch.equal(again[0], pts_img) and torch.equal(again[1], pts) and torch.equal(again[2], hm)
    err = float((hm.double().cpu() - hm64).abs().max())
    print('geometry %s: last heatmaps max |HIP - fp64| %.3e = %.2f x dev_heatmaps %.3e   bar 8 x; heatmap range %.3f .. %.3f' % (
        name, err, err / dev, dev, float(hm64.min()), float(hm64.max())))
    assert err <= bar
    d = RF.decode(hm64, faces)
    safe = RF.safe_landmarks(hm64, faces, 16 * bar)
    unsafe = (~safe).sum(1).tolist()
    print('geometry %s: unsafe landmarks per row %s (at most 8 of 68)' % (name, unsafe))
    assert max(unsafe) <= 8, 'badly chosen case: %s' % unsafe
    idx = hm.reshape(B, 68, -1).argmax(2).cpu()
    pi, p, bx = pts_img.cpu(), pts.cpu(), boxes.cpu()
    assert torch.isfinite(pi).all() and torch.isfinite(p).all()
    n_idx = int((idx != d['idx'])[safe].sum())
    n_pts = int((p != d['pts'])[safe].sum())
    n_img = int((pi != d['pts_img'])[safe].sum())
    print('geometry %s: on the safe landmarks arg-max differs in %d, pts in %d, pts_img in %d values' % (name, n_idx, n_pts, n_img))
    assert n_idx == 0 and n_pts == 0 and n_img == 0
    assert torch.equal(bx, torch.cat([pi.min(1).values, pi.max(1).values], 1)) and torch.equal(L.kpt68_boxes(pts_img).cpu(), bx)
    for b in range(B):
        if unsafe[b] == 0:
            assert torch.equal(bx[b], d['boxes'][b])
        else:
            mine, want = pi[b][safe[b]], d['pts_img'][b][safe[b]]
            assert torch.equal(torch.cat([mine.min(0).values, mine.max(0).values]), torch.cat([want.min(0).values, want.max(0).values]))
    if name == 'tiny_up':
        assert unsafe == [0]


def test_fan_degenerate_box_gives_a_zero_crop_and_finite_outputs():
    """x0 = x1, y0 = y1: scale 0, the inverse transform is not a number and gives no window."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    kat, _, fan, _ = _fan()
    x, good = RF.fixture_inputs(S, int(kat['seed']), 'b')
    faces = torch.stack([torch.tensor([120.0, 90.0, 120.0, 90.0]), good[1]])
    for input_range in ('255', 'gan'):
        xi = RF.to_gan(x) if input_range == 'gan' else x
        c = L.crop(xi.cuda(), faces.cuda(), input_range)
        assert int(torch.count_nonzero(c[0])) == 0 and float(c[1].max()) > 0.5
    pts_img, pts, hm, boxes, _ = L.run_debug(fan, x.cuda(), faces.cuda())
    torch.cuda.synchronize()
    print('degenerate box: pts_img %s .. %s, heatmaps %.3f .. %.3f, box %s' % (pts_img[0].min().item(), pts_img[0].max().item(),
                                                                              float(hm[0].min()), float(hm[0].max()), boxes[0].tolist()))
    for t in (pts_img, pts, hm, boxes):
        assert bool(torch.isfinite(t).all())
    assert np_equal(pts_img[1], kat['pts_img_b'][1]) and np_equal(pts[1], kat['pts_b'][1])      # the row beside it is untouched


def np_equal(t, a):
    return bool((t.cpu().numpy() == a).all())


FAN_PATTERN = [(i * i + i // 3 + i // 5) % 2 for i in range(48)]


def test_fan_48_rows_copies_are_bit_equal_and_counts_match_the_plan():
    """48 rows from the two rows of kat13's case b in a fixed irregular pattern: copies bit-equal in heatmaps, pts, pts_img and
    boxes; the first copies within the bar of test_rows_are_independent_across_batch_sizes_and_plans; the landmarks equal the
    fixture's.  Finish launches at B = 1, 3, 16, 17, 48: DESIGN 4.16's 188, 165, 132, 108, 96 with 191 conv launches each."""
    from stylegan_directions_face_reenactment_amd import landmarks as L
    kat, state, fan, _ = _fan()
    x2, f2 = RF.fixture_inputs(S, int(kat['seed']), 'b')
    assert sorted(set(FAN_PATTERN)) == [0, 1] and FAN_PATTERN[:24] != FAN_PATTERN[24:]
    with torch.no_grad():
        want = RF.network(state, RF.crop(x2.double(), f2))['heatmaps'][-1]
    bar = 8 * float(kat['dev_heatmaps_b'])
    x, f = x2[FAN_PATTERN].cuda(), f2[FAN_PATTERN].cuda()
    pts_img, pts, hm, boxes, _ = L.run_debug(fan, x, f)
    torch.cuda.synchronize()
    groups = [torch.tensor([i for i, r in enumerate(FAN_PATTERN) if r == d]).cuda() for d in range(2)]
    unequal = [k for k, t in (('heatmaps', hm), ('pts', pts), ('pts_img', pts_img), ('boxes', boxes)) if not _same_rows(t, groups)]
    first = [int(g[0]) for g in groups]
    err = float((hm[first].double().cpu() - want).abs().max())
    print('fan 48 rows: not bit-equal across copies: %s; first copies max |HIP - fp64| %.3e   bar %.3e' % (unequal, err, bar))
    assert not unequal
    assert err <= bar
    assert np_equal(pts_img[first], kat['pts_img_b']) and np_equal(pts[first], kat['pts_b']) and np_equal(boxes[first], kat['boxes_b'])
    counts = {}
    for B in ROW_COUNTS:
        xb, fb = x[:B].contiguous(), f[:B].contiguous()
        L.get_landmarks(fan, xb, fb)
        counts[B] = _launches(lambda: L.get_landmarks(fan, xb, fb), 'fan')
        print('fan B = %2d: %d convs, %d of them sliced over K; the rule gives %d' % (B, counts[B][0], counts[B][1],
                                                                                    planned_finishes(fan_layers(), B)))
    assert all(c[0] == 191 for c in counts.values()), counts
    assert [counts[B][1] for B in ROW_COUNTS] == [188, 165, 132, 108, 96], counts

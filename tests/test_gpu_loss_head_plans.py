"""GPU: the three loss heads (csrc/lpips.hip, csrc/idloss.hip, csrc/flame.hip) on the sides of their host-side choices that the
per-head modules do not reach: convs that keep all of K in one slice and apply their epilogue themselves (LPIPS at 1024^2 and at
the trainer's batch of 16, IDLoss at B >= 8), the smallest and the uneven image geometries, the enlarging / 1x1 / 9-10 pixel bins
of the IDLoss front, and FLAME row chunks after the first.  Every figure is measured against the fp64 restatements on the CPU
(lpips_restatement, idloss_restatement, flame_restatement), never against another run of the HIP code.

Bars are the ones of test_gpu_lpips / test_gpu_id_loss / test_gpu_flame for the same quantities: LPIPS taps 1e-5, loss 1e-5,
dL/dx 1e-4; IDLoss stages, embedding and dL/dx 1e-4, at most 1e-4 of the PReLU / SE-ReLU decisions differing from fp64; FLAME
outputs 2e-6, ShapeLoss within max(4 x the composition's own deviation from fp64, 2e-6).

Which path ran is proven by counting the `lpips_finish_kernel` / `idl_finish_kernel` launches with torch.profiler (a conv whose K
is sliced is followed by one; a conv that applies its epilogue itself is not).

Measured on an MI355X, the largest over all cases of this module (each test prints its own): LPIPS taps 2.7e-6 (tap 4 at
(16,256,256) live), loss 1.1e-7, dL/dx 4.0e-6 ((1,1024,1024) cached); IDLoss stages 3.4e-6 (c2[20] at B=33), embedding 1.3e-6,
dL/dx 1.2e-6, at most 1.3e-7 of the decisions differing from fp64 (13 of 122.5 M at B=33); ShapeLoss against the composition at
most 1.7e-7 with the gradients bit-equal; decode rows bit-equal.  Finish launches, forward + backward: LPIPS (1,256,256) cached
4 + 2, (1,1024,1024) and (16,256,256) cached 2 + 1, (2,1024,1024) live 0 + 0; IDLoss 92 of 102 convs at B=3, 10 of 102 at B=33.
The module takes about 40 s, most of it the fp64 restatements.

LPIPS gradients: with a live y, x's taps come out of launches of 2B rows, whose split-K plan and so summation order differ from
those of x alone; at (16,256,256), (1,1024,1024) and (1,512,512) one ReLU decision of x's taps differs between the two forwards.
With the decisions of the forward of x alone, the fp64 gradient of the live call at (16,256,256) is 1.01e-4 away (one flipped
decision), with the live forward's own decisions 3.8e-6: each gradient is compared under the decisions of its own forward.
"""
import pytest
import torch

from util import S, SEED
import flame_restatement as RF
import idloss_restatement as RI
import lpips_restatement as RL
import test_gpu_flame as TF
import test_gpu_id_loss as TI
import test_gpu_lpips as TL

pytestmark = pytest.mark.gpu


def _finish_launches(fn, needle):
    """Names of the device kernels of fn() (profiled after the caller's warm-up) and how many of them contain `needle`."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return names, sum(needle in n for n in names)


# ---------------------------------------------------------------------------------------------------------------- LPIPS
# (B, H, W, target rows, gradient modes): 'live' = y as an image in the same launches (2B rows), 'cached' = m.target(y)
LPIPS_CASES = [
    (16, 256, 256, 16, ('live', 'cached')),     # trainer batch: forward K slices 1,1,1,2,2 cached and all 1 live
    (1, 1024, 1024, 1, ('cached',)),            # PTI on the 1024 generator: 1,1,1,2,2 / input gradient 2,2,1,2
    (2, 1024, 1024, 2, ('live',)),              # no slicing anywhere
    (1, 512, 512, 1, ('cached',)),              # 1,2,5,8,8 / 8,10,5,8
    (1, 31, 31, 1, ('live', 'cached')),         # smallest supported side: last maps 1x1
    (2, 31, 47, 2, ('live', 'cached')),         # last maps 1x2
    (1, 67, 95, 1, ('live', 'cached')),         # tap 1 is 16x23: the 3/2 pool never reads its last row
    (5, 100, 76, 1, ('cached',)),               # one-row target against five images: maps 24x18, 11x8, 5x3
    (17, 40, 40, 17, ('live', 'cached')),       # many rows of tiny maps, partial 64-pixel tiles in every layer
]


def _lpips_taps_of_x(m, x, y):
    """The five taps of x's rows from the HIP forward of x alone (y None) or of x and a live y in the same launches."""
    from stylegan_directions_face_reenactment_amd import lpips as L
    B, _, H, W = x.shape
    rows = B + (0 if y is None else y.shape[0])
    feats = L._features(m.packed(), x.contiguous(), y, H, W).cpu()
    out, o = [], 0
    for t in RL.taps(m.state_dict(), torch.zeros(1, 3, H, W, dtype=torch.float64)):
        n = rows * t[0].numel()
        out.append(feats[o:o + n].view((rows,) + tuple(t.shape[1:]))[:B])
        o += n
    assert o == feats.numel()
    return out


@pytest.mark.parametrize('B,H,W,By,modes', LPIPS_CASES, ids=['%dx%dx%d' % c[:3] for c in LPIPS_CASES])
def test_lpips_taps_loss_and_gradient_match_fp64(B, H, W, By, modes):
    m, sd = TL._module()
    tag = '%d_%d_%d' % (B, H, W)
    x = S.counter_tensor(SEED, 'lp.sw.x' + tag, (B, 3, H, W), 0.0, 0.5).clamp(-1, 1)
    y = S.counter_tensor(SEED, 'lp.sw.y' + tag, (By, 3, H, W), 0.0, 0.5).clamp(-1, 1)
    xh, yh = x.cuda(), y.cuda()
    ylive = yh if By == B else yh.expand(B, -1, -1, -1).contiguous()
    ref_taps = RL.taps(sd, x)
    ref = float(RL.lpips(sd, x, y))
    figures = []
    figures.append(('loss live', abs(float(m(xh, ylive)) - ref) / abs(ref), 1e-5))
    figures.append(('loss cached', abs(float(m(xh, m.target(yh))) - ref) / abs(ref), 1e-5))
    # x's taps as each kind of call computes them: alone (cached target) or in the same launches as a live y, where the 2B rows
    # make another split-K plan, so another summation order and, now and then, another ReLU / pool decision near a tie.  The
    # fp64 gradient takes the decisions of the forward that is differentiated.
    alone = None
    for mode in ('cached', 'live'):
        hip = _lpips_taps_of_x(m, xh, ylive if mode == 'live' else None)
        if alone is None:
            alone = hip
        else:
            print('lpips (%d,%d,%d) live against alone: %d tap values differ, %d ReLU decisions' % (
                B, H, W, sum(int((a != b).sum()) for a, b in zip(hip, alone)), sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(hip, alone))))
        for t, (a, b) in enumerate(zip(hip, ref_taps)):
            assert a.shape == b.shape
            figures.append(('tap %d %s %s' % (t + 1, tuple(a.shape[2:]), mode), TL._rel(a, b), 1e-5))
        if mode not in modes:
            continue
        xr = x.double().requires_grad_(True)
        (RL.lpips(sd, xr, y, fixed=hip) * 3.0).backward()
        xg = x.cuda().requires_grad_(True)
        (m(xg, ylive if mode == 'live' else m.target(yh)) * 3.0).backward()
        figures.append(('dL/dx ' + mode, TL._rel(xg.grad, xr.grad), 1e-4))
    for what, v, bar in figures:
        print('lpips (%d,%d,%d) %-18s %.3e   bar %.0e' % (B, H, W, what, v, bar))
    assert ref > 1e-3
    for what, v, bar in figures:
        assert v <= bar, (what, v, bar)


def _lpips_finish_counts(m, B, H, W, live):
    """(forward, backward) lpips_finish_kernel launches of one loss and one backward; the target is computed outside."""
    tag = '%d_%d_%d' % (B, H, W)
    x = S.counter_tensor(SEED, 'lp.sw.x' + tag, (B, 3, H, W), 0.0, 0.5).clamp(-1, 1).cuda().requires_grad_(True)
    y = S.counter_tensor(SEED, 'lp.sw.y' + tag, (B, 3, H, W), 0.0, 0.5).clamp(-1, 1).cuda()
    tgt = y if live else m.target(y)
    m(x, tgt).backward()                                    # warm-up: the weight pack, the allocator
    out = {}
    names_f, nf = _finish_launches(lambda: out.update(loss=m(x, tgt)), 'lpips_finish_kernel')
    names_b, nb = _finish_launches(lambda: out['loss'].backward(), 'lpips_finish_kernel')
    convs = sum('lpips_conv_kernel' in n for n in names_f), sum('lpips_conv_kernel' in n for n in names_b)
    assert convs == (5, 4), (convs, names_f, names_b)
    return nf, nb


def test_lpips_unsliced_convs_run_their_own_epilogue():
    """K slices per conv from plan_conv (csrc/lpips.hip), forward layers 0..4 / input-gradient convs of layers 4..1:
    (1,256,256) cached 1,10,16,16,16 / 16,16,16,16 -> 4 + 2 finish launches (layers 1-4; layers 4 and 3 -- the pooled layers 2 and 1
    sum their slices in lpips_pool_bwd_kernel); (1,1024,1024) and (16,256,256) cached 1,1,1,2,2 / 2,1,2,2 -> 2 + 1 (layer 3's
    input-gradient conv masks and adds the tap gradient itself); (2,1024,1024) live: 1 everywhere -> none."""
    m, _ = TL._module()
    got = {}
    for B, H, W, live in ((1, 256, 256, False), (1, 1024, 1024, False), (16, 256, 256, False), (2, 1024, 1024, True)):
        got[(B, H, W)] = _lpips_finish_counts(m, B, H, W, live)
        print('lpips (%d,%d,%d) %s: %d forward + %d backward finish launches' % ((B, H, W, 'live' if live else 'cached') + got[(B, H, W)]))
    assert got[(1, 256, 256)] == (4, 2)
    assert got[(1, 1024, 1024)] == (2, 1)
    assert got[(16, 256, 256)] == (2, 1)
    assert got[(2, 1024, 1024)] == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- IDLoss
IDL_CASES = [
    (8, 256, 256, True), (16, 256, 256, True), (33, 256, 256, True),     # ~20 %, ~36 %, ~90 % of the convs unsliced
    (2, 64, 64, False),            # the pool enlarges 64 -> 112
    (2, 100, 90, True),            # crop window 65x58, enlarged
    (2, 36, 33, True),             # crop window 1x1
    (1, 1024, 1024, False),        # bins of 9-10 pixels
    (2, 1024, 1024, True),         # the 188x188 window inside a large image
    (3, 300, 200, False),          # different bin widths per axis
    (1, 20, 20, False),            # below the crop window's origin: no-crop only
]
IDL_CHUNK = 8                      # rows per fp64 pass (eval mode: rows are independent), bounds the host memory of its autograd


@pytest.mark.parametrize('B,H,W,crop', IDL_CASES, ids=['%dx%dx%d' % c[:3] for c in IDL_CASES])
def test_idloss_stages_embedding_and_gradient_match_fp64(B, H, W, crop):
    from stylegan_directions_face_reenactment_amd import id_loss as L
    m, sd = TI._module()
    x = S.counter_tensor(SEED, 'idl.sw%d_%d_%d' % (B, H, W), (B, 3, H, W), 0.0, 0.5).clamp(-1, 1)
    ge = S.counter_tensor(SEED, 'idl.sw.ge%d_%d_%d' % (B, H, W), (B, 512))
    emb, saved = L._forward(m.facenet.packed(), x.cuda().contiguous(), None, crop, True)
    V = L.saved_views(saved.cpu(), B)
    del saved
    masks = {'p0': V['p0'] > 0, 'p1': [p > 0 for p in V['p1']], 'h': [gt[:, gt.shape[1] * 16 // 17:] > 0 for gt in V['gate']]}
    xg = x.cuda().requires_grad_(True)
    (m.extract_feats(xg, crop) * ge.cuda()).sum().backward()
    first = [i for i, u in enumerate(RI.UNITS) if u[2] == 2]
    units = first + [i - 1 for i in first[1:]] + [len(RI.UNITS) - 1]     # each stage's first (stride-2) unit and each stage's last
    worst = {'p0': 0.0, 'p1': 0.0, 'c2': 0.0, 'gate': 0.0}
    scale = {'p0': 0.0, 'p1': {}, 'c2': {}, 'gate': {}}
    diff = {'p1': {}, 'c2': {}, 'gate': {}}
    flips = total = 0
    e_ref, g_ref = [], []
    for r0 in range(0, B, IDL_CHUNK):
        sl = slice(r0, min(B, r0 + IDL_CHUNK))
        with torch.no_grad():
            ref = RI.backbone(sd, x[sl], crop)
        pairs = [(masks['p0'][sl], ref['p0'] > 0)]
        pairs += [(a[sl], b > 0) for a, b in zip(masks['p1'], ref['p1'])] + [(a[sl], b > 0) for a, b in zip(masks['h'], ref['h'])]
        flips += sum(int((a != b).sum()) for a, b in pairs)
        total += sum(a.numel() for a, _ in pairs)
        # max-abs difference and max-abs reference per quantity, accumulated over the chunks (the _rel of the whole batch)
        worst['p0'] = max(worst['p0'], float((V['p0'][sl].double() - ref['p0']).abs().max()))
        scale['p0'] = max(scale['p0'], float(ref['p0'].abs().max()))
        for i in units:
            d = ref['c2'][i].shape[1]
            for k, a, b in (('p1', V['p1'][i][sl], ref['p1'][i]), ('c2', V['c2'][i][sl], ref['c2'][i]), ('gate', V['gate'][i][sl, :d], ref['g'][i])):
                diff[k][i] = max(diff[k].get(i, 0.0), float((a.double() - b).abs().max()))
                scale[k][i] = max(scale[k].get(i, 0.0), float(b.abs().max()))
        e_ref.append(ref['e'])
        del ref, pairs
        mk = {'p0': masks['p0'][sl], 'p1': [a[sl] for a in masks['p1']], 'h': [a[sl] for a in masks['h']]}
        xr = x[sl].double().requires_grad_(True)
        (RI.backbone(sd, xr, crop, mk)['e'] * ge[sl].double()).sum().backward()
        g_ref.append(xr.grad)
    e_ref, g_ref = torch.cat(e_ref), torch.cat(g_ref)
    figures = [('p0', worst['p0'] / scale['p0'])]
    for i in units:
        figures += [('%s[%d]' % (k, i), diff[k][i] / scale[k][i]) for k in ('p1', 'c2', 'gate')]
    figures += [('embedding', TI._rel(emb, e_ref)), ('dL/dx', TI._rel(xg.grad, g_ref))]
    for what, v in figures:
        print('idloss (%d,%d,%d,%s) %-10s %.3e   bar 1e-04' % (B, H, W, crop, what, v))
    print('idloss (%d,%d,%d,%s) decisions: %d of %d differ from fp64 (cap %d)' % (B, H, W, crop, flips, total, int(1e-4 * total)))
    assert float(g_ref.abs().max()) > 0
    assert flips <= 1e-4 * total, (flips, total)
    for what, v in figures:
        assert v <= 1e-4, (what, v)
    if crop:
        assert TI._outside_window_nonzero(xg.grad) == 0


def test_idloss_no_crop_takes_images_smaller_than_the_crop_window():
    """crop=False pools whatever it is given (AdaptiveAvgPool2d accepts any size); crop=True on an image that ends before the
    window's origin (row 35, column 32) has nothing to pool and is refused by name."""
    m, sd = TI._module()
    x = S.counter_tensor(SEED, 'idl.sw.small', (1, 3, 20, 20), 0.0, 0.5).clamp(-1, 1)
    e = m.extract_feats(x.cuda(), crop=False)
    assert TI._rel(e, RI.backbone(sd, x, False)['e']) <= 1e-4
    with pytest.raises(RuntimeError, match=r'unsupported image size 20x20 \(crop=1\)'):
        m.extract_feats(x.cuda(), crop=True)
    for shape in ((1, 3, 35, 64), (1, 3, 64, 32)):
        with pytest.raises(RuntimeError, match=r'\(crop=1\)'):
            m.extract_feats(torch.zeros(shape).cuda(), crop=True)


def test_idloss_most_convs_finish_in_kernel_at_b33():
    """plan_conv (csrc/idloss.hip) slices K while a conv has fewer than 512 output tiles, and a sliced conv is followed by
    idl_finish_kernel: 92 of the 102 conv launches of a forward + backward at B=3, 10 of 102 at B=33 (the 25088-deep head GEMM
    is sliced at every batch size, so the count never reaches zero)."""
    m, _ = TI._module()
    counts = {}
    for B in (3, 33):
        x = S.counter_tensor(SEED, 'idl.sw%d_256_256' % B, (B, 3, 256, 256), 0.0, 0.5).clamp(-1, 1).cuda().requires_grad_(True)
        y = m.target(S.counter_tensor(SEED, 'idl.sw.y%d' % B, (B, 3, 256, 256), 0.0, 0.5).clamp(-1, 1).cuda())
        m(x, y).backward()                                  # warm-up

        def step():
            m(x, y).backward()

        names, n = _finish_launches(step, 'idl_finish_kernel')
        counts[B] = (n, sum('idl_conv_kernel' in k for k in names))
        print('idloss B=%d forward + backward: %d of %d conv launches are followed by idl_finish_kernel' % (B, n, counts[B][1]))
    assert counts[3][1] == counts[33][1] and counts[33][1] > 0
    assert 0 < counts[33][0] < counts[3][0]
    assert counts[33][0] < 0.5 * counts[33][1]              # most convs finish in-kernel


# ---------------------------------------------------------------------------------------------------------------- FLAME
@pytest.mark.parametrize('B', [9, 20])
def test_shape_loss_equals_the_composition_across_row_chunks(B):
    """ShapeLoss decodes the gt rows and the reenacted rows in one launch of 2B rows, walked in chunks of 16: B=9 puts the
    gt/reenacted boundary inside chunk 0 and leaves a two-row tail chunk, B=20 puts it inside chunk 1."""
    from stylegan_directions_face_reenactment_amd import flame as FL
    m = TF._module(SEED)
    T = RF.tables(TF.flame_state(SEED))
    names = ('shape', 'exp', 'pose')
    gt = S.synthetic_flame_coeffs(SEED, 'flame.sw.gt%d' % B, B, [0.25 * ((i % 5) - 2) for i in range(B)])
    reen = S.synthetic_flame_coeffs(SEED, 'flame.sw.re%d' % B, B, [0.2 * ((i % 7) - 3) for i in range(B)])
    lam = (0.7, 1.3, 2.0)
    cd = {k: v.double().requires_grad_(k != 'cam') for k, v in reen.items()}
    l2g, _, tvg, _ = RF.decode(T, RF.fixed_cam({k: v.double() for k, v in gt.items()}))
    l2r, _, tvr, _ = RF.decode(T, RF.fixed_cam(cd))
    terms64 = RF.losses(l2g, tvg, l2r, tvr)
    (lam[1] * terms64[1] + lam[0] * terms64[0] + lam[2] * terms64[2]).backward()
    cg, cc = TF._cuda(gt, names), TF._cuda(reen, names)
    termsc = TF._composition(m, cg, cc)
    (lam[1] * termsc[1] + lam[0] * termsc[0] + lam[2] * termsc[2]).backward()
    chg, ch = TF._cuda(gt, names), TF._cuda(reen, names)
    loss, terms = FL.ShapeLoss(m)(chg, ch, *lam)
    loss.backward()
    assert all(chg[k].grad is None for k in names)
    figures = []
    for i, k in enumerate(('loss_shape', 'loss_mouth', 'loss_eye')):
        figures.append((k, TF._rel(terms[k], lam[i] * termsc[i]), TF._rel(termsc[i], terms64[i])))
    for k in names:
        figures.append(('d' + k, TF._rel(ch[k].grad, cc[k].grad), TF._rel(cc[k].grad, cd[k].grad)))
    for k, rel, dev in figures:
        print('ShapeLoss B=%d %-10s vs composition %.3e   composition vs fp64 %.3e   bar %.3e' % (B, k, rel, dev, TF._bar(dev)))
    for k, rel, dev in figures:
        assert rel <= TF._bar(dev), (k, rel, dev)


def test_decode_rows_do_not_depend_on_their_chunk():
    """flame_verts_kernel keeps one accumulator per row: rows 0..15 and 16..39 of a 40-row decode are bit for bit the rows
    decoded on their own (where rows 16..39 sit in chunks 0-1 instead of 1-2)."""
    from stylegan_directions_face_reenactment_amd import flame as FL
    m = TF._module(SEED)
    c = S.synthetic_flame_coeffs(SEED, 'flame.sw.rows', 40, [0.3 * ((i % 7) - 3) for i in range(40)])
    with torch.no_grad():
        whole = FL.decode(m, TF._cuda(c))
        for lo, hi in ((0, 16), (16, 40)):
            part = FL.decode(m, TF._cuda({k: v[lo:hi] for k, v in c.items()}))
            for a, b, what in zip(whole, part, ('landmarks2d', 'landmarks3d', 'trans_verts')):
                assert a.shape[0] == 40 and b.shape[0] == hi - lo
                assert torch.equal(a[lo:hi], b), (what, lo, hi, float((a[lo:hi] - b).abs().max()))

"""Writes tests/golden/kat21_fan3d.npz from the reference's own landmark class beyond the 2D branch (libs/face_models/
landmarks_estimation.py:155-181 flip_input and the 3D type, fan_model/utils.py flip / shuffle_lr / draw_gaussian / _gaussian,
fan_model/models.py ResNetDepth).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_fan3d.py        (CPU only, a few minutes)

cv2, torchvision and the S3FD detector package are stubbed in sys.modules as scripts/make_golden_fan.py does (none of the stubbed
names is called on this path).  FAN(4) loads the seeded state of kat13 (synthetic.synthetic_fan_state at kat13's seed), ResNetDepth
the state of synthetic.synthetic_fan_depth_state; both run in fp64 and in fp32 on the CPU.  Cases: kat13's 'a', kat13's geometry 'b' and the
B = 2 case 'c' of tests/fan3d_restatement.py, whose boxes differ in scale by a factor of two; 'b' and 'c' with images under seeds of
their own (fan3d_restatement.IMAGE_SEEDS).  The crop in front is kat13's.

The file holds seeds, the reference module's key -> shape list, and per case and mode ('plain', 'flip'): arg-max, top-2 values and
3 x 3 neighbourhoods of the decoded heatmaps in fp64 (top-2 in fp32 too), two full maps of row 0 of the flip sum, dev = the reference's own max
|fp32 - fp64| on them, pts, pts_img, boxes; the drawn maps as their non-zero bounding box, the 13 x 13 window from its corner, the
count and the exact sum of the non-zero values (every value outside the box is zero, so this pins every bit); the same for the
injected points of fan3d_restatement.edge_points; per ResNetDepth tap (plain mode) mean, mean |.| and 64 values in fp64 with the
reference's own max |fp32 - fp64|; depth, its deviation, the z factor and pts_img3 per mode; and the reference's flip sum on an
injected pair of heatmaps as a strided sample with exact row and column sums.

The script ASSERTS on the flip sum what make_golden_fan.py asserts on the plain heatmaps (decisions beyond 16 x dev, truncations
1e-3 from an integer, a border and an interior maximum per case).  If an assertion fails, change an image seed, not the assertion.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
import fan_restatement as R                                                       # noqa: E402
import fan3d_restatement as R3                                                    # noqa: E402
import make_golden_fan as G13                                                     # noqa: E402

DEPTH_SEED = 20261020
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat21_fan3d.npz')
KAT13 = os.path.join(ROOT, 'tests', 'golden', 'kat13_fan.npz')
FULL = (9, 48)                                 # the flip sums of row 0 stored in full
CASES = ('a', 'b', 'c')


def depth_reference(model, x):
    taps, hooks = {'layer': []}, []
    hooks.append(model.maxpool.register_forward_pre_hook(lambda m, a: taps.__setitem__('stem', a[0].detach().clone())))
    hooks.append(model.maxpool.register_forward_hook(lambda m, a, o: taps.__setitem__('pool', o.detach().clone())))
    for i in range(4):
        hooks.append(getattr(model, 'layer%d' % (i + 1)).register_forward_hook(lambda m, a, o: taps['layer'].append(o.detach().clone())))
    hooks.append(model.avgpool.register_forward_hook(lambda m, a, o: taps.__setitem__('feat', o.detach().flatten(1).clone())))
    with torch.no_grad():
        taps['depth'] = model(x)
    for h in hooks:
        h.remove()
    return taps


def main():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    sys.path.insert(0, ref)
    G13._stub_imports()
    from libs.face_models.fan_model.models import FAN, ResNetDepth
    from libs.face_models import landmarks_estimation as LE
    from libs.face_models.fan_model.utils import transform, flip, draw_gaussian
    torch.manual_seed(0)
    seed = int(np.load(KAT13)['seed'])
    fan = FAN(4)
    fan.load_state_dict(S.synthetic_fan_state(seed), strict=True)
    fan.eval()
    depth_net = ResNetDepth()
    depth_net.load_state_dict(S.synthetic_fan_depth_state(DEPTH_SEED), strict=True)
    depth_net.eval()
    keys = ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in depth_net.state_dict().items()]
    assert len(keys) == 932
    out = {'seed': np.int64(seed), 'depth_seed': np.int64(DEPTH_SEED), 'depth_keys': np.array(keys), 'full': np.array(FULL, dtype=np.int64)}

    def draw_reference(pts):
        """landmarks_estimation.py:166-171 per row."""
        maps = torch.zeros((pts.shape[0], 68, 256, 256), dtype=torch.float32)
        for b in range(pts.shape[0]):
            for i in range(68):
                if pts[b, i, 0] > 0:
                    maps[b, i] = draw_gaussian(maps[b, i], pts[b, i], 2)
        return maps

    # ---- the flip sum and draw_gaussian on injected inputs
    hm2 = S.counter_tensor(seed, 'fan3d.flip.hm2', (2, 68, 64, 64))
    fsum = hm2[:1] + flip(hm2[1:], is_label=True)
    out['flipadd_sub'] = fsum[0, :, ::8, ::8].numpy()
    out['flipadd_rowsum'] = fsum[0].double().sum(2).numpy()
    out['flipadd_colsum'] = fsum[0].double().sum(1).numpy()
    edge = R3.edge_points()
    for k, v in zip(('box', 'win', 'count', 'sum'), R3.map_digest(draw_reference(edge))):
        out['draw_%s_edge' % k] = v
    n_drawn = int((out['draw_count_edge'] > 0).sum())
    print('injected points: %d of %d maps drawn' % (n_drawn, edge.shape[0] * 68))

    for name in CASES:
        x, faces = R3.case_inputs(S, seed, name)
        B = x.shape[0]
        centres, scales, wins = [], [], []
        for b in range(B):                               # LandmarksEstimation.get_landmarks :145-150, one face at a time
            face = faces[b]
            center = torch.FloatTensor([(face[2] + face[0]) / 2.0, (face[3] + face[1]) / 2.0])
            center[1] = center[1] - (face[3] - face[1]) * 0.12
            scale = (face[2] - face[0] + face[3] - face[1]) / 195.0
            l1 = transform([1, 1], center, scale, 256.0, True)
            l2 = transform([256.0, 256.0], center, scale, 256.0, True)
            centres.append(center), scales.append(scale)
            wins.append([int(l1[0]), int(l1[1]), int(l2[0]), int(l2[1])])
        assert wins == R.windows(faces), (wins, R.windows(faces))
        c64, s64 = R.centre_scale(faces.double())
        for b in range(B):                               # the window corners are decisive
            for p in ([1.0, 1.0], [256.0, 256.0]):
                pre = R.inv_transform_float(torch.tensor(p, dtype=torch.float64), c64[b], s64[b], 256.0)
                assert float((pre - pre.round()).abs().min()) >= 1e-3, (name, b, p, pre)
        crop64 = torch.cat([G13.F_resize(R.window_of(x[b].double(), wins[b])) for b in range(B)]) / 255.0
        crop32 = torch.cat([G13.F_resize(R.window_of(x[b], wins[b])) for b in range(B)]) / 255.0
        out['faces_' + name] = faces.numpy()
        out['scale_' + name] = torch.stack(scales).numpy()
        out['zfac_' + name] = torch.stack([1.0 / (256.0 / (200.0 * s)) for s in scales]).numpy()
        assert out['zfac_' + name].dtype == np.float32
        with torch.no_grad():
            heat = {}
            for dt, crop in ((torch.float32, crop32), (torch.float64, crop64)):
                model = fan.to(dt)
                plain = model(crop)[-1]
                heat[dt] = {'plain': plain, 'flip': plain + flip(model(flip(crop))[-1], is_label=True)}      # :155-159
        for mode in ('plain', 'flip'):
            tag = '%s_%s' % (mode, name)
            hm32, hm64 = heat[torch.float32][mode], heat[torch.float64][mode]
            dev = float((hm32.double() - hm64).abs().max())
            out['dev_heatmaps_' + tag] = np.asarray(dev)
            pts, pts_img, pts32, pts_img32 = [], [], [], []
            for b in range(B):
                p, pi = LE.get_preds_fromhm(hm64[b:b + 1].clone(), centres[b], scales[b])
                pts.append(p.view(-1, 68, 2) * 4), pts_img.append(pi.view(-1, 68, 2))
                p, pi = LE.get_preds_fromhm(hm32[b:b + 1].clone(), centres[b], scales[b])
                pts32.append(p.view(-1, 68, 2) * 4), pts_img32.append(pi.view(-1, 68, 2))
            pts, pts_img = torch.cat(pts), torch.cat(pts_img)
            assert torch.equal(torch.cat(pts_img32), pts_img) and torch.equal(torch.cat(pts32), pts)     # fp32 and fp64 agree
            flat = hm64.reshape(B, 68, -1)
            top2, idx2 = flat.topk(2, dim=2)
            idx = idx2[..., 0]
            assert torch.equal(idx, flat.argmax(2)) and torch.equal(idx, hm32.reshape(B, 68, -1).argmax(2))
            margin = float((top2[..., 0] - top2[..., 1]).min())
            assert margin > 16 * dev, (tag, margin, dev)
            d = R.decode(hm64, faces)
            assert torch.equal(d['idx'], idx) and torch.equal(d['pts'], pts.float()) and torch.equal(d['pts_img'], pts_img.float())
            inner = d['interior']
            assert bool(inner.any()) and bool((~inner).any()), (tag, int(inner.sum()))
            nb = float(torch.minimum(d['dx'].abs(), d['dy'].abs())[inner].min())
            assert nb > 16 * dev, (tag, nb, dev)
            pre64 = torch.stack([R.inv_transform_float((d['pts'][b] / 4).double(), c64[b], s64[b], 64.0) for b in range(B)])
            frac = float((pre64 - pre64.round()).abs().min())
            assert frac >= 1e-3, (tag, frac)
            assert torch.equal(pre64.trunc().float(), pts_img.float())
            print('case %s: dev %.3e, top-2 margin %.1f x, neighbour difference %.1f x, %d of %d maxima interior, coordinates >= %.2e from '
                  'an integer' % (tag, dev, margin / dev, nb / dev, int(inner.sum()), inner.numel(), frac))
            nbh = torch.full((B, 68, 3, 3), float('nan'), dtype=torch.float64)
            py, px = idx // 64, idx % 64
            for b in range(B):
                for j in range(68):
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            yy, xx = int(py[b, j]) + dy, int(px[b, j]) + dx
                            if 0 <= yy < 64 and 0 <= xx < 64:
                                nbh[b, j, dy + 1, dx + 1] = hm64[b, j, yy, xx]
            out['argmax_' + tag] = idx.numpy()
            out['top2_' + tag] = top2.numpy()
            out['top2_f32_' + tag] = hm32.reshape(B, 68, -1).topk(2, dim=2).values.numpy()
            out['nbh_' + tag] = nbh.numpy()
            if mode == 'flip':
                out['heatmaps_full_' + tag] = hm64[0, list(FULL)].numpy()
            out['pts_' + tag] = pts.float().numpy()
            out['pts_img_' + tag] = pts_img.float().numpy()
            out['boxes_' + tag] = torch.cat([pts_img.min(1).values, pts_img.max(1).values], 1).float().numpy()
            # ---- the 3D type behind the decode (:165-181), one row at a time
            pts4 = pts.float()
            assert float(pts4.min()) >= 1 and float(pts4.max()) <= 255 and torch.equal(pts4, pts4.round())
            maps = draw_reference(pts4)
            for k, v in zip(('box', 'win', 'count', 'sum'), R3.map_digest(maps)):
                out['draw_%s_%s' % (k, tag)] = v
            with torch.no_grad():
                t32 = depth_reference(depth_net.float(), torch.cat((crop32, maps), 1))
                t64 = depth_reference(depth_net.double(), torch.cat((crop64, maps.double()), 1))
            for (tap, t), (_, u) in zip(R3.tap_list(t64), R3.tap_list(t32)):
                dv = float((u.double() - t).abs().max())
                out['dev_%s_%s' % (tap, tag)] = np.asarray(dv)
                if mode == 'plain' or tap == 'depth':
                    out['tap_%s_%s' % (tap, tag)] = R3.tap_checksum(t)
                if mode == 'plain':
                    print('case %s tap %-7s mean %.4g, max |.| %.4g, dev %.3e' % (tag, tap, float(t.mean()), float(t.abs().max()), dv))
            depth = t64['depth']
            out['depth_' + tag] = depth.numpy()
            rows = []
            for b in range(B):                           # :179-181
                rows.append(torch.cat((pts_img[b], depth[b].view(68, 1) * (1.0 / (256.0 / (200.0 * scales[b])))), 1))
            out['pts_img3_' + tag] = torch.stack(rows).double().numpy()
            print('case %s: depth %.3g .. %.3g, dev_depth %.3e' % (tag, float(depth.min()), float(depth.max()), float(out['dev_depth_' + tag])))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) <= os.path.getsize(KAT13)


if __name__ == '__main__':
    main()

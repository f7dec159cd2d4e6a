"""Writes tests/golden/kat13_fan.npz from the reference's own landmark network and decode (libs/face_models/fan_model/models.py
FAN(4), landmarks_estimation.py get_preds_fromhm, fan_model/utils.py transform).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_fan.py        (CPU only, a few minutes)

models.py imports torch only.  landmarks_estimation.py and fan_model/utils.py import cv2, torchvision and the S3FD detector package
at module level; those are stubbed in sys.modules (none of the stubbed names is called on this path).  The network loads the seeded
state of synthetic.synthetic_fan_state and runs in fp64 and in fp32 on the CPU, one call per case; centre and scale follow
LandmarksEstimation.get_landmarks (:145-150) in float32.  The crop in front restates crop_torch with tests/fan_restatement.py's zero
window and F.interpolate(bilinear, align_corners=False) in place of torchvision's Resize (unverified against torchvision), with
the window corners taken from the reference's own transform.

The file holds the seed, the reference module's key -> shape list, and per case: faces, centre / scale / window corners, per heatmap
the arg-max index, the two largest values and the 3 x 3 neighbourhood of the maximum (fp64, NaN outside the map), eight full
heatmaps of row 0 (fp64), per debug tap (mean, mean |.|, an 8 x 8 window) in fp64 and the reference's own max |fp32 - fp64|, pts,
pts_img, boxes and dev_heatmaps = the reference's own max |fp32 - fp64| on the last heatmaps.  Images are regenerated from keys,
not stored.

The script ASSERTS that the fixture is decisive, so that exact comparisons of the landmarks are fair: for every heatmap the top-2
margin and, for interior maxima, both neighbour differences exceed 16 x dev_heatmaps; every coordinate of both transform calls is
at least 1e-3 away from an integer before truncation (in fp64); each case has a maximum on the border and one in the interior.  If
an assertion fails, change the seed or the synthetic state, not the assertion.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
import fan_restatement as R                                                       # noqa: E402

SEED = 20261208
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat13_fan.npz')
FULL = (0, 9, 17, 27, 36, 48, 57, 67)          # the heatmaps of row 0 stored in full


def _stub_imports():
    cv2 = types.ModuleType('cv2')
    tv, tr = types.ModuleType('torchvision'), types.ModuleType('torchvision.transforms')
    tv.transforms = tr
    det = types.ModuleType('libs.face_models.sfd.sfd_detector')
    det.SFDDetector = type('SFDDetector', (), {})
    sys.modules.update({'cv2': cv2, 'torchvision': tv, 'torchvision.transforms': tr, 'libs.face_models.sfd.sfd_detector': det})


def run_reference(model, crop):
    """The reference module's outputs and the debug taps, by hooks."""
    taps, hooks = {}, []
    hooks.append(model.conv2.register_forward_pre_hook(lambda m, a: taps.__setitem__('stem', a[0].detach().clone())))
    hooks.append(model.conv4.register_forward_hook(lambda m, a, o: taps.__setitem__('conv4', o.detach().clone())))
    for i in range(4):
        hooks.append(getattr(model, 'm%d' % i).register_forward_hook(lambda m, a, o, i=i: taps.__setitem__('hg%d' % i, o.detach().clone())))
        hooks.append(getattr(model, 'l%d' % i).register_forward_hook(lambda m, a, o, i=i: taps.__setitem__('heatmaps%d' % i, o.detach().clone())))
    with torch.no_grad():
        out = model(crop)
    for h in hooks:
        h.remove()
    assert len(out) == 4 and torch.equal(out[-1], taps['heatmaps3'])
    return out[-1], taps


def main():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    sys.path.insert(0, ref)
    _stub_imports()
    from libs.face_models.fan_model.models import FAN
    from libs.face_models import landmarks_estimation as LE
    from libs.face_models.fan_model.utils import transform
    torch.manual_seed(0)
    sd = S.synthetic_fan_state(SEED)
    model = FAN(4)
    model.load_state_dict(sd, strict=True)
    model.eval()
    keys = ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in model.state_dict().items()]
    assert len(keys) == 1129
    out = {'seed': np.int64(SEED), 'keys': np.array(keys), 'full': np.array(FULL, dtype=np.int64)}
    for name in R.CASES:
        x, faces = R.fixture_inputs(S, SEED, name)
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
        crop64 = torch.cat([F_resize(R.window_of(x[b].double(), wins[b])) for b in range(B)]) / 255.0
        crop32 = torch.cat([F_resize(R.window_of(x[b], wins[b])) for b in range(B)]) / 255.0
        hm32, taps32 = run_reference(model.float(), crop32)
        hm64, taps64 = run_reference(model.double(), crop64)
        dev = float((hm32.double() - hm64).abs().max())
        out['dev_heatmaps_' + name] = np.asarray(dev)
        for tap, t in taps64.items():
            out['tap_%s_%s' % (tap, name)] = R.tap_checksum(t)
            out['dev_%s_%s' % (tap, name)] = np.asarray(float((taps32[tap].double() - t).abs().max()))
        # the reference's decode, one row at a time as get_landmarks runs it
        pts, pts_img, pts32 = [], [], []
        for b in range(B):
            p, pi = LE.get_preds_fromhm(hm64[b:b + 1].clone(), centres[b], scales[b])
            pts.append(p.view(-1, 68, 2) * 4), pts_img.append(pi.view(-1, 68, 2))
            pts32.append(LE.get_preds_fromhm(hm32[b:b + 1].clone(), centres[b], scales[b])[1].view(-1, 68, 2))
        pts, pts_img = torch.cat(pts), torch.cat(pts_img)
        assert torch.equal(torch.cat(pts32), pts_img)                      # fp32 and fp64 agree on every landmark
        # decisiveness
        flat = hm64.reshape(B, 68, -1)
        top2, idx2 = flat.topk(2, dim=2)
        idx = idx2[..., 0]
        assert torch.equal(idx, flat.argmax(2)) and torch.equal(idx, hm32.reshape(B, 68, -1).argmax(2))
        margin = float((top2[..., 0] - top2[..., 1]).min())
        assert margin > 16 * dev, (name, margin, dev)
        d = R.decode(hm64, faces)
        assert torch.equal(d['idx'], idx) and torch.equal(d['pts'], pts.float()) and torch.equal(d['pts_img'], pts_img.float())
        inner = d['interior']
        assert bool(inner.any()) and bool((~inner).any()), (name, int(inner.sum()))
        nb = float(torch.minimum(d['dx'].abs(), d['dy'].abs())[inner].min())
        assert nb > 16 * dev, (name, nb, dev)
        pre64 = torch.stack([R.inv_transform_float((d['pts'][b] / 4).double(), c64[b], s64[b], 64.0) for b in range(B)])
        frac = float((pre64 - pre64.round()).abs().min())
        assert frac >= 1e-3, (name, frac)
        assert torch.equal(pre64.trunc().float(), pts_img.float())
        print('case %s: dev_heatmaps %.3e, top-2 margin %.1f x, neighbour difference %.1f x, %d of %d maxima interior, coordinates >= %.2e '
              'from an integer' % (name, dev, margin / dev, nb / dev, int(inner.sum()), inner.numel(), frac))
        nbh = torch.full((B, 68, 3, 3), float('nan'), dtype=torch.float64)
        py, px = idx // 64, idx % 64
        for b in range(B):
            for j in range(68):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = int(py[b, j]) + dy, int(px[b, j]) + dx
                        if 0 <= yy < 64 and 0 <= xx < 64:
                            nbh[b, j, dy + 1, dx + 1] = hm64[b, j, yy, xx]
        out['faces_' + name] = faces.numpy()
        out['centre_' + name] = torch.stack(centres).numpy()
        out['scale_' + name] = torch.stack(scales).numpy()
        out['window_' + name] = np.array(wins, dtype=np.int64)
        out['argmax_' + name] = idx.numpy()
        out['top2_' + name] = top2.numpy()
        out['nbh_' + name] = nbh.numpy()
        out['heatmaps_full_' + name] = hm64[0, list(FULL)].numpy()
        out['heatmaps_max_' + name] = np.asarray(float(hm64.abs().max()))
        out['pts_' + name] = pts.float().numpy()
        out['pts_img_' + name] = pts_img.float().numpy()
        out['boxes_' + name] = torch.cat([pts_img.min(1).values, pts_img.max(1).values], 1).float().numpy()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


def F_resize(window):
    return torch.nn.functional.interpolate(window[None], size=(256, 256), mode='bilinear', align_corners=False)


if __name__ == '__main__':
    main()

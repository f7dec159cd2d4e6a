"""Writes tests/golden/kat19_paired_losses.npz from the reference's own functions, run on CPU tensors with torch autograd.

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_paired.py        (CPU only, a second)

image_utils imports cv2 and torchvision at its top and uses neither in torch_range_1_to_255; two empty stub modules stand in for
them.  What is called: libs.utilities.image_utils.torch_range_1_to_255, libs.criteria.losses.Losses().calculate_pixel_wise_loss
and torch.nn.L1Loss, as utils_train.py:438-439, :488 and :493-494 call them.

The file holds arrays only.  Inputs: images x, y [2,3,32,32] ~ N(0, 0.8^2) (about a fifth of x leaves [-1,1]) with planted pixels --
x = +1 and x = -1 exactly (the clamp's bounds pass gradient), x = 1.5 / y = 2 and x = -2 / y = -1 (x clamped: gradient exactly 0),
two pixels with x == y inside the range (sign(0) = 0: only the image gradient passes) -- a weight image c, and latents lat, tw
[2,14,512] with a few equal entries.  Recorded: t(x), t(y), pw = the pixel-wise loss of them, wreg = L1Loss(lat, tw), the gradient
of 0.37 pw + sum(c t(x)) with respect to x (sum(c t(x)) stands in for a loss that reads the transformed image, as LPIPS does) and
of 0.61 wreg with respect to lat.  The script ASSERTS that tests/pair_loss_restatement.py meets every array at the tests' bars.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pair_loss_restatement as R                                                 # noqa: E402

SEED = 20261019
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat19_paired_losses.npz')
G_PW, G_WREG = 0.37, 0.61
# (n, c, h, w) of the planted pixels
BOUND = ((0, 0, 0, 0, 1.0), (0, 0, 0, 1, -1.0))
CLAMPED = ((0, 0, 0, 2, 1.5, 2.0), (0, 0, 0, 3, -2.0, -1.0))
EQUAL = ((1, 1, 5, 5, 0.25), (1, 2, 7, 9, -0.5))


def _reference():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref or not os.path.isdir(ref):
        raise SystemExit('set SGDFR_REFERENCE to a checkout of the reference')
    for name in ('cv2', 'torchvision'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['cv2'].INTER_AREA = 3                   # a default argument of image_resize, read when the module is loaded
    sys.path.insert(0, ref)
    from libs.criteria.losses import Losses
    from libs.utilities.image_utils import torch_range_1_to_255
    return torch_range_1_to_255, Losses()


def _flat(shape, idx):
    return int(np.ravel_multi_index(idx, shape))


def main():
    to255, losses = _reference()
    rng = np.random.default_rng(SEED)
    shape = (2, 3, 32, 32)
    x = rng.normal(0, 0.8, shape).astype(np.float32)
    y = rng.normal(0, 0.8, shape).astype(np.float32)
    for n, c, h, w, v in BOUND:
        x[n, c, h, w] = v
    for n, c, h, w, vx, vy in CLAMPED:
        x[n, c, h, w], y[n, c, h, w] = vx, vy
    for n, c, h, w, v in EQUAL:
        x[n, c, h, w] = y[n, c, h, w] = v
    cw = rng.normal(0, 1, shape).astype(np.float32)
    lat = rng.normal(0, 1, (2, 14, 512)).astype(np.float32)
    tw = rng.normal(0, 1, (2, 14, 512)).astype(np.float32)
    tw[0, 0, :3] = lat[0, 0, :3]
    tw[1, 13, 500:] = lat[1, 13, 500:]

    xt, yt, ct = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y), torch.from_numpy(cw)
    x_before = xt.detach().clone()
    tx, ty = to255(xt), to255(yt)
    assert torch.equal(xt.detach(), x_before)                                     # the reference clones: its input is not modified
    pw = losses.calculate_pixel_wise_loss(tx, ty.detach())
    (G_PW * pw + (ct * tx).sum()).backward()
    lt, twt = torch.from_numpy(lat).requires_grad_(True), torch.from_numpy(tw)
    wreg = torch.nn.L1Loss()(lt, twt)
    (G_WREG * wreg).backward()

    out = {'x': x, 'y': y, 'c': cw, 'lat': lat, 'tw': tw, 'tx': tx.detach().numpy(), 'ty': ty.detach().numpy(),
           'pw': np.float32(pw.item()), 'wreg': np.float32(wreg.item()), 'g_pw': np.float32(G_PW), 'g_wreg': np.float32(G_WREG),
           'gx': xt.grad.numpy(), 'glat': lt.grad.numpy(),
           'bound_idx': np.array([_flat(shape, p[:4]) for p in BOUND], dtype=np.int64),
           'clamped_idx': np.array([_flat(shape, p[:4]) for p in CLAMPED], dtype=np.int64),
           'equal_idx': np.array([_flat(shape, p[:4]) for p in EQUAL], dtype=np.int64)}

    outside = float(((x < -1) | (x > 1)).mean())
    print('x outside [-1,1]: %.3f of %d pixels; pw %.6f, wreg %.6f' % (outside, x.size, out['pw'], out['wreg']))
    assert 0.15 < outside < 0.27
    # the restatement meets the reference at the tests' bars
    et = max(float((R.t(xt.detach()) - tx.detach().double()).abs().max()), float((R.t(yt) - ty.double()).abs().max()))
    ep = abs(float(R.pixel_wise(xt.detach(), yt)) - pw.item()) / pw.item()
    ew = abs(float(R.l1_mean(lt.detach(), twt)) - wreg.item()) / wreg.item()
    eg = R.rel(R.pixel_wise_grad(xt.detach(), yt, G_PW, ct), xt.grad)
    el = R.rel(R.l1_mean_grad(lt.detach(), twt, G_WREG), lt.grad)
    print('restatement against the reference: t %.3e (bar %.3e), pw %.3e, wreg %.3e (bar %.0e), gx %.3e, glat %.3e (bar %.0e)'
          % (et, R.T_ABS, ep, ew, R.MEAN_REL, eg, el, R.GRAD_REL))
    assert et <= R.T_ABS and ep <= R.MEAN_REL and ew <= R.MEAN_REL and eg <= R.GRAD_REL and el <= R.GRAD_REL
    gx = xt.grad.reshape(-1)
    assert (gx[out['clamped_idx']] == 0).all() and (gx[out['bound_idx']] != 0).all()
    assert torch.equal(gx[out['equal_idx']], (ct.reshape(-1)[out['equal_idx']] * 255.0) / np.float32(2 + 1e-5))
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()

"""Plain-torch restatement, in float64, of the paired step's own loss arithmetic (pair_loss.py, csrc/pairloss.hip): the
[-1,1] -> [0,255] transform t of libs/utilities/image_utils.py:87-94, the two means of utils_train.py:488, :494 and their gradients in
closed form.  It is the yardstick at sizes tests/golden/kat19_paired_losses.npz does not hold; tests/test_cpu_pair_loss.py holds it to
that fixture.  Every function takes tensors on any device and computes in float64.

The divisor is the float32 value of 2 + 1e-5: the reference divides a float32 tensor by that Python scalar, which torch rounds to
the tensor's type first.  (Against the real number 2.00001 the transform would sit 1.7e-6 lower at 255.)
"""
import numpy as np
import torch

SPAN = float(np.float32(2 + 1e-5))
S = 255.0 / SPAN

# the bars of the issue, shared by the CPU and GPU tests
T_ABS = 255 * 2.0 ** -22            # t(x): three roundings after the exact clamp, and a device may multiply by 1/SPAN
MEAN_REL = 2e-6                     # a tree sum of <= 2^22 float32 terms plus t's roundings: (log2 n + 4) 2^-24
GRAD_REL = 1e-6                     # of the gradient's largest element


def t(v):
    return (v.double().clamp(-1, 1) + 1) / SPAN * 255


def l1_mean(a, b):
    return (a.double() - b.double()).abs().mean()


def pixel_wise(x, y):
    """losses.py:14-18 on the transformed images: L1Loss(t(y), t(x))."""
    return (t(y) - t(x)).abs().mean()


def l1_mean_grad(a, b, g):
    """d(g * l1_mean)/da; sign(0) = 0 as torch's L1Loss backward."""
    return g * torch.sign(a.double() - b.double()) / a.numel()


def pixel_wise_grad(x, y, g, g255=None):
    """d(g * pixel_wise(x, y) + sum(g255 * t(x)))/dx: m(x) * s * (g255 + g * sign(t(x) - t(y)) / n), m = 1 on -1 <= x <= 1."""
    xd = x.double()
    up = g * torch.sign(t(x) - t(y)) / x.numel()
    if g255 is not None:
        up = up + g255.double()
    return ((xd >= -1) & (xd <= 1)).double() * S * up


def rel(got, want):
    """max |got - want| over max |want|, in float64 on want's device."""
    want = want.detach().double()
    got = got.detach().double().to(want.device)
    return float((got - want).abs().max() / want.abs().max())

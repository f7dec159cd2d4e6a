"""The stock expression of the pooled image loss (stylegan_directions_face_reenactment_amd/pool_loss.py, csrc/sweep.hip), in any
dtype on any device: F.adaptive_avg_pool2d -> F.mse_loss, dx by autograd.  fp64 on the CPU is the yardstick of the GPU tests and
the same expression in fp32 on the same inputs gives their bar."""
import torch
import torch.nn.functional as F


def forward(x, real, P):
    """(pooled [B,3,P,P], mse 0-d) of x [B,3,P*f,P*f] against real [B,3,P,P]."""
    pooled = F.adaptive_avg_pool2d(x, (P, P))
    return pooled, F.mse_loss(pooled, real)


def backward(x, real, P, g_pooled=None, g_mse=None):
    """dx of sum(pooled * g_pooled) + mse * g_mse; a gradient given as None is left out."""
    x = x.detach().clone().requires_grad_(True)
    pooled, mse = forward(x, real, P)
    total = 0
    if g_pooled is not None:
        total = total + (pooled * g_pooled).sum()
    if g_mse is not None:
        total = total + mse * g_mse
    return torch.autograd.grad(total, x)[0]

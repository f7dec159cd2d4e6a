"""The pooled image loss of PTI above 256^2: the generator's [B,3,P*f,P*f] image pooled f x f to [B,3,P,P] (AdaptiveAvgPool2d
((P,P)), as generic.generate_image pools above 256: generic.py:146-148) and its MSE against the real [B,3,P,P] crop, in one walk
over the image (``sgdfr_pool_mse_f32``), with the gradient of both outputs back onto the image in one launch
(``sgdfr_pool_mse_bwd_f32``).  `pooled` has the bits of reenact.pool_images(x, P); `mse` is reduced without float atomics and has
the same bits from call to call.  No host synchronisation; the workspace comes from the torch allocator, so the pair can be
captured (functional.capture_graph)."""
import torch

from . import _native as N


def _shapes(who, x, real, P):
    """(B, P, f) of x [B,3,P*f,P*f] against real [B,3,P,P]; ValueError for anything else."""
    if not torch.is_tensor(x) or not torch.is_tensor(real):
        raise ValueError('%s: expected tensors, got %s and %s' % (who, type(x).__name__, type(real).__name__))
    if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= 8192:
        raise ValueError('%s: P must be an int in 1..8192, got %r' % (who, P))
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[0] < 1:
        raise ValueError('%s: expected square RGB images [B,3,S,S], got %s' % (who, tuple(x.shape)))
    B, S = x.shape[0], x.shape[2]
    if tuple(real.shape) != (B, 3, P, P):
        raise ValueError('%s: the real images must be [%d,3,%d,%d], got %s' % (who, B, P, P, tuple(real.shape)))
    f = S // P if S % P == 0 else 0
    if f not in (1, 2, 4):
        raise ValueError('%s: images of side %d do not pool to %d by a factor of 1, 2 or 4' % (who, S, P))
    if B > 4096:
        raise ValueError('%s: 1..4096 images, got %d' % (who, B))
    return B, P, f


def pool_mse_backward(g_pooled, pooled, real, g_mse, f, out=None):
    """dx [B,3,P*f,P*f] = (g_pooled + g_mse * 2 (pooled - real) / (3 B P^2)) / f^2 spread over every f x f window: one launch of
    ``sgdfr_pool_mse_bwd_f32``.  g_pooled [B,3,P,P] and g_mse (one element on the device) may each be None.  `out`: where to write
    (contiguous; 16-byte stores when it is 16-byte aligned and P*f is a multiple of 4, dword stores of the same values otherwise)."""
    B, _, P, _ = pooled.shape
    N.require_device(g_pooled, pooled, real, g_mse, out)
    if f not in (1, 2, 4):
        raise ValueError('pool_mse_backward: the pooling factor must be 1, 2 or 4, got %r' % (f,))
    if out is None:
        out = torch.empty((B, 3, P * f, P * f), dtype=torch.float32, device=pooled.device)
    elif tuple(out.shape) != (B, 3, P * f, P * f) or not out.is_contiguous():
        raise ValueError('pool_mse_backward: out must be contiguous [%d,3,%d,%d], got %s' % (B, P * f, P * f, tuple(out.shape)))
    for t in (g_pooled, pooled, real):
        if t is not None and (tuple(t.shape) != (B, 3, P, P) or not t.is_contiguous()):
            raise ValueError('pool_mse_backward: expected contiguous [%d,3,%d,%d], got %s' % (B, P, P, tuple(t.shape)))
    if g_mse is not None and g_mse.numel() != 1:
        raise ValueError('pool_mse_backward: g_mse is one element, got %s' % (tuple(g_mse.shape),))
    N.call('sgdfr_pool_mse_bwd_f32', N.ptr(g_pooled), N.ptr(pooled), N.ptr(real), N.ptr(g_mse), B, P, f, N.ptr(out), N.stream())
    return out


class PoolMse(torch.autograd.Function):
    """(x [B,3,P*f,P*f], real [B,3,P,P], P) -> (pooled [B,3,P,P], mse 0-d): PoolMse.apply(x, real, P).  The gradient goes to x only
    (a `real` that requires grad is refused); an output nobody uses has no gradient, which the backward kernel takes as NULL."""

    @staticmethod
    def forward(ctx, x, real, P):
        B, P, f = _shapes('PoolMse', x, real, P)
        if real.requires_grad:
            raise ValueError('PoolMse: the real images get no gradient; detach them')
        N.require_device(x, real)
        x, real = N.f32c(x.detach()), N.f32c(real.detach())
        pooled = torch.empty((B, 3, P, P), dtype=torch.float32, device=x.device)
        mse = torch.empty(1, dtype=torch.float32, device=x.device)
        ws, nbytes = N.workspace('sgdfr_pool_mse_workspace_bytes', x.device, B, P, error='PoolMse: unsupported shape B=%d P=%d' % (B, P))
        N.call('sgdfr_pool_mse_f32', N.ptr(x), N.ptr(real), B, P, f, N.ptr(pooled), N.ptr(mse), N.ptr(ws), nbytes, N.stream())
        ctx.save_for_backward(pooled, real)
        ctx.f = f
        ctx.set_materialize_grads(False)        # an unused output's gradient arrives as None, not as zeros
        return pooled, mse.view(())

    @staticmethod
    def backward(ctx, g_pooled, g_mse):
        pooled, real = ctx.saved_tensors
        if g_pooled is None and g_mse is None:
            return None, None, None
        if g_pooled is not None:
            g_pooled = N.f32c(g_pooled.to(torch.float32))
        if g_mse is not None:
            g_mse = g_mse.reshape(1).to(torch.float32).contiguous()
        return pool_mse_backward(g_pooled, pooled, real, g_mse, ctx.f), None, None


def pool_mse(x, real, P):
    """PoolMse.apply(x, real, P)."""
    return PoolMse.apply(x, real, P)

"""The loss arithmetic that only the paired training step has, on the HIP kernels of csrc/pairloss.hip -- DESIGN.md section 4.22.
Counterparts:

  * ``torch_range_1_to_255``   libs/utilities/image_utils.py:87-94 (clone, clamp to [-1,1], +1, /(2+1e-5), *255)
  * ``l1_mean``                torch.nn.L1Loss() as utils_train.py:493-494 uses it on the latents
  * ``pixel_wise_255``         utils_train.py:438-439 with losses.py:14-18: both transforms and the L1 of the transformed images

    loss, x255, y255 = pixel_wise_255(imgs_shifted, imgs_target, want_images=True)     # one pass; LPIPS reads x255, y255
    w_reg = l1_mean(shifted_latents, target_w)

Stock torch spends about a dozen elementwise and reduction launches on these and as many in the backward.  Here a forward is
one streaming launch and a fixed-order finish, a backward is one launch: pixel_wise_255 is ONE autograd.Function whose backward
takes the gradients of `loss` and of `x255` together.  Every result and every upstream gradient is a device tensor; nothing
synchronises.  Gradient reaches the first argument only, as everywhere in this package's losses.
"""
import torch

from . import _native as N

INT_MAX = 2 ** 31 - 1
# how many 0..255 images this module has materialised (tests read it: a paired step without LPIPS must not write any)
COUNTERS = {'images_255': 0}


def _check(name, a, b):
    N.require_device(a, b)
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError('%s: the two arguments differ in shape, %s and %s' % (name, tuple(a.shape), tuple(b.shape)))
    if a.numel() == 0:
        raise ValueError('%s: empty tensors %s' % (name, tuple(a.shape)))
    if b.requires_grad and torch.is_grad_enabled():
        raise RuntimeError('%s: no gradient with respect to the second argument; pass it detached' % name)


def _forward(x, y, mode, x255=None, y255=None):
    n = x.numel()
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    ws, nbytes = N.workspace('sgdfr_pairloss_workspace_bytes', x.device, min(n, INT_MAX), error='pair_loss: empty input')
    N.call('sgdfr_pairloss_forward_f32', N.ptr(x), N.ptr(y), n, mode, N.ptr(x255), N.ptr(y255), N.ptr(loss), N.ptr(ws), nbytes,
           N.stream())
    return loss.view(())


def _backward(x, y, mode, gloss, g255):
    g = None if gloss is None else gloss.reshape(1).to(torch.float32).contiguous()
    g255 = None if g255 is None else N.f32c(g255.to(torch.float32))
    dx = torch.empty_like(x)
    N.call('sgdfr_pairloss_backward_f32', N.ptr(x), N.ptr(y), x.numel(), mode, N.ptr(g), N.ptr(g255), N.ptr(dx), N.stream())
    return dx


class _PairLossFn(torch.autograd.Function):
    """(loss, x255, y255) of one forward pass; the images are None where not wanted (mode PLAIN never has them).  backward: one
    launch from the gradients of loss and x255 (either may be absent); y255 is a constant of the graph."""

    @staticmethod
    def forward(ctx, x, y, mode, want_images):
        ctx.set_materialize_grads(False)            # an output nobody used arrives as None, not as an image of zeros
        x255 = torch.empty_like(x) if want_images else None
        y255 = torch.empty_like(y) if want_images else None
        loss = _forward(x, y, mode, x255, y255)
        if want_images:
            COUNTERS['images_255'] += 2
            ctx.mark_non_differentiable(y255)
        ctx.save_for_backward(x, y)
        ctx.mode = mode
        return loss, x255, y255

    @staticmethod
    def backward(ctx, gloss, g255, _gy255):
        x, y = ctx.saved_tensors
        return _backward(x, y, ctx.mode, gloss, g255), None, None, None


def _pair(name, a, b):
    _check(name, a, b)
    return N.f32c(a), N.f32c(b.detach())


def l1_mean(a, b):
    """mean |a - b| (torch.nn.L1Loss()) of two float32 device tensors of one shape -> 0-d tensor; gradient goes to `a` only."""
    x, y = _pair('l1_mean', a, b)
    return _PairLossFn.apply(x, y, N.PAIRLOSS_PLAIN, False)[0]


def pixel_wise_255(imgs_shifted, imgs_target, want_images=False):
    """(loss, x255 | None, y255 | None): loss = L1Loss(t(imgs_target), t(imgs_shifted)) with t = torch_range_1_to_255, as
    utils_train.py:438-439, 488 with losses.py:14-18; with want_images the two transformed images come from the same pass (x255
    carries gradient back to imgs_shifted through this Function, y255 is a constant).  imgs_target gets no gradient."""
    x, y = _pair('pixel_wise_255', imgs_shifted, imgs_target)
    return _PairLossFn.apply(x, y, N.PAIRLOSS_RANGE255, bool(want_images))


class _Range255Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        out = torch.empty_like(x)
        # (the pass forms |t(x) - t(x)| = 0 beside the image; its mean is discarded)
        _forward(x, x, N.PAIRLOSS_RANGE255, out, None)
        COUNTERS['images_255'] += 1
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g255):
        x, = ctx.saved_tensors
        return _backward(x, x, N.PAIRLOSS_RANGE255, None, g255)


def torch_range_1_to_255(image):
    """image_utils.py:87-94 for a float32 device tensor: a new tensor, differentiable; the input is never modified."""
    N.require_device(image)
    if image.numel() == 0:
        raise ValueError('torch_range_1_to_255: empty tensor %s' % (tuple(image.shape),))
    return _Range255Fn.apply(N.f32c(image))

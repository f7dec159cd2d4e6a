"""LPIPS (AlexNet, v0.1) on the HIP kernels of csrc/lpips.hip: the counterpart of libs/criteria/lpips/lpips.py with its
networks.py / utils.py, without torchvision and without the URL download of the `lin` weights.

    lpips = LPIPS().cuda(); lpips.load_state_dict(sd)      # sd: this module's keys, torchvision alexnet's or alex.pth's
    loss = lpips(x, y)                                      # dL/dx through autograd; y is a constant
    tgt = lpips.target(y); loss = lpips(x, tgt)             # y's features computed once (PTI: 200 steps against one image)

The state dict keys are the reference's (`net.mean`, `net.std`, `net.layers.{0,3,6,8,10}.{weight,bias}`, `lin.{0..4}.1.weight`);
every parameter is frozen as in the reference (networks.py:33,85).  The forward runs x and a live y through the same launches
as one batch of 2B images; the backward forms dL/dx only.  The library handle stays in _native (modules stay deep-copyable and
picklable); the weight pack is rebuilt whenever a parameter's storage or version changes, like ModulatedConv2d.packed().
"""
from collections import OrderedDict

import torch
from torch import nn

from . import _native as N
from .packs import PackedWeights

CHANNELS = (64, 192, 384, 256, 256)
CONV_INDICES = (0, 3, 6, 8, 10)


def _alexnet_features():
    """torchvision.models.alexnet().features: the module layout (and so the state-dict keys) the reference loads."""
    c = CHANNELS
    return nn.Sequential(
        nn.Conv2d(3, c[0], 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
        nn.Conv2d(c[0], c[1], 5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
        nn.Conv2d(c[1], c[2], 3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(c[2], c[3], 3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(c[3], c[4], 3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2))


class AlexNet(nn.Module):
    """networks.py BaseNet + AlexNet: z-score buffers and the `features` stack (weights only; the HIP kernels run it)."""

    def __init__(self):
        super().__init__()
        self.register_buffer('mean', torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('std', torch.Tensor([.458, .448, .450])[None, :, None, None])
        self.layers = _alexnet_features()
        self.target_layers = [2, 5, 8, 10, 12]
        self.n_channels_list = list(CHANNELS)
        for p in self.parameters():
            p.requires_grad = False


class LinLayers(nn.ModuleList):
    """networks.py LinLayers: per tap a 1x1 conv to one channel, no bias, frozen."""

    def __init__(self, n_channels_list):
        super().__init__([nn.Sequential(nn.Identity(), nn.Conv2d(nc, 1, 1, 1, 0, bias=False)) for nc in n_channels_list])
        for p in self.parameters():
            p.requires_grad = False


def convert_state_dict(state_dict):
    """This module's keys from any of the three formats on disk: this module's own (= the reference LPIPS's), torchvision alexnet's
    (`features.N.*`; `classifier.*` is dropped) and PerceptualSimilarity's alex.pth (`lin{i}.model.1.weight`, renamed as
    lpips/utils.py:28-33 does) -- or the two partial ones merged.  Returns (dict, set of key groups present: 'net', 'lin')."""
    out, groups = OrderedDict(), set()
    for k, v in state_dict.items():
        if k.startswith('classifier.'):
            continue
        if k.startswith('features.'):
            k = 'net.layers.' + k[len('features.'):]
        elif k.startswith('lin') and '.model.' in k:             # lin0.model.1.weight -> lin.0.1.weight
            k = 'lin.' + k[3:].replace('model.', '')
        elif k[:1].isdigit() and k.endswith('.1.weight'):        # the already renamed alex.pth (utils.get_state_dict)
            k = 'lin.' + k
        if k.startswith('net.layers.'):
            groups.add('net')
        elif k.startswith('lin.'):
            groups.add('lin')
        out[k] = v
    return out, groups


class LpipsTarget:
    """The five tap features of a fixed comparison image y (LPIPS.target): PTI compares every generated image with one real
    image, and the reference recomputes that image's features on every step."""

    def __init__(self, feats, rows, H, W, source, pack_key):
        self.feats, self.rows, self.H, self.W = feats, rows, H, W
        self.source = source                        # the image tensor (for PtiLoss's staleness checks)
        self.source_version = source._version
        self.pack_key = pack_key


def _workspace(B, H, W, device):
    return N.workspace('sgdfr_lpips_workspace_bytes', device, B, H, W, error='LPIPS: unsupported image size %dx%d' % (H, W))


def _features(pack, x, y, H, W):
    """Taps of x's rows followed by y's rows (y may be None) -> feature buffer."""
    rows = x.shape[0] + (0 if y is None else y.shape[0])
    n = N.size('sgdfr_lpips_feature_elems', rows, H, W, error='LPIPS: unsupported image size %dx%d' % (H, W))
    feats = torch.empty(n, dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(max(x.shape[0], (rows + 1) // 2), H, W, x.device)
    N.call('sgdfr_lpips_features_f32', N.ptr(x), x.shape[0], N.ptr(y), 0 if y is None else y.shape[0], H, W, N.ptr(pack), N.ptr(feats),
           N.ptr(ws), nbytes, N.stream())
    return feats


class _LpipsFn(torch.autograd.Function):
    """loss = LPIPS(x, y) on the HIP kernels; backward: dL/dx only (y and the frozen weights get no gradient).
    y: a live image tensor, or (feats, rows) of a cached target."""

    @staticmethod
    def forward(ctx, x, pack, y, y_feats, y_rows):
        B, _, H, W = x.shape
        if y is not None:
            feats = _features(pack, x, y, H, W)
            fy, rows_y, y_row0 = feats, 2 * B, B
            bcast = 0
        else:
            feats = _features(pack, x, None, H, W)
            fy, rows_y, y_row0 = y_feats, y_rows, 0
            bcast = int(y_rows == 1 and B > 1)
        rows_x = B if y is None else 2 * B
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ws, nbytes = _workspace(B, H, W, x.device)
        N.call('sgdfr_lpips_distance_f32', N.ptr(feats), rows_x, N.ptr(fy), rows_y, y_row0, bcast, B, H, W, N.ptr(pack), N.ptr(loss),
               N.ptr(ws), nbytes, N.stream())
        ctx.save_for_backward(feats, fy, pack)
        ctx.meta = (B, H, W, rows_x, rows_y, y_row0, bcast)
        return loss.view(())

    @staticmethod
    def backward(ctx, gloss):
        feats, fy, pack = ctx.saved_tensors
        B, H, W, rows_x, rows_y, y_row0, bcast = ctx.meta
        g = gloss.reshape(1).to(torch.float32).contiguous()
        dx = torch.empty((B, 3, H, W), dtype=torch.float32, device=feats.device)
        ws, nbytes = _workspace(B, H, W, feats.device)
        N.call('sgdfr_lpips_backward_f32', N.ptr(g), N.ptr(feats), rows_x, N.ptr(fy), rows_y, y_row0, bcast, B, H, W, N.ptr(pack),
               N.ptr(dx), N.ptr(ws), nbytes, N.stream())
        return dx, None, None, None, None


class LPIPS(PackedWeights, nn.Module):
    r"""Learned Perceptual Image Patch Similarity, AlexNet v0.1 (lpips.py:8-34): forward(x, y) -> scalar
    (1/B) sum over taps and images of the spatially averaged, lin-weighted squared difference of channel-normalised features.
    x, y: [B,3,H,W] fp32 GPU images in [-1,1] (no resize), or y = LPIPS.target(...)."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_lpips_prepack_f32', 'sgdfr_lpips_pack_elems', N.LPIPS_PARAMS
    # no TRAIN_ERROR: the network has no BatchNorm and no Dropout, train mode changes nothing
    GRAD_ERROR = ('LPIPS: the HIP kernels give no gradient for the LPIPS weights; keep every parameter at '
                  'requires_grad=False (as the reference does)')

    def __init__(self, net_type: str = 'alex', version: str = '0.1'):
        if net_type != 'alex':
            raise NotImplementedError('LPIPS: only net_type="alex" has HIP kernels (got %r)' % (net_type,))
        if version != '0.1':
            raise NotImplementedError('LPIPS: only version 0.1 (got %r)' % (version,))
        super().__init__()
        self.net = AlexNet()
        self.lin = LinLayers(self.net.n_channels_list)

    # ---- weights
    def folded(self):
        """The 17 tensors sgdfr_lpips_prepack_f32 takes: nothing is folded, they are the state dict's own entries in the pack's order."""
        L = self.net.layers
        ps = []
        for i in CONV_INDICES:
            ps += [L[i].weight, L[i].bias]
        ps += [self.net.mean, self.net.std] + [self.lin[t][1].weight for t in range(5)]
        return [p.detach().contiguous() for p in ps]

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """Accepts this module's keys, torchvision alexnet's (`features.N.*`) and PerceptualSimilarity's alex.pth
        (`lin{i}.model.1.weight`); a dict holding only one of the two halves loads that half (strictly, with strict=True)."""
        sd, groups = convert_state_dict(state_dict)
        if groups:              # the z-score constants (networks.py:55-58) are not in either on-disk format
            for k in ('net.mean', 'net.std'):
                sd.setdefault(k, getattr(self.net, k[4:]))
        if groups == {'net', 'lin'} or not groups:
            return super().load_state_dict(sd, strict=strict, **kwargs)
        else:
            own = self.state_dict()
            prefix = 'net.layers.' if groups == {'net'} else 'lin.'
            need = {k for k in own if k.startswith(prefix)}
            extra = set(sd) - set(own)
            if strict and (need - set(sd) or extra):
                raise RuntimeError('LPIPS.load_state_dict: missing %s, unexpected %s' % (sorted(need - set(sd)), sorted(extra)))
            merged = OrderedDict(own)
            merged.update({k: v for k, v in sd.items() if k in own})
            return super().load_state_dict(merged, strict=True, **kwargs)

    # ---- forward
    def _check(self, x):
        self.check()
        N.require_device(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('LPIPS: expected [B,3,H,W] images, got %s' % (tuple(x.shape),))

    @torch.no_grad()
    def target(self, y):
        """Features of a fixed comparison image y [By,3,H,W] (By = 1 is compared with every image of x)."""
        self._check(y)
        y = N.f32c(y.detach())
        feats = _features(self.packed(), y, None, y.shape[2], y.shape[3])
        return LpipsTarget(feats, y.shape[0], y.shape[2], y.shape[3], y, self._key())

    def forward(self, x, y):
        self._check(x)
        x = N.f32c(x)
        pack = self.packed()
        if isinstance(y, LpipsTarget):
            if y.pack_key != self._key():
                raise RuntimeError('LPIPS: the target was computed with other weights; call target() again')
            if (y.H, y.W) != tuple(x.shape[2:]) or y.rows not in (1, x.shape[0]):
                raise ValueError('LPIPS: target of %d images %dx%d against x %s' % (y.rows, y.H, y.W, tuple(x.shape)))
            return _LpipsFn.apply(x, pack, None, y.feats, y.rows)
        self._check(y)
        if y.requires_grad and torch.is_grad_enabled():
            raise RuntimeError('LPIPS: no gradient with respect to y; pass y.detach()')
        if y.shape != x.shape:
            raise ValueError('LPIPS: x %s and y %s differ in shape' % (tuple(x.shape), tuple(y.shape)))
        return _LpipsFn.apply(x, pack, N.f32c(y.detach()), None, 0)

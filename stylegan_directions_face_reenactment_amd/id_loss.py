"""ArcFace identity loss (IR-SE-50) on the HIP kernels of csrc/idloss.hip: the counterpart of libs/criteria/id_loss.py with its
model_irse.py / helpers.py.

    idl = IDLoss('model_ir_se50.pth').cuda().eval()         # or IDLoss() + idl.facenet.load_state_dict(sd)
    loss = idl(y_hat, y)                                    # (1 - cos(e(y_hat), e(y).detach())).mean(); dL/dy_hat via autograd
    tgt = idl.target(y); loss = idl(y_hat, tgt)             # y's embeddings computed once
    e = idl.extract_feats(x)                                # [B,512] unit-norm, differentiable to x

`Backbone` has the module layout and state-dict keys of model_irse.Backbone(112, 50, 'ir_se', 0.6) and holds the weights only;
the HIP kernels run it in eval mode (running BatchNorm statistics, Dropout off).  The reference leaves the facenet's parameters
trainable but never reads their gradients (its optimiser holds the direction matrix only); here they are frozen at construction,
and re-enabling requires_grad or calling facenet.train() (batch-statistics BatchNorm) raises before any launch.

x and a live y run through the same launches as one batch of B + B_y rows; activations are saved only for x's rows and only
when a gradient is needed (nothing under torch.no_grad(): CSIM evaluation).  y is detached silently, as the reference detaches
y's embeddings.  The cosine and the mean stay in torch on [B,512] (nn.CosineSimilarity(dim=1, eps=1e-6), as the reference calls
it), so autograd supplies dL/de.  Every BatchNorm is folded into the weights on the host in fp64, once per weight version; the
device pack (forward and input-gradient weights, ~2 x 175 MB) is rebuilt whenever a parameter's storage or version changes.
"""
from collections import OrderedDict

import torch
from torch import nn

from . import _native as N
from .encoder import ResidualUnit, _TRUNK
from .packs import PackedWeights, views

EMB = 512


class Backbone(PackedWeights, nn.Module):
    """model_irse.Backbone(input_size=112, num_layers=50, mode='ir_se', drop_ratio=0.6): weights only.  forward(x) runs the HIP
    kernels on [B,3,112,112] faces (AdaptiveAvgPool2d(112) is the identity there), returning l2-normalised [B,512] embeddings."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_idloss_prepack_f32', 'sgdfr_idloss_pack_elems', N.IDLOSS_PARAMS
    TRAIN_ERROR = ('IDLoss: the HIP kernels run the facenet in eval mode only (running BatchNorm statistics); '
                   'call facenet.eval()')
    GRAD_ERROR = ('IDLoss: the HIP kernels give no gradient for the facenet weights; keep every parameter at '
                  'requires_grad=False (the reference never reads them)')

    def __init__(self, input_size=112, num_layers=50, mode='ir_se', drop_ratio=0.6, affine=True):
        if (input_size, num_layers, mode, affine) != (112, 50, 'ir_se', True):
            raise NotImplementedError('Backbone: only input_size=112, num_layers=50, mode="ir_se", affine=True have HIP kernels '
                                      '(got %r, %r, %r, %r)' % (input_size, num_layers, mode, affine))
        super().__init__()
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(512), nn.Dropout(drop_ratio), nn.Flatten(),
                                          nn.Linear(512 * 7 * 7, 512), nn.BatchNorm1d(512, affine=affine))
        units, c = [], 64
        for depth, n in _TRUNK[50]:
            for u in range(n):
                units.append(ResidualUnit(c, depth, 2 if u == 0 else 1, True))
                c = depth
        self.body = nn.Sequential(*units)
        for p in self.parameters():
            p.requires_grad = False

    # ---- weights
    def folded(self, dtype=torch.float32):
        """The 245 tensors sgdfr_idloss_prepack_f32 takes (None for the shortcut conv of an identity unit), every BatchNorm
        folded in fp64 on the parameters' device, returned in `dtype`."""
        def bn(m):
            s = m.weight.detach().double() * torch.rsqrt(m.running_var.detach().double() + m.eps)
            return s, m.bias.detach().double() - m.running_mean.detach().double() * s

        out = []
        conv, bn0, prelu = self.input_layer
        s, t = bn(bn0)
        out += [conv.weight.detach().double() * s.view(-1, 1, 1, 1), t, prelu.weight.detach().double()]
        for unit in self.body:
            bn1, c1, pr, c2, bn2, se = unit.res_layer
            s1, t1 = bn(bn1)
            s2, t2 = bn(bn2)
            d = c2.weight.shape[0]
            out += [s1, t1, c1.weight.detach().double(), pr.weight.detach().double(), c2.weight.detach().double() * s2.view(-1, 1, 1, 1),
                    t2, se.fc1.weight.detach().double().reshape(d // 16, d), se.fc2.weight.detach().double().reshape(d, d // 16)]
            if isinstance(unit.shortcut_layer, nn.Sequential):
                sc, scbn = unit.shortcut_layer
                ss, st = bn(scbn)
                out += [sc.weight.detach().double().reshape(d, -1) * ss.view(-1, 1), st]
            else:
                out += [None, None]
        bn2d, _, _, lin, bn1d = self.output_layer
        s, t = bn(bn2d)
        q, r = bn(bn1d)
        hw = 7 * 7
        W = lin.weight.detach().double()
        sk, tk = s.repeat_interleave(hw), t.repeat_interleave(hw)           # BN2d per flattened index c*49 + hw
        out += [q.view(-1, 1) * W * sk.view(1, -1), q * (W @ tk + lin.bias.detach().double()) + r]
        return [None if v is None else v.to(dtype).contiguous() for v in out]

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """model_ir_se50.pth's keys, or the same with an `facenet.` prefix (an IDLoss state dict)."""
        sd = OrderedDict((k[len('facenet.'):] if k.startswith('facenet.') else k, v) for k, v in state_dict.items())
        return super().load_state_dict(sd, strict=strict, **kwargs)

    def forward(self, x):
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, 112, 112):
            raise ValueError('Backbone: expected [B,3,112,112] faces, got %s' % (tuple(x.shape),))
        return embed(self, x, crop=False)[0]


def _check_image(x, what):
    N.require_device(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError('IDLoss: expected [B,3,H,W] images for %s, got %s' % (what, tuple(x.shape)))


def _workspace(rows, H, W, device):
    return N.workspace('sgdfr_idloss_workspace_bytes', device, rows, H, W, error='IDLoss: unsupported image size %dx%d' % (H, W))


def _forward(pack, x, y, crop, save):
    """Embeddings of x's rows followed by y's rows (y may be None) -> (emb [R,512], saved or None)."""
    B, _, H, W = x.shape
    rows_y = 0 if y is None else y.shape[0]
    emb = torch.empty((B + rows_y, EMB), dtype=torch.float32, device=x.device)
    saved = torch.empty(N.load().sgdfr_idloss_saved_elems(B), dtype=torch.float32, device=x.device) if save else None
    ws, nbytes = _workspace(B + rows_y, H, W, x.device)
    N.call('sgdfr_idloss_forward_f32', N.ptr(x), B, N.ptr(y), rows_y, H, W, int(crop), N.ptr(pack), N.ptr(emb), N.ptr(saved),
           N.ptr(ws), nbytes, N.stream())
    return emb, saved


class _IdFn(torch.autograd.Function):
    """(e(x), e(y)) on the HIP kernels; backward: dL/dx only (y and the frozen weights get no gradient)."""

    @staticmethod
    def forward(ctx, x, pack, y, crop, save):
        emb, saved = _forward(pack, x, y, crop, save)
        B = x.shape[0]
        if save:
            ctx.save_for_backward(saved, pack)
        ctx.meta = (B, x.shape[2], x.shape[3], crop)
        ey = emb[B:]
        ctx.mark_non_differentiable(ey)
        return emb[:B], ey

    @staticmethod
    def backward(ctx, gex, gey):
        saved, pack = ctx.saved_tensors
        B, H, W, crop = ctx.meta
        g = gex.to(torch.float32).contiguous()
        dx = torch.empty((B, 3, H, W), dtype=torch.float32, device=g.device)
        ws, nbytes = _workspace(B, H, W, g.device)
        N.call('sgdfr_idloss_backward_f32', N.ptr(g), N.ptr(saved), B, H, W, int(crop), N.ptr(pack), N.ptr(dx), N.ptr(ws), nbytes,
               N.stream())
        return dx, None, None, None, None


def embed(facenet, x, y=None, crop=True):
    """(e(x), e(y)) of the HIP backbone in one pass (y may be None: e(y) is then [0,512]); e(x) is differentiable to x."""
    facenet.check()
    _check_image(x, 'x')
    x = N.f32c(x)
    if y is not None:
        _check_image(y, 'y')
        if tuple(y.shape[2:]) != tuple(x.shape[2:]) or y.shape[0] not in (1, x.shape[0]):
            raise ValueError('IDLoss: y %s against x %s (y needs 1 or B rows of the same size)' % (tuple(y.shape), tuple(x.shape)))
        y = N.f32c(y.detach())
    save = torch.is_grad_enabled() and x.requires_grad      # nothing is kept for a forward without a gradient
    return _IdFn.apply(x, facenet.packed(), y, bool(crop), save)


def saved_views(saved, rows):
    """The saved buffer of a forward with `rows` x rows as named views (the layout of csrc/idloss.hip's SavedLayout): p0 (stem
    pre-activation), per unit p1 (conv1 output before PReLU), c2 (conv2 + BN2), gate (g [D] then h [D/16] per row), hv (e, |v|)."""
    out, take = {'p1': [], 'c2': [], 'gate': []}, views(saved, rows)

    out['p0'] = take((64, 112, 112))
    c, h = 64, 112
    for depth, n in _TRUNK[50]:
        for u in range(n):
            ho = (h - 1) // 2 + 1 if u == 0 else h
            out['p1'].append(take((depth, h, h)))
            out['c2'].append(take((depth, ho, ho)))
            out['gate'].append(take((depth + depth // 16,)))
            c, h = depth, ho
    out['hv'] = take((EMB + 1,))
    take.done()
    return out


class IdTarget:
    """The embeddings of a fixed comparison image y (IDLoss.target)."""

    def __init__(self, feats, H, W, crop, source, pack_key):
        self.feats, self.H, self.W, self.crop = feats, H, W, crop
        self.source = source
        self.source_version = source._version
        self.pack_key = pack_key


class IDLoss(nn.Module):
    r"""libs/criteria/id_loss.py on the HIP backbone: forward(y_hat, y, crop=True) -> (1 - cos(e(y_hat), e(y).detach())).mean().
    y_hat, y: [B,3,H,W] fp32 GPU images (y may have one row: compared with every row of y_hat), or y = IDLoss.target(...)."""

    def __init__(self, pretrained_model_path=None):
        super().__init__()
        self.facenet = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')
        if pretrained_model_path is not None:
            self.facenet.load_state_dict(torch.load(pretrained_model_path, map_location='cpu'))
        self.facenet.eval()
        self.criterion = nn.CosineSimilarity(dim=1, eps=1e-6)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """An IDLoss state dict (`facenet.*`) or a bare model_ir_se50.pth one."""
        return self.facenet.load_state_dict(state_dict, strict=strict, **kwargs)

    def extract_feats(self, x, crop=True):
        """[B,512] unit-norm embeddings of crop -> AdaptiveAvgPool2d(112) -> facenet, differentiable to x."""
        return embed(self.facenet, x, None, crop)[0]

    @torch.no_grad()
    def target(self, y, crop=True):
        """Embeddings of a fixed comparison image y [By,3,H,W], computed once."""
        self.facenet.check()
        _check_image(y, 'y')
        yd = N.f32c(y.detach())
        emb, _ = _forward(self.facenet.packed(), yd, None, bool(crop), False)
        return IdTarget(emb, y.shape[2], y.shape[3], bool(crop), y, self.facenet._key())

    def forward(self, y_hat, y, crop=True):
        if isinstance(y, IdTarget):
            self.facenet.check()
            if y.pack_key != self.facenet._key():
                raise RuntimeError('IDLoss: the target was computed with other weights; call target() again')
            if y.source._version != y.source_version:
                raise RuntimeError('IDLoss: the target image was modified in place after target(); call target() again')
            if bool(crop) != y.crop or (y.H, y.W) != tuple(y_hat.shape[2:]):
                raise ValueError('IDLoss: target of %dx%d (crop=%s) against y_hat %s (crop=%s)' % (y.H, y.W, y.crop, tuple(y_hat.shape), crop))
            y_feats = y.feats
            y_hat_feats = self.extract_feats(y_hat, crop)
        else:
            y_hat_feats, y_feats = embed(self.facenet, y_hat, y, crop)
        if y_feats.shape[0] not in (1, y_hat_feats.shape[0]):
            raise ValueError('IDLoss: %d target rows against %d images' % (y_feats.shape[0], y_hat_feats.shape[0]))
        cosine_sim = self.criterion(y_hat_feats, y_feats.detach())
        return torch.mean(1 - cosine_sim)

"""e4e W+ producer: the step *before* the generator path in the inference flow.

`Encoder4Editing(50, 'ir_se', 256)` maps aligned faces `[B,3,256,256]` in [-1,1] to W+ codes `[B,14,512]`
(reference: libs/gan/encoder4editing/psp_encoders.py:122-199 on the IR-SE-50 trunk of helpers.py:25-112; built at
run_inference.py:74-79 and invert_images.py:63-70).  The state_dict key set is the reference's
(`input_layer.*`, `body.N.{shortcut_layer,res_layer}.*`, `styles.N.{convs.M,linear}.*`, `latlayer{1,2}.*`) so an
e4e checkpoint loads unchanged.

Convolutions run on MIOpen through PyTorch-ROCm (stock 3x3/1x1 convs; nothing here is a modulated conv); what is
specific to this build:

  * inference plan (`no_grad` + `eval()`): every conv->BatchNorm pair (second conv of each unit, shortcut
    projection, stem) is folded into one conv with bias, activations are kept channels-last for MIOpen's NHWC
    kernels, and the plan is cached until a parameter changes;
  * the 14 style heads are evaluated as 3 groups (coarse / middle / fine share their input feature map): the
    first conv of a group is one conv with the heads' filters concatenated, the following stride-2 convs (per-head
    filters on 8x8 ... 1x1 maps) are an unfold + one batched GEMM per depth, and the 14 `EqualLinear`s run on the HIP
    linear kernel (`sgdfr_linear_f32`);
  * like the reference (psp_encoders.py:185-199) no `latent_avg` is added; the generator applies truncation.

Beside that, `encode(enc, images)` runs the whole encoder on the hand-written kernels of csrc/e4e.hip (exact-f32 MFMA implicit
GEMM, forward only, one stream, no host synchronisation); `Encoder4Editing.forward` itself stays on the MIOpen plan.

`image_resolution` and the side of the input are two numbers (psp_encoders.py:143-156, 171-199): the first only sets
`style_count` = 2 log2(image_resolution) - 2 (14, 16, 18 heads for the 256, 512, 1024 generators), the input is the 256 x 256
alignment crop for all three.  `input_size` is the side the HIP path is built for; its default min(image_resolution, 256) is the
old meaning of every construction up to 256.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from . import _native as N
from .model import EqualLinear
from .packs import PackedWeights, views

# (depth, units) of the four trunk stages; the first unit of a stage has stride 2 (helpers.py:29-36, num_layers=50)
_TRUNK = {50: ((64, 3), (128, 4), (256, 14), (512, 3)),
          100: ((64, 3), (128, 13), (256, 30), (512, 3)),
          152: ((64, 3), (128, 8), (256, 36), (512, 3))}


class SEModule(nn.Module):
    """Channel gate x * sigmoid(fc2(relu(fc1(mean_hw x)))) (helpers.py:57-74)."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, channels // reduction, 1, bias=False)
        self.fc2 = nn.Conv2d(channels // reduction, channels, 1, bias=False)

    def forward(self, x):
        g = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.fc2(F.relu(self.fc1(g))))


class ResidualUnit(nn.Module):
    """BN -> conv3x3 -> PReLU -> conv3x3(stride) -> BN [-> SE]  +  shortcut (helpers.py:77-121).
    The shortcut is a strided subsample when in == depth (the reference's MaxPool2d(1, stride)), else 1x1 conv + BN."""

    def __init__(self, in_channel, depth, stride, se):
        super().__init__()
        self.stride = stride
        if in_channel == depth:
            self.shortcut_layer = nn.MaxPool2d(1, stride)
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(in_channel, depth, 1, stride, bias=False),
                                                nn.BatchNorm2d(depth))
        layers = [nn.BatchNorm2d(in_channel), nn.Conv2d(in_channel, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                  nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth)]
        if se:
            layers.append(SEModule(depth, 16))
        self.res_layer = nn.Sequential(*layers)

    def forward(self, x):
        return self.res_layer(x) + self.shortcut_layer(x)


class GradualStyleBlock(nn.Module):
    """log2(spatial) stride-2 conv3x3 + LeakyReLU(0.01) down to 1x1, then EqualLinear (psp_encoders.py:33-53)."""

    def __init__(self, in_c, out_c, spatial):
        super().__init__()
        self.out_c, self.spatial = out_c, spatial
        mods, c = [], in_c
        for _ in range(int(math.log2(spatial))):
            mods += [nn.Conv2d(c, out_c, 3, 2, 1), nn.LeakyReLU()]
            c = out_c
        self.convs = nn.Sequential(*mods)
        self.linear = EqualLinear(out_c, out_c, lr_mul=1)

    def forward(self, x):
        return self.linear(self.convs(x).view(-1, self.out_c))


def _fold(conv, bn):
    """conv (no bias) followed by eval-mode BatchNorm == conv with scaled filters and a bias."""
    g = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    return (conv.weight * g.view(-1, 1, 1, 1)).contiguous(memory_format=torch.channels_last), bn.bias - bn.running_mean * g


class Encoder4Editing(PackedWeights, nn.Module):
    PREPACK, PACK_ELEMS = 'sgdfr_e4e_prepack_n_f32', 'sgdfr_e4e_pack_elems_n'
    TRAIN_ERROR = 'encode: the module is in train() mode; the HIP path folds the BatchNorm statistics, call .eval() first'
    # no GRAD_ERROR: the module's own forward trains; encode() is forward only and returns no graph
    WRAP_STATE_DICT = False         # a checkpoint's `_metadata` decides how its BatchNorms load: the dict is passed on as it comes

    def __init__(self, num_layers, mode='ir', image_resolution=256, input_size=None):
        super().__init__()
        if num_layers not in _TRUNK:
            raise ValueError('num_layers should be 50, 100 or 152, got %r' % (num_layers,))
        if mode not in ('ir', 'ir_se'):
            raise ValueError("mode should be 'ir' or 'ir_se', got %r" % (mode,))
        self.num_layers, self.mode, self.image_resolution = num_layers, mode, image_resolution
        # the side encode() takes: the reference feeds every encoder the 256 x 256 crop, whatever the generator renders
        self.input_size = min(image_resolution, 256) if input_size is None else input_size
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        units, c = [], 64
        for depth, n in _TRUNK[num_layers]:
            for u in range(n):
                units.append(ResidualUnit(c, depth, 2 if u == 0 else 1, mode == 'ir_se'))
                c = depth
        self.body = nn.Sequential(*units)
        # feature taps after these trunk units (psp_encoders.py:171-177): 128ch @ /4, 256ch @ /8, 512ch @ /16
        self._taps = (6, 20, 23)
        self.style_count = 2 * int(math.log2(image_resolution)) - 2
        self.coarse_ind, self.middle_ind = 3, 7
        self.styles = nn.ModuleList(
            GradualStyleBlock(512, 512, 16 if i < self.coarse_ind else 32 if i < self.middle_ind else 64)
            for i in range(self.style_count))
        self.latlayer1 = nn.Conv2d(256, 512, 1)
        self.latlayer2 = nn.Conv2d(128, 512, 1)
        self._plan_key, self._plan = None, None

    # ------------------------------------------------------------------ reference-shaped (autograd-capable) forward
    def _features(self, x):
        x = self.input_layer(x)
        taps = []
        for i, unit in enumerate(self.body):
            x = unit(x)
            if i in self._taps:
                taps.append(x)
        c1, c2, c3 = taps
        p2 = F.interpolate(c3, size=c2.shape[2:], mode='bilinear', align_corners=True) + self.latlayer1(c2)
        p1 = F.interpolate(p2, size=c1.shape[2:], mode='bilinear', align_corners=True) + self.latlayer2(c1)
        return c3, p2, p1

    def _groups(self):
        n = self.style_count
        return ((0, min(self.coarse_ind, n)), (min(self.coarse_ind, n), min(self.middle_ind, n)),
                (min(self.middle_ind, n), n))

    def forward(self, x):
        """[B,3,R,R] -> W+ [B,style_count,512]: w0 from the coarse map for every row, plus one delta per row > 0
        (the reference's `Inference` progressive stage, psp_encoders.py:185-199)."""
        if not (self.training or torch.is_grad_enabled()):
            return self._forward_planned(x)
        feats = self._features(x)
        rows = []
        for (lo, hi), f in zip(self._groups(), feats):
            rows += [self.styles[j](f) for j in range(lo, hi)]
        w0 = rows[0]
        return torch.stack([w0] + [w0 + d for d in rows[1:]], dim=1)

    # ------------------------------------------------------------------ inference plan
    def _state_key(self):
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def invalidate_packs(self):
        """Drop the folded inference plan with the HIP weight pack (needed only after in-place `.data` edits, which the version
        counters behind `_state_key` and `_key` do not see)."""
        self._plan_key, self._plan = None, None
        super().invalidate_packs()

    def _load_from_state_dict(self, *args, **kwargs):
        """Also drops the packs when the encoder is loaded as a part of a larger module, whose load_state_dict is not ours."""
        super()._load_from_state_dict(*args, **kwargs)
        self.invalidate_packs()

    def folded(self, dtype=torch.float32):
        return folded(self, dtype)

    def _prepack_plan(self, ps):
        R, n, lib = self.input_size, self.style_count, N.load()
        count = lib.sgdfr_e4e_param_count_n(R, n)
        if count != len(ps):
            raise RuntimeError('encode: %d folded tensors, the kernels expect %d for %d heads at an input of %d' % (len(ps), count, n, R))
        return count, (R, n), (R, n)

    def _build_plan(self):
        cl = torch.channels_last
        plan = {'stem': _fold(self.input_layer[0], self.input_layer[1]), 'units': [], 'heads': []}
        for unit in self.body:
            r = unit.res_layer
            bn1 = r[0]
            g1 = bn1.weight * torch.rsqrt(bn1.running_var + bn1.eps)
            entry = {'bn1': (g1.view(1, -1, 1, 1), (bn1.bias - bn1.running_mean * g1).view(1, -1, 1, 1)),
                     'w1': r[1].weight.contiguous(memory_format=cl), 'prelu': r[2].weight,
                     'c2': _fold(r[3], r[4]), 'stride': unit.stride,
                     'se': (r[5].fc1.weight, r[5].fc2.weight) if len(r) > 5 else None,
                     'sc': _fold(unit.shortcut_layer[0], unit.shortcut_layer[1])
                     if isinstance(unit.shortcut_layer, nn.Sequential) else None}
            plan['units'].append(entry)
        for lo, hi in self._groups():
            heads = [self.styles[j] for j in range(lo, hi)]
            if not heads:
                plan['heads'].append(None)
                continue
            depth = len(heads[0].convs) // 2
            # first conv of the group: one conv with the heads' filters concatenated (they share the input map)
            w0 = torch.cat([h.convs[0].weight for h in heads], 0).contiguous(memory_format=cl)
            b0 = torch.cat([h.convs[0].bias for h in heads], 0)
            # deeper stride-2 convs: per-head filters on tiny maps (8x8 ... 1x1) -> unfold + ONE batched GEMM per depth
            # (MIOpen only has its naive kernel for grouped fp32 NHWC convs: measured 100x slower than this)
            deeper = []
            for k in range(1, depth):
                wk = torch.stack([h.convs[2 * k].weight.reshape(h.out_c, -1).t() for h in heads], 0).contiguous()   # [G, Cin*9, Cout]
                bk = torch.stack([h.convs[2 * k].bias for h in heads], 0).unsqueeze(1)                              # [G, 1, Cout]
                deeper.append((wk, bk))
            plan['heads'].append(((w0, b0), deeper, heads))
        return plan

    @torch.no_grad()
    def _forward_planned(self, x):
        key = self._state_key()
        if key != self._plan_key:
            self._plan, self._plan_key = self._build_plan(), key
        plan = self._plan
        x = x.contiguous(memory_format=torch.channels_last)
        x = F.prelu(F.conv2d(x, plan['stem'][0], plan['stem'][1], 1, 1), self.input_layer[2].weight)
        taps = []
        for i, u in enumerate(plan['units']):
            s = u['stride']
            short = x[:, :, ::s, ::s] if u['sc'] is None else F.conv2d(x, u['sc'][0], u['sc'][1], s)
            y = F.conv2d(torch.addcmul(u['bn1'][1], x, u['bn1'][0]), u['w1'], None, 1, 1)
            y = F.conv2d(F.prelu(y, u['prelu']), u['c2'][0], u['c2'][1], s, 1)
            if u['se'] is not None:
                g = torch.sigmoid(F.conv2d(F.relu(F.conv2d(y.mean((2, 3), keepdim=True), u['se'][0])), u['se'][1]))
                x = torch.addcmul(short, y, g)
            else:
                x = y + short
            if i in self._taps:
                taps.append(x)
        c1, c2, c3 = taps
        p2 = F.interpolate(c3, size=c2.shape[2:], mode='bilinear', align_corners=True) + self.latlayer1(c2)
        p1 = F.interpolate(p2, size=c1.shape[2:], mode='bilinear', align_corners=True) + self.latlayer2(c1)
        rows = []
        for f, grp in zip((c3, p2, p1), plan['heads']):
            if grp is None:
                continue
            (w0, b0), deeper, heads = grp
            G, C, B = len(heads), heads[0].out_c, f.shape[0]
            h = F.leaky_relu(F.conv2d(f, w0, b0, 2, 1), 0.01)                                  # [B, G*C, H, W]
            for wk, bk in deeper:
                Hc, Wc = h.shape[2], h.shape[3]
                Ho, Wo = (Hc + 1) // 2, (Wc + 1) // 2
                cols = F.unfold(h.reshape(B * G, C, Hc, Wc), 3, padding=1, stride=2)           # [B*G, C*9, Ho*Wo]
                cols = cols.view(B, G, C * 9, Ho * Wo).permute(1, 0, 3, 2).reshape(G, B * Ho * Wo, C * 9)
                h = F.leaky_relu(torch.baddbmm(bk, cols, wk), 0.01)                            # [G, B*Ho*Wo, C]
                h = h.view(G, B, Ho, Wo, C).permute(1, 0, 4, 2, 3).reshape(B, G * C, Ho, Wo)
            if h.shape[2] != 1 or h.shape[3] != 1:
                raise RuntimeError('style heads expect a %dx%d feature map' % (heads[0].spatial, heads[0].spatial))
            h = h.reshape(B, G, C)                                                             # spatial is 1x1 here
            rows += [head.linear(h[:, j].contiguous()) for j, head in enumerate(heads)]
        w0 = rows[0]
        return torch.stack([w0] + [w0 + d for d in rows[1:]], dim=1)


# ---------------------------------------------------------------------------------------------------------------- HIP path
DEBUG_TAPS = ('stem', 'u0', 'u3', 'c1', 'c2', 'c3', 'p2', 'p1')       # then the head vectors h_coarse, h_middle, h_fine


def _bn_affine(bn):
    g = bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + bn.eps)
    return g, bn.bias.detach().double() - bn.running_mean.detach().double() * g


def _fold64(conv, bn):
    g, h = _bn_affine(bn)
    return conv.weight.detach().double() * g.view(-1, 1, 1, 1), h


def folded(enc, dtype=torch.float32):
    """The tensors sgdfr_e4e_prepack_n_f32 takes, in the order include/sgdfr.h documents, every BatchNorm but BN1 folded into its
    conv in fp64 (BN1 sits in front of a zero-padded conv: it travels as scale and shift).  None where a unit has no shortcut conv."""
    out = list(_fold64(enc.input_layer[0], enc.input_layer[1])) + [enc.input_layer[2].weight.detach().double()]
    for unit in enc.body:
        r = unit.res_layer
        out += list(_bn_affine(r[0])) + [r[1].weight.detach().double(), r[2].weight.detach().double()]
        out += list(_fold64(r[3], r[4])) + [r[5].fc1.weight.detach().double().flatten(1), r[5].fc2.weight.detach().double().flatten(1)]
        if isinstance(unit.shortcut_layer, nn.Sequential):
            w, b = _fold64(unit.shortcut_layer[0], unit.shortcut_layer[1])
            out += [w.flatten(1), b]
        else:
            out += [None, None]
    for lat in (enc.latlayer1, enc.latlayer2):
        out += [lat.weight.detach().double().flatten(1), lat.bias.detach().double()]
    for head in enc.styles:
        for m in head.convs:
            if isinstance(m, nn.Conv2d):
                out += [m.weight.detach().double(), m.bias.detach().double()]
        lin = head.linear
        if lin.activation is not None or lin.lr_mul != 1:
            raise ValueError('encode: the style heads end in EqualLinear(512, 512, lr_mul=1) without activation')
        out += [lin.weight.detach().double() * (1.0 / math.sqrt(lin.weight.shape[1])), lin.bias.detach().double()]
    return [None if v is None else v.to(dtype).contiguous() for v in out]


def _check_module(enc):
    if not isinstance(enc, Encoder4Editing):
        raise TypeError('encode: expected an Encoder4Editing, got %s' % type(enc).__name__)
    if enc.mode != 'ir_se' or enc.num_layers != 50:
        raise ValueError("encode: the HIP path runs Encoder4Editing(50, 'ir_se', R) only, got (%r, %r); use the module's own "
                         'forward for the other trunks' % (enc.num_layers, enc.mode))
    enc.check()
    R = getattr(enc, 'input_size', enc.image_resolution)        # (a module unpickled from before input_size existed)
    if not isinstance(R, int) or isinstance(R, bool) or R % 16 or not 32 <= R <= 256:
        raise ValueError('encode: input size %r is not a multiple of 16 in 32..256 (every style head must end at 1x1)' % (R,))
    n = enc.style_count
    if not isinstance(n, int) or not 8 <= n <= 18 or len(enc.styles) != n:
        raise ValueError('encode: %r style heads (image_resolution %r), the kernels take 8..18 (image_resolution 32..1024)'
                         % (n, enc.image_resolution))
    return R


def packed(enc):
    """The device weight pack of sgdfr_e4e_prepack_n_f32, rebuilt when any parameter's or buffer's storage or version changes."""
    return enc.packed()


def _workspace(rows, R, style_count, device):
    return N.workspace('sgdfr_e4e_workspace_bytes_n', device, rows, R, style_count,
                       error='encode: unsupported batch of %d images at resolution %d (1..256 rows, rows*R*R <= 2^24)' % (rows, R))


def debug_views(debug, rows, R, style_count):
    """The debug buffer as named views (csrc/e4e.hip's DebugLayout): the eight feature taps, then the head vectors in front of the
    EqualLinears as h_coarse [B,3,512], h_middle [B,4,512], h_fine [B,style_count-7,512]."""
    shapes = (('stem', 64, R), ('u0', 64, R // 2), ('u3', 128, R // 4), ('c1', 128, R // 4), ('c2', 256, R // 8), ('c3', 512, R // 16),
              ('p2', 512, R // 8), ('p1', 512, R // 4))
    out, cut = OrderedDict(), views(debug, rows)
    for name, ch, side in shapes:
        out[name] = cut((ch, side, side))
    h = cut((style_count, 512))
    cut.done()
    out['h_coarse'], out['h_middle'], out['h_fine'] = h[:, :3], h[:, 3:7], h[:, 7:]
    return out


def _encode(enc, images, debug):
    R = _check_module(enc)
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError('encode: expected [B,3,%d,%d] images, got %s' % (R, R, tuple(images.shape) if torch.is_tensor(images) else
                                                                         type(images)))
    if images.shape[2] != R or images.shape[3] != R:
        raise ValueError('encode: images of %dx%d, the module was built for %dx%d (its input_size: a multiple of 16 in 32..256, '
                         'whatever image_resolution the heads are counted from)' % (images.shape[2], images.shape[3], R, R))
    N.require_device(images)
    x = N.f32c(images.detach())
    B = x.shape[0]
    lib = N.load()
    n = enc.style_count
    ws, nbytes = _workspace(B, R, n, x.device)
    w = torch.empty((B, n, 512), dtype=torch.float32, device=x.device)
    dbg = torch.empty(lib.sgdfr_e4e_debug_elems_n(B, R, n), dtype=torch.float32, device=x.device) if debug else None
    N.call('sgdfr_e4e_forward_n_f32', N.ptr(x), B, R, n, N.ptr(packed(enc)), N.ptr(w), N.ptr(dbg), N.ptr(ws), nbytes, N.stream())
    return w, (None if dbg is None else debug_views(dbg, B, R, n))


def encode(enc, images):
    """Encoder4Editing(50, 'ir_se', image_resolution, input_size=R) on the kernels of csrc/e4e.hip: images [B,3,R,R] float32 in
    [-1,1] on the device, R = enc.input_size -> W+ [B,style_count,512] with style_count = 2 log2(image_resolution) - 2.  Forward
    only (the result carries no graph), eval mode only, no CPU path, no host synchronisation."""
    return _encode(enc, images, False)[0]


def run_debug(enc, images):
    """One pass with the debug taps -> dict: w [B,style_count,512] and debug (debug_views).  For tests."""
    w, dbg = _encode(enc, images, True)
    return {'w': w, 'debug': dbg}

"""DECA's coefficient encoder on the HIP kernels of csrc/deca.hip: the counterpart of decalib/models/encoders.py ResnetEncoder with
models/resnet.py, of the crop in datasets/datasets.py TestData.get_image_tensor, of DECA.encode's split of the 236 parameters
(deca.py:150-165) and of DECA_model.extract_DECA_params / generic.calculate_shapemodel.

    E = ResnetEncoder(outsize=236); E.load_state_dict(ckpt['E_flame']); E = E.cuda().eval()
    E_detail = ResnetEncoder(outsize=128); E_detail.load_state_dict(ckpt['E_detail']); E_detail = E_detail.cuda().eval()
    M = crop_matrix(bbox, (H, W))                         # [B,2,3] from [B,4] 'kpt68' boxes [left, top, right, bottom]
    code = encode(E, images, M)                           # {'shape','tex','exp','pose','cam','light' [B,9,3],'images' [B,3,224,224]}
    code = encode(E, images, M, E_detail=E_detail)        # ... and 'detail' [B,128], from the same crop (detail.decode_detail takes it)
    params, angles = calculate_shapemodel(E, images, M)   # {'pose','alpha_exp','alpha_shp','cam'}, [B,3] degrees

`ResnetEncoder` has the module layout and state-dict keys of the reference's (deca_model.tar's 'E_flame' loads unchanged) and
holds the weights only, frozen at construction; the HIP kernels run it in eval mode (running BatchNorm statistics).  The images
are GAN-range ([-1,1], values beyond are clamped as torch_range_1_to_255 does); the whole batch runs in one pass, where the
reference encodes one row at a time.  The parameters are differentiable to the images (dL/dimages only); `angles` and the crop
`images` are marked non-differentiable: no caller differentiates them.  Nothing is saved for a backward under torch.no_grad() or
when the images need no gradient.  All 53 BatchNorms are folded into filters + bias on the host in fp64, once per weight
version; the device pack (forward and input-gradient weights, ~2 x 102 MB) is rebuilt whenever a parameter's storage or version
changes.  The 'kpt68' boxes come in as numbers: landmarks.get_landmarks -> landmarks.kpt68_boxes computes them on the device from the
caller's face boxes (the S3FD face detector itself stays with the caller), and a row the detector failed on is the caller's
business (the reference zeroes its coefficients and sets its angles to -180).

E_detail is the same network with a 128-row last layer (encoders.ResnetEncoder(outsize=128)): ResnetEncoder(outsize=128) loads
deca_model.tar's 'E_detail' unchanged and runs on the same kernels, whose output width of 236 is compiled in: `folded()` pads the last
Linear with zero rows to 236, `forward` / `run` return the first 128 columns, and the angles the kernel computes from the padded
columns mean nothing and are dropped by `encode`.  The detail code is forward only: it carries no gradient to the images.  Other
widths (and any last_op) have no kernels.
"""
from collections import OrderedDict

import torch
from torch import nn

from . import _native as N
from .packs import PackedWeights, views

OUTSIZE = 236
DETAIL_OUTSIZE = 128                                      # n_detail (decalib/utils/config.py)
CROP = 224
SCALE = 1.25
PARAM_LIST = (('shape', 100), ('tex', 50), ('exp', 50), ('pose', 6), ('cam', 3), ('light', 27))   # decalib/utils/config.py:34-40
_LAYERS = ((64, 3), (128, 4), (256, 6), (512, 3))


class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample


class _ResNet(nn.Module):
    """models/resnet.py ResNet(Bottleneck, [3, 4, 6, 3]) without its fc: weights only."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for i, (planes, count) in enumerate(_LAYERS):
            blocks = []
            for k in range(count):
                stride = 2 if (k == 0 and i > 0) else 1
                ds = None
                if k == 0:
                    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
                blocks.append(_Bottleneck(inplanes, planes, stride, ds))
                inplanes = planes * 4
            setattr(self, 'layer%d' % (i + 1), nn.Sequential(*blocks))

    def blocks(self):
        for i in range(4):
            for b in getattr(self, 'layer%d' % (i + 1)):
                yield b


class ResnetEncoder(PackedWeights, nn.Module):
    """encoders.ResnetEncoder(outsize=236) (E_flame) or (outsize=128) (E_detail): weights only.  forward(images, M) -> [B,outsize]
    parameters on the HIP kernels."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_deca_prepack_f32', 'sgdfr_deca_pack_elems', N.DECA_PARAMS
    TRAIN_ERROR = ('ResnetEncoder: the HIP kernels run the encoder in eval mode only (running BatchNorm statistics); '
                   'call .eval()')
    GRAD_ERROR = ('ResnetEncoder: the HIP kernels give no gradient for the encoder weights; keep every parameter at '
                  'requires_grad=False')

    def __init__(self, outsize=OUTSIZE, last_op=None):
        if outsize not in (OUTSIZE, DETAIL_OUTSIZE) or last_op is not None:
            raise NotImplementedError('ResnetEncoder: only outsize=236 (E_flame) and outsize=128 (E_detail) without last_op have HIP '
                                      'kernels (got %r, %r)' % (outsize, last_op))
        super().__init__()
        self.outsize = outsize
        self.encoder = _ResNet()
        self.layers = nn.Sequential(nn.Linear(2048, 1024), nn.ReLU(), nn.Linear(1024, outsize))
        for p in self.parameters():
            p.requires_grad = False

    # ---- weights
    def folded(self, dtype=torch.float32):
        """The 134 tensors sgdfr_deca_prepack_f32 takes (None for the projection of an identity block), every BatchNorm folded
        in fp64 on the parameters' device, returned in `dtype`.  The last Linear always has the kernels' 236 rows: rows beyond
        `outsize` are zero."""
        def fold(conv, bn):
            s = bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + bn.eps)
            w = conv.weight.detach().double() * s.view(-1, 1, 1, 1)
            return w, bn.bias.detach().double() - bn.running_mean.detach().double() * s

        r = self.encoder
        out = list(fold(r.conv1, r.bn1))
        for b in r.blocks():
            w1, b1 = fold(b.conv1, b.bn1)
            w2, b2 = fold(b.conv2, b.bn2)
            w3, b3 = fold(b.conv3, b.bn3)
            out += [w1.flatten(1), b1, w2, b2, w3.flatten(1), b3]
            if b.downsample is not None:
                wd, bd = fold(b.downsample[0], b.downsample[1])
                out += [wd.flatten(1), bd]
            else:
                out += [None, None]
        for lin in (self.layers[0], self.layers[2]):
            w, b = lin.weight.detach().double(), lin.bias.detach().double()
            if lin is self.layers[2] and w.shape[0] < OUTSIZE:
                w = torch.cat([w, w.new_zeros(OUTSIZE - w.shape[0], w.shape[1])])
                b = torch.cat([b, b.new_zeros(OUTSIZE - b.shape[0])])
            out += [w, b]
        return [None if v is None else v.to(dtype).contiguous() for v in out]

    def forward(self, images, M):
        return run(self, images, M)[0]


def crop_matrix(bbox, src_hw, align_corners=False, dtype=torch.float32):
    """[B,2,3] matrices from an output pixel (u, v, 1) of the 224x224 crop to a source pixel (x, y), for [B,4] boxes
    [left, top, right, bottom] of the 68 landmarks ('kpt68', the only type the reference's detectors.FAN returns) on images of
    src_hw = (H, W).  Restates TestData.get_image_tensor (datasets.py:57-82) with its constants (scale 1.25, crop 224):
    bbox2point, size = int(old_size * scale), the similarity transform through the three corner points -- exact, with the closed form
    s = (crop - 1) / size, no rotation, t = -s (center - size / 2) -- and kornia 0.4.1's warp_affine: normalise both pixel grids
    with normal_transform_pixel (2 / (size - 1), -1), invert, F.affine_grid + F.grid_sample(bilinear, zeros) with `align_corners`
    (kornia 0.4.1's default: False).  The kornia half is written from its 0.4.1 source as remembered and is pinned only against
    F.affine_grid + F.grid_sample composed that way: the composition itself is UNVERIFIED against kornia.  `encode` takes the
    matrix, not the box, so a caller who knows kornia's behaviour better can pass another.  Host maths in fp64 on the boxes'
    device (a device tensor stays on the device, no synchronisation); returns `dtype` (the kernels take float32)."""
    H, W = int(src_hw[0]), int(src_hw[1])
    b = torch.as_tensor(bbox)
    if b.dim() != 2 or b.shape[1] != 4:
        raise ValueError('crop_matrix: expected [B,4] boxes [left, top, right, bottom], got %s' % (tuple(b.shape),))
    b = b.to(torch.float64)
    left, top, right, bottom = b.unbind(1)
    old_size = (right - left + bottom - top) / 2 * 1.1
    cx, cy = right - (right - left) / 2.0, bottom - (bottom - top) / 2.0
    size = torch.trunc(old_size * SCALE)
    s = (CROP - 1) / size                                  # crop pixel = s * (source pixel - (center - size / 2))
    ox, oy = cx - size / 2, cy - size / 2
    if align_corners:                                      # every normalisation cancels: sample at T^-1 (u, v)
        au, bu, av, bv = 1 / s, ox, 1 / s, oy
    else:
        # u -> dst_norm = (2u + 1) / 224 - 1 -> "pixel" (dst_norm + 1) (224 - 1) / 2 -> T^-1 -> src_norm = 2 p / (W - 1) - 1
        # -> sampled pixel ((src_norm + 1) W - 1) / 2 = p W / (W - 1) - 1 / 2
        k, k0 = (CROP - 1) / CROP, (CROP - 1) / (2.0 * CROP)
        fx, fy = W / (W - 1.0), H / (H - 1.0)
        au, bu = fx * k / s, fx * (k0 / s + ox) - 0.5
        av, bv = fy * k / s, fy * (k0 / s + oy) - 0.5
    z = torch.zeros_like(au)
    M = torch.stack([torch.stack([au, z, bu], 1), torch.stack([z, av, bv], 1)], 1)
    return M.to(dtype)


def _workspace(rows, H, W, device):
    return N.workspace('sgdfr_deca_workspace_bytes', device, rows, H, W,
                       error='deca: unsupported batch of %d images of %dx%d' % (rows, H, W))


def debug_views(debug, rows):
    """The debug buffer as named views (csrc/deca.hip's DebugLayout): stem, pool, first / last (per stage), feat."""
    out, take = {'first': [], 'last': []}, views(debug, rows)

    out['stem'] = take((64, 112, 112))
    out['pool'] = take((64, 56, 56))
    for s in range(4):
        shape = (256 << s, 56 >> s, 56 >> s)
        out['first'].append(take(shape))
        out['last'].append(take(shape))
    out['feat'] = take((2048,))
    take.done()
    return out


def saved_views(saved, rows):
    """The saved bytes of a forward with `rows` rows as named uint8 views (csrc/deca.hip's SavedLayout): stem (ReLU mask), arg
    (max-pool choice kh * 3 + kw), per bottleneck m1, m2, m3 (ReLU masks after conv1, conv2 and the sum), fc (regressor mask)."""
    out, take = {'m1': [], 'm2': [], 'm3': []}, views(saved, rows, align=64)

    out['stem'] = take((64, 112, 112))
    out['arg'] = take((64, 56, 56))
    h = 56
    for i, (planes, count) in enumerate(_LAYERS):
        for k in range(count):
            ho = h // 2 if (k == 0 and i > 0) else h
            out['m1'].append(take((planes, h, h)))
            out['m2'].append(take((planes, ho, ho)))
            out['m3'].append(take((4 * planes, ho, ho)))
            h = ho
    out['fc'] = take((1024,))
    take.done()
    return out


def _forward(pack, x, M, save, debug=False):
    B, _, H, W = x.shape
    dev = x.device
    lib = N.load()
    crop = torch.empty((B, 3, CROP, CROP), dtype=torch.float32, device=dev)
    params = torch.empty((B, OUTSIZE), dtype=torch.float32, device=dev)
    angles = torch.empty((B, 3), dtype=torch.float32, device=dev)
    saved = torch.empty(lib.sgdfr_deca_saved_elems(B), dtype=torch.uint8, device=dev) if save else None
    dbg = torch.empty(lib.sgdfr_deca_debug_elems(B), dtype=torch.float32, device=dev) if debug else None
    ws, nbytes = _workspace(B, H, W, dev)
    N.call('sgdfr_deca_forward_f32', N.ptr(x), N.ptr(M), B, H, W, N.ptr(pack), N.ptr(crop), N.ptr(params), N.ptr(angles), N.ptr(saved),
           N.ptr(dbg), N.ptr(ws), nbytes, N.stream())
    return params, angles, crop, saved, dbg


class _DecaFn(torch.autograd.Function):
    """(parameters, angles, crop) on the HIP kernels; backward: dL/dx of the parameters only (frozen weights, constant M)."""

    @staticmethod
    def forward(ctx, x, pack, M, save):
        params, angles, crop, saved, _ = _forward(pack, x, M, save)
        if save:
            ctx.save_for_backward(saved, pack, x, M)
        ctx.saved_bytes = 0 if saved is None else saved.numel()
        ctx.mark_non_differentiable(angles, crop)
        return params, angles, crop

    @staticmethod
    def backward(ctx, gp, ga, gc):
        saved, pack, x, M = ctx.saved_tensors
        B, _, H, W = x.shape
        g = gp.to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        ws, nbytes = _workspace(B, H, W, g.device)
        N.call('sgdfr_deca_backward_f32', N.ptr(g), N.ptr(x), N.ptr(M), N.ptr(saved), B, H, W, N.ptr(pack), N.ptr(dx), N.ptr(ws), nbytes,
               N.stream())
        return dx, None, None, None


def _check_inputs(images, M):
    N.require_device(images, M)
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError('deca: expected [B,3,H,W] images, got %s' % (tuple(images.shape),))
    if tuple(M.shape) != (images.shape[0], 2, 3):
        raise ValueError('deca: expected [%d,2,3] crop matrices, got %s' % (images.shape[0], tuple(M.shape)))


def run(E, images, M):
    """(parameters [B,236], angles [B,3] degrees, crop [B,3,224,224]) of one pass; the parameters are differentiable to images.
    For E_detail (outsize 128): the [B,128] detail code, forward only, and angles that mean nothing."""
    E.check()
    _check_inputs(images, M)
    x = N.f32c(images)
    if E.outsize != OUTSIZE:
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError('ResnetEncoder(outsize=%d): the detail code has no gradient to the images; call it under '
                               'torch.no_grad() or on detached images' % E.outsize)
        params, angles, crop, _, _ = _forward(E.packed(), x, N.f32c(M.detach()), False)
        return params[:, :E.outsize], angles, crop
    save = torch.is_grad_enabled() and x.requires_grad      # nothing is kept for a forward without a gradient
    return _DecaFn.apply(x, E.packed(), N.f32c(M.detach()), save)


def run_debug(E, images, M, save=False):
    """One forward with the debug switch on -> (parameters, angles, crop, saved bytes or None, debug_views dict).  For tests."""
    E.check()
    _check_inputs(images, M)
    with torch.no_grad():
        x = N.f32c(images.detach())
        params, angles, crop, saved, dbg = _forward(E.packed(), x, N.f32c(M.detach()), save, debug=True)
    return params, angles, crop, saved, debug_views(dbg, x.shape[0])


def backward_from(E, grad_params, images, M, saved):
    """dL/dimages for grad_params [B,236] from the saved bytes of a forward on the same images and M (run_debug(save=True))."""
    x = N.f32c(images.detach())
    B, _, H, W = x.shape
    g = grad_params.to(torch.float32).contiguous()
    dx = torch.empty_like(x)
    ws, nbytes = _workspace(B, H, W, x.device)
    N.call('sgdfr_deca_backward_f32', N.ptr(g), N.ptr(x), N.ptr(N.f32c(M)), N.ptr(saved), B, H, W, N.ptr(E.packed()), N.ptr(dx), N.ptr(ws),
           nbytes, N.stream())
    return dx


class _CropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, M):
        B, _, H, W = x.shape
        out = torch.empty((B, 3, CROP, CROP), dtype=torch.float32, device=x.device)
        N.call('sgdfr_deca_crop_f32', N.ptr(x), N.ptr(M), B, H, W, N.ptr(out), N.stream())
        ctx.save_for_backward(x, M)
        return out

    @staticmethod
    def backward(ctx, g):
        x, M = ctx.saved_tensors
        B, _, H, W = x.shape
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        N.call('sgdfr_deca_crop_backward_f32', N.ptr(g), N.ptr(x), N.ptr(M), B, H, W, N.ptr(dx), N.stream())
        return dx, None


def crop(images, M):
    """The front alone: GAN-range images [B,3,H,W] -> [0,255] -> bilinear crop at (u, v, 1) M^T with zero padding -> / 255, as
    [B,3,224,224] in [0,1]; differentiable to the images (the gradient passes where -1 <= x <= 1, as through torch.clamp)."""
    _check_inputs(images, M)
    return _CropFn.apply(N.f32c(images), N.f32c(M.detach()))


def split_parameters(params):
    """DECA.decompose_code (deca.py:118-131): the 236 parameters as views in param_list order; light as [B,9,3]."""
    code, o = OrderedDict(), 0
    for name, n in PARAM_LIST:
        code[name] = params[:, o:o + n]
        o += n
    code['light'] = code['light'].reshape(params.shape[0], 9, 3)
    return code


def encode(E, images, M, E_detail=None):
    """DECA.encode (deca.py:150-165) for a batch of GAN-range images and their crop matrices: {'shape' [B,100], 'tex' [B,50],
    'exp' [B,50], 'pose' [B,6], 'cam' [B,3], 'light' [B,9,3], 'images' [B,3,224,224] (the crop in [0,1])}; with E_detail
    (ResnetEncoder(outsize=128)) also 'detail' [B,128] from the same crop, which carries no gradient."""
    if E_detail is not None and (not isinstance(E_detail, ResnetEncoder) or E_detail.outsize != DETAIL_OUTSIZE):
        raise ValueError('encode: E_detail must be a ResnetEncoder(outsize=%d)' % DETAIL_OUTSIZE)
    if E.outsize != OUTSIZE:
        raise ValueError('encode: E must be a ResnetEncoder(outsize=%d), got outsize=%d' % (OUTSIZE, E.outsize))
    params, _, crop = run(E, images, M)
    code = split_parameters(params)
    if E_detail is not None:
        code['detail'] = run(E_detail, images.detach(), M)[0]
    code['images'] = crop
    return code


def calculate_shapemodel(E, images, M):
    """generic.calculate_shapemodel with DECA_model.extract_DECA_params (estimate_DECA.py:30-53) in one batched call:
    ({'pose', 'alpha_exp', 'alpha_shp', 'cam'}, angles [B,3]) with angles = rad2deg(batch_axis2euler(pose[:, :3])) for EVERY
    row, on the device (the reference's batch_matrix2euler returns its last row as a [1,3] CPU tensor because it is called with
    one row).  For |R20| > 0.998 the reference's `> 0.998` branch calls an undefined bare atan2 and would raise; what the code
    evidently means is implemented: z = 0, x = +-pi/2, y = atan2(-+R01, -+R02)."""
    params, angles, _ = run(E, images, M)
    code = split_parameters(params)
    return {'pose': code['pose'], 'alpha_exp': code['exp'], 'alpha_shp': code['shape'], 'cam': code['cam']}, angles

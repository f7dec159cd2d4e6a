"""The 2D-FAN-4 landmark detector on the HIP kernels of csrc/fan.hip: the counterpart of libs/face_models/fan_model/models.py
FAN(4), of LandmarksEstimation.get_landmarks (landmarks_estimation.py:143-185, 2D branch, flip_input=False) with crop_torch and
transform (fan_model/utils.py:63-97, 140-165) and get_preds_fromhm (landmarks_estimation.py:50-88), and of the 'kpt68' box of
libs/DECA/decalib/datasets/detectors.py:38-41 that deca.crop_matrix takes.

    fan = FAN(4); fan.load_state_dict(sd); fan = fan.cuda().eval()          # 2DFAN4-*.pth.tar loads unchanged
    pts_img, pts, heatmaps = get_landmarks(fan, images, faces, input_range='255')
    boxes = kpt68_boxes(pts_img)                                            # [B,4] left, top, right, bottom -> deca.crop_matrix

`FAN` has the module layout and the 1129 state-dict keys of the reference's and holds the weights only, frozen at construction;
the HIP kernels run it in eval mode (running BatchNorm statistics), forward only: the box is a number, nothing differentiates it.
The whole batch runs in one pass (the reference crops, runs and decodes one face at a time and moves the heatmaps to the CPU and
back); centre, scale and the integer window are computed on the device, so nothing in a call synchronises with the host.  The
BatchNorms in front of the ConvBlock convs cannot be folded into filters (a ReLU sits between): they are folded on the host in fp64
to a per-channel (g, h) that the conv's loader applies; only conv1 + bn1 and conv_last + bn_end fold into filters.  The device pack
(~95 MB) is rebuilt whenever a parameter's storage or version changes.

The crop: `transforms.Resize` on a tensor is F.interpolate(mode='bilinear', align_corners=False) without antialiasing in the
torchvision the reference was written for.  torchvision was not available when this was written, so the resize is pinned only
against F.interpolate composed that way: the composition itself is UNVERIFIED against torchvision.

Face boxes come in as numbers or as a device tensor; face_detector.py (S3FD on csrc/s3fd.hip) produces them and
face_detector.detect_landmarks chains the two.

The rest of the class (landmarks_estimation.py:155-181): `get_landmarks(..., flip_input=True)` runs the network once on the crops
with their mirrors behind them and decodes the sum net(inp) + flip(net(flip(inp)), is_label=True); `get_landmarks_3d` is the 3D
landmark type, the class's default: a 13x13 Gaussian is drawn per landmark (fan_model/utils.py:13-60), `ResNetDepth`
(fan_model/models.py:205-265, csrc/fandepth.hip: 155 convs with every BatchNorm folded into its filters, ~234 MB pack) reads the
crop and the 68 maps through a stem that gathers from both tensors, and pts_img becomes [B,68,3].

    depth_net = ResNetDepth(); depth_net.load_state_dict(sd); depth_net = depth_net.cuda().eval()     # 'module.' prefix stripped
    pts_img3, pts, heatmaps = get_landmarks_3d(fan, depth_net, images, faces, flip_input=False)

`flip_add`, `draw` and `depth_network` are the pieces alone.
"""
import torch
from torch import nn

from . import _native as N
from .packs import PackedWeights, views

STACKS = 4
DEPTH = 4
POINTS = 68
CROP = 256
MAP = 64
RANGES = {'255': N.FAN_RANGE_255, 'gan': N.FAN_RANGE_GAN}


class _ConvBlock(nn.Module):
    """models.py ConvBlock(in, out): BN -> ReLU -> conv3x3 three times, concatenated, plus the (projected) input.  Weights only."""

    def __init__(self, cin, cout):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, cout // 2, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout // 2)
        self.conv2 = nn.Conv2d(cout // 2, cout // 4, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout // 4)
        self.conv3 = nn.Conv2d(cout // 4, cout // 4, 3, padding=1, bias=False)
        self.downsample = None
        if cin != cout:
            self.downsample = nn.Sequential(nn.BatchNorm2d(cin), nn.ReLU(True), nn.Conv2d(cin, cout, 1, bias=False))


class _HourGlass(nn.Module):
    """models.py HourGlass(1, 4, 256): b1, b2 per level going down, b2_plus at the bottom, b3 per level coming up.  Weights only."""

    def __init__(self, depth, features):
        super().__init__()
        self._add(depth, features)

    def _add(self, level, f):
        self.add_module('b1_%d' % level, _ConvBlock(f, f))
        self.add_module('b2_%d' % level, _ConvBlock(f, f))
        if level > 1:
            self._add(level - 1, f)
        else:
            self.add_module('b2_plus_%d' % level, _ConvBlock(f, f))
        self.add_module('b3_%d' % level, _ConvBlock(f, f))


class FAN(PackedWeights, nn.Module):
    """models.FAN(num_modules=4): weights only.  forward(crop [B,3,256,256] in [0,1]) -> the last stack's heatmaps [B,68,64,64]."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_fan_prepack_f32', 'sgdfr_fan_pack_elems', N.FAN_PARAMS
    TRAIN_ERROR = 'FAN: the HIP kernels run the network in eval mode only (running BatchNorm statistics); call .eval()'
    GRAD_ERROR = ('FAN: the HIP kernels are forward only and give no gradient for the weights; keep every parameter at '
                  'requires_grad=False')

    def __init__(self, num_modules=4):
        if num_modules != STACKS:
            raise NotImplementedError('FAN: only num_modules=4 (NetworkSize.LARGE, 2DFAN-4) has HIP kernels, got %r' % (num_modules,))
        super().__init__()
        self.num_modules = num_modules
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = _ConvBlock(64, 128)
        self.conv3 = _ConvBlock(128, 128)
        self.conv4 = _ConvBlock(128, 256)
        for i in range(num_modules):
            self.add_module('m%d' % i, _HourGlass(DEPTH, 256))
            self.add_module('top_m_%d' % i, _ConvBlock(256, 256))
            self.add_module('conv_last%d' % i, nn.Conv2d(256, 256, 1))
            self.add_module('bn_end%d' % i, nn.BatchNorm2d(256))
            self.add_module('l%d' % i, nn.Conv2d(256, POINTS, 1))
            if i < num_modules - 1:
                self.add_module('bl%d' % i, nn.Conv2d(256, 256, 1))
                self.add_module('al%d' % i, nn.Conv2d(POINTS, 256, 1))
        for p in self.parameters():
            p.requires_grad = False

    # ---- weights
    def blocks(self):
        """The 59 ConvBlocks in the order sgdfr_fan_prepack_f32 takes them."""
        out = [self.conv2, self.conv3, self.conv4]
        for i in range(STACKS):
            m = getattr(self, 'm%d' % i)
            for level in range(DEPTH, 0, -1):
                out += [getattr(m, 'b%d_%d' % (k, level)) for k in (1, 2, 3)]
            out += [m.b2_plus_1, getattr(self, 'top_m_%d' % i)]
        return out

    def folded(self, dtype=torch.float32):
        """The 735 tensors sgdfr_fan_prepack_f32 takes (None for the projection of an identity block), every BatchNorm folded in
        fp64 on the parameters' device, returned in `dtype`."""
        def gh(bn):
            g = bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + bn.eps)
            return g, bn.bias.detach().double() - bn.running_mean.detach().double() * g

        def fold(conv, bn):
            g, h = gh(bn)
            return conv.weight.detach().double() * g.view(-1, 1, 1, 1), conv.bias.detach().double() * g + h

        out = list(fold(self.conv1, self.bn1))
        for b in self.blocks():
            for bn, conv in ((b.bn1, b.conv1), (b.bn2, b.conv2), (b.bn3, b.conv3)):
                out += list(gh(bn)) + [conv.weight.detach().double()]
            if b.downsample is not None:
                out += list(gh(b.downsample[0])) + [b.downsample[2].weight.detach().double().flatten(1)]
            else:
                out += [None, None, None]
        for i in range(STACKS):
            w, bias = fold(getattr(self, 'conv_last%d' % i), getattr(self, 'bn_end%d' % i))
            l = getattr(self, 'l%d' % i)
            out += [w.flatten(1), bias, l.weight.detach().double().flatten(1), l.bias.detach().double()]
        for i in range(STACKS - 1):
            bl, al = getattr(self, 'bl%d' % i), getattr(self, 'al%d' % i)
            out += [bl.weight.detach().double().flatten(1), al.weight.detach().double().flatten(1),
                    bl.bias.detach().double() + al.bias.detach().double()]
        return [None if v is None else v.to(dtype).contiguous() for v in out]

    def forward(self, crop):
        return network(self, crop)


class _Bottleneck(nn.Module):
    """models.py Bottleneck(inplanes, planes, stride, downsample): conv1x1 -> conv3x3 at the stride -> conv1x1, each with its BatchNorm,
    plus the (projected) input.  Weights only."""

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample


class ResNetDepth(PackedWeights, nn.Module):
    """models.ResNetDepth(Bottleneck, [3, 8, 36, 3], 68): weights only, the reference's 932 state-dict keys (its `depth` checkpoint
    loads once the 'module.' prefix is stripped, as landmarks_estimation.py:136-138 does).  forward(crop [B,3,256,256] in [0,1], maps
    [B,68,256,256]) -> depth [B,68]."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_fandepth_prepack_f32', 'sgdfr_fandepth_pack_elems', N.FANDEPTH_PARAMS
    TRAIN_ERROR = 'ResNetDepth: the HIP kernels run the network in eval mode only (running BatchNorm statistics); call .eval()'
    GRAD_ERROR = ('ResNetDepth: the HIP kernels are forward only and give no gradient for the weights; keep every parameter at '
                  'requires_grad=False')
    LAYERS = (3, 8, 36, 3)

    def __init__(self):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3 + POINTS, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        for i, (planes, blocks) in enumerate(zip((64, 128, 256, 512), self.LAYERS)):
            self.add_module('layer%d' % (i + 1), self._make_layer(planes, blocks, 1 if i == 0 else 2))
        self.fc = nn.Linear(2048, POINTS)
        for p in self.parameters():
            p.requires_grad = False

    def _make_layer(self, planes, blocks, stride):
        downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
        layers = [_Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * 4
        layers += [_Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def bottlenecks(self):
        """The 50 bottlenecks in forward order."""
        return [b for i in range(4) for b in getattr(self, 'layer%d' % (i + 1))]

    def folded(self, dtype=torch.float32):
        """The 312 tensors sgdfr_fandepth_prepack_f32 takes, every BatchNorm folded into its conv in fp64 on the parameters' device,
        returned in `dtype`: stem w, b; per bottleneck w1, b1, w2, b2, w3, b3 and, behind the first of a layer, wd, bd; fc w, b."""
        def fold(conv, bn):
            g = bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + bn.eps)
            return conv.weight.detach().double() * g.view(-1, 1, 1, 1), bn.bias.detach().double() - bn.running_mean.detach().double() * g

        out = list(fold(self.conv1, self.bn1))
        for b in self.bottlenecks():
            for conv, bn in ((b.conv1, b.bn1), (b.conv2, b.bn2), (b.conv3, b.bn3)):
                out += list(fold(conv, bn))
            if b.downsample is not None:
                out += list(fold(b.downsample[0], b.downsample[1]))
        out += [self.fc.weight.detach().double(), self.fc.bias.detach().double()]
        return [v.to(dtype).contiguous() for v in out]

    def forward(self, crop, maps):
        return depth_network(self, crop, maps)


# ---------------------------------------------------------------------------------------------------------------- checks
def _faces(faces, images):
    """[B,4] float32 x0, y0, x1, y1 on the images' device from a [B,4] / [B,5] tensor or numbers (a fifth column, the score, is
    dropped).  A device tensor stays on the device."""
    f = faces if torch.is_tensor(faces) else torch.as_tensor(faces, dtype=torch.float32)
    if f.dim() != 2 or f.shape[1] not in (4, 5) or f.shape[0] != images.shape[0]:
        raise ValueError('landmarks: expected [%d,4] (or [%d,5]) face boxes x0, y0, x1, y1, got %s' % (images.shape[0], images.shape[0],
                                                                                                      tuple(f.shape)))
    return f


def _check_images(images):
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError('landmarks: expected [B,3,H,W] images, got %s' % (tuple(images.shape) if torch.is_tensor(images) else type(images),))


def _range(input_range):
    if input_range not in RANGES:
        raise ValueError("landmarks: input_range must be '255' (0..255 values) or 'gan' ([-1,1]), got %r" % (input_range,))
    return RANGES[input_range]


def _prepare(images, faces, input_range):
    code = _range(input_range)
    _check_images(images)
    f = _faces(faces, images)
    N.require_device(images)
    f = f.to(device=images.device, dtype=torch.float32)[:, :4].contiguous()
    return N.f32c(images.detach()), f, code


def _unsupported(rows, H, W):
    return 'landmarks: unsupported batch of %d images of %dx%d' % (rows, H, W)


def _workspace(rows, H, W, device):
    return N.workspace('sgdfr_fan_workspace_bytes', device, rows, H, W, error=_unsupported(rows, H, W))


def debug_views(debug, rows):
    """The debug buffer as named views (csrc/fan.hip's DebugLayout): stem, conv4, hg (per stack), heatmaps (per stack)."""
    out, take = {'hg': [], 'heatmaps': []}, views(debug, rows)

    out['stem'] = take((64, 128, 128))
    out['conv4'] = take((256, MAP, MAP))
    for _ in range(STACKS):
        out['hg'].append(take((256, MAP, MAP)))
        out['heatmaps'].append(take((POINTS, MAP, MAP)))
    take.done()
    return out


# ---------------------------------------------------------------------------------------------------------------- calls
def crop(images, faces, input_range='255'):
    """The front alone: the window of crop_torch around each face box with zero padding, resized to 256x256, / 255 -> [B,3,256,256]."""
    x, f, code = _prepare(images, faces, input_range)
    B, _, H, W = x.shape
    N.size('sgdfr_fan_workspace_bytes', B, H, W, error=_unsupported(B, H, W))
    out = torch.empty((B, 3, CROP, CROP), dtype=torch.float32, device=x.device)
    N.call('sgdfr_fan_crop_f32', N.ptr(x), N.ptr(f), B, H, W, code, N.ptr(out), N.stream())
    return out


def _check_crop(c):
    if not torch.is_tensor(c) or c.dim() != 4 or tuple(c.shape[1:]) != (3, CROP, CROP) or c.shape[0] < 1:
        raise ValueError('landmarks: expected [B,3,256,256] crops, got %s' % (tuple(c.shape) if torch.is_tensor(c) else type(c),))
    N.require_device(c)


def network(fan, crops, debug=False):
    """The network alone: crops [B,3,256,256] in [0,1] -> the last stack's heatmaps [B,68,64,64]; with debug=True
    (heatmaps, debug_views dict)."""
    fan.check()
    _check_crop(crops)
    c = N.f32c(crops.detach())
    B = c.shape[0]
    lib = N.load()
    ws, nbytes = _workspace(B, CROP, CROP, c.device)
    hm = torch.empty((B, POINTS, MAP, MAP), dtype=torch.float32, device=c.device)
    dbg = torch.empty(lib.sgdfr_fan_debug_elems(B), dtype=torch.float32, device=c.device) if debug else None
    N.call('sgdfr_fan_network_f32', N.ptr(c), B, N.ptr(fan.packed()), N.ptr(hm), N.ptr(dbg), N.ptr(ws), nbytes, N.stream())
    return (hm, debug_views(dbg, B)) if debug else hm


def decode(heatmaps, faces):
    """get_preds_fromhm for [B,68,64,64] heatmaps and their face boxes -> (pts_img [B,68,2], pts [B,68,2], boxes [B,4])."""
    if not torch.is_tensor(heatmaps) or heatmaps.dim() != 4 or tuple(heatmaps.shape[1:]) != (POINTS, MAP, MAP) or heatmaps.shape[0] < 1:
        raise ValueError('landmarks: expected [B,68,64,64] heatmaps, got %s' % (tuple(heatmaps.shape) if torch.is_tensor(heatmaps) else
                                                                               type(heatmaps),))
    f = _faces(faces, heatmaps)
    N.require_device(heatmaps)
    f = f.to(device=heatmaps.device, dtype=torch.float32)[:, :4].contiguous()
    hm = N.f32c(heatmaps.detach())
    B = hm.shape[0]
    pts = torch.empty((B, POINTS, 2), dtype=torch.float32, device=hm.device)
    pts_img = torch.empty_like(pts)
    boxes = torch.empty((B, 4), dtype=torch.float32, device=hm.device)
    N.call('sgdfr_fan_decode_f32', N.ptr(hm), N.ptr(f), B, N.ptr(pts), N.ptr(pts_img), N.ptr(boxes), N.stream())
    return pts_img, pts, boxes


def flip_add(hm2):
    """The sum of flip_input (landmarks_estimation.py:157-159) alone: hm2 [2B,68,64,64], rows 0..B-1 the heatmaps of the crops and
    rows B..2B-1 those of their mirrors -> [B,68,64,64] = hm2[:B] + flip(hm2[B:], is_label=True)."""
    if (not torch.is_tensor(hm2) or hm2.dim() != 4 or tuple(hm2.shape[1:]) != (POINTS, MAP, MAP) or hm2.shape[0] < 2
            or hm2.shape[0] % 2):
        raise ValueError('landmarks: expected [2B,68,64,64] heatmaps, got %s' % (tuple(hm2.shape) if torch.is_tensor(hm2) else type(hm2),))
    N.require_device(hm2)
    h = N.f32c(hm2.detach())
    B = h.shape[0] // 2
    N.size('sgdfr_fan_debug_elems', 2 * B, error=_unsupported(B, MAP, MAP))
    out = torch.empty((B, POINTS, MAP, MAP), dtype=torch.float32, device=h.device)
    N.call('sgdfr_fan_flip_add_f32', N.ptr(h), B, N.ptr(out), N.stream())
    return out


def draw(pts):
    """draw_gaussian (fan_model/utils.py:39-60, sigma 2) as get_landmarks calls it (:166-171): pts [B,68,2] crop pixels ->
    [B,68,256,256] maps, zero but for one 13x13 Gaussian each, and zero throughout where pts.x <= 0 or the window misses the map."""
    if not torch.is_tensor(pts) or pts.dim() != 3 or tuple(pts.shape[1:]) != (POINTS, 2) or pts.shape[0] < 1:
        raise ValueError('landmarks: expected [B,68,2] points, got %s' % (tuple(pts.shape) if torch.is_tensor(pts) else type(pts),))
    N.require_device(pts)
    p = N.f32c(pts.detach())
    B = p.shape[0]
    N.size('sgdfr_fan_debug_elems', B, error=_unsupported(B, CROP, CROP))
    maps = torch.empty((B, POINTS, CROP, CROP), dtype=torch.float32, device=p.device)
    N.call('sgdfr_fan_draw_f32', N.ptr(p), B, N.ptr(maps), N.stream())
    return maps


def depth_debug_views(debug, rows):
    """The debug buffer as named views (csrc/fandepth.hip's DebugLayout): stem, pool, layer (four), feat."""
    out, take = {}, views(debug, rows)
    out['stem'] = take((64, 128, 128))
    out['pool'] = take((64, 64, 64))
    out['layer'] = [take((256 << s, 64 >> s, 64 >> s)) for s in range(4)]
    out['feat'] = take((2048,))
    take.done()
    return out


def _depth_workspace(rows, device):
    return N.workspace('sgdfr_fandepth_workspace_bytes', device, rows, error=_unsupported(rows, CROP, CROP))


def depth_network(depth_net, crops, maps, debug=False):
    """ResNetDepth alone: crops [B,3,256,256] in [0,1] and maps [B,68,256,256] (the reference concatenates them; the stem reads both)
    -> depth [B,68]; with debug=True (depth, depth_debug_views dict)."""
    depth_net.check()
    _check_crop(crops)
    if not torch.is_tensor(maps) or tuple(maps.shape) != (crops.shape[0], POINTS, CROP, CROP):
        raise ValueError('landmarks: expected [%d,68,256,256] maps, got %s' % (crops.shape[0], tuple(maps.shape) if torch.is_tensor(maps)
                                                                                 else type(maps),))
    N.require_device(maps)
    c, m = N.f32c(crops.detach()), N.f32c(maps.detach())
    B = c.shape[0]
    ws, nbytes = _depth_workspace(B, c.device)
    depth = torch.empty((B, POINTS), dtype=torch.float32, device=c.device)
    dbg = torch.empty(N.load().sgdfr_fandepth_debug_elems(B), dtype=torch.float32, device=c.device) if debug else None
    N.call('sgdfr_fandepth_network_f32', N.ptr(c), N.ptr(m), B, N.ptr(depth_net.packed()), N.ptr(depth), N.ptr(dbg), N.ptr(ws), nbytes,
           N.stream())
    return (depth, depth_debug_views(dbg, B)) if debug else depth


def _forward(fan, images, faces, input_range, debug):
    fan.check()
    x, f, code = _prepare(images, faces, input_range)
    B, _, H, W = x.shape
    dev = x.device
    lib = N.load()
    ws, nbytes = _workspace(B, H, W, dev)
    hm = torch.empty((B, POINTS, MAP, MAP), dtype=torch.float32, device=dev)
    pts = torch.empty((B, POINTS, 2), dtype=torch.float32, device=dev)
    pts_img = torch.empty_like(pts)
    boxes = torch.empty((B, 4), dtype=torch.float32, device=dev)
    dbg = torch.empty(lib.sgdfr_fan_debug_elems(B), dtype=torch.float32, device=dev) if debug else None
    N.call('sgdfr_fan_forward_f32', N.ptr(x), N.ptr(f), B, H, W, code, N.ptr(fan.packed()), N.ptr(hm), N.ptr(pts), N.ptr(pts_img),
           N.ptr(boxes), N.ptr(dbg), N.ptr(ws), nbytes, N.stream())
    return pts_img, pts, hm, boxes, dbg


def _forward3d(fan, depth_net, images, faces, input_range, flip_input):
    """One sgdfr_fan_forward3d_f32 call: the network runs on 2B rows with flip_input (the mirrors behind the crops), so workspace and
    row limit are those of 2B rows; depth_net None stops behind the decode."""
    fan.check()
    if depth_net is not None:
        depth_net.check()
    x, f, code = _prepare(images, faces, input_range)
    B, _, H, W = x.shape
    dev = x.device
    rows = 2 * B if flip_input else B
    ws, nbytes = N.workspace('sgdfr_fan_workspace_bytes', dev, rows, H, W, error=_unsupported(rows, H, W))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    hm2 = new(rows, POINTS, MAP, MAP) if flip_input else None
    hm, pts, pts_img, boxes = new(B, POINTS, MAP, MAP), new(B, POINTS, 2), new(B, POINTS, 2), new(B, 4)
    maps = depth = pts_img3 = dws = dpack = None
    dbytes = 0
    if depth_net is not None:
        dws, dbytes = _depth_workspace(B, dev)
        maps, depth, pts_img3, dpack = new(B, POINTS, CROP, CROP), new(B, POINTS), new(B, POINTS, 3), depth_net.packed()
    N.call('sgdfr_fan_forward3d_f32', N.ptr(x), N.ptr(f), B, H, W, code, 1 if flip_input else 0, N.ptr(fan.packed()), N.ptr(dpack),
           N.ptr(hm2), N.ptr(hm), N.ptr(pts), N.ptr(pts_img), N.ptr(boxes), N.ptr(maps), N.ptr(depth), N.ptr(pts_img3), None, N.ptr(ws),
           nbytes, N.ptr(dws), dbytes, N.stream())
    return pts_img3, pts_img, pts, hm, depth, maps


def get_landmarks(fan, images, faces, input_range='255', flip_input=False):
    """LandmarksEstimation.get_landmarks (2D type) for a whole batch in one pass.  images [B,3,H,W] float32 on the device, 0..255
    values (input_range='255', as the reference takes them) or GAN-range [-1,1] (input_range='gan': torch_range_1_to_255 is applied,
    the map deca.encode applies, so one generated tensor feeds both); faces [B,4] (or [B,5], the score ignored) x0, y0, x1, y1 from the
    caller's detector, a tensor or numbers.  flip_input=True adds the heatmaps of the mirrored crop (:157-159) in front of the decode:
    the network then runs on 2B rows, and a call takes half as many images.  Returns (pts_img [B,68,2] image pixels, integer-valued
    float32; pts [B,68,2] crop pixels = preds * 4; heatmaps [B,68,64,64] of the last stack, the sum with flip_input).  No host
    synchronisation; nothing is differentiable."""
    if flip_input:
        _, pts_img, pts, hm, _, _ = _forward3d(fan, None, images, faces, input_range, True)
        return pts_img, pts, hm
    pts_img, pts, hm, _, _ = _forward(fan, images, faces, input_range, False)
    return pts_img, pts, hm


def get_landmarks_3d(fan, depth_net, images, faces, input_range='255', flip_input=False):
    """LandmarksEstimation.get_landmarks with the 3D landmark type, the class's default (:165-181): behind the decode one Gaussian
    per landmark is drawn at pts, ResNetDepth reads the crop with the 68 maps, and z = depth * (1 / (256 / (200 scale))) joins the
    image coordinates.  Returns (pts_img [B,68,3], pts [B,68,2], heatmaps [B,68,64,64]); the first two columns of pts_img are
    get_landmarks' own.  One native call, no host synchronisation."""
    pts_img3, _, pts, hm, _, _ = _forward3d(fan, depth_net, images, faces, input_range, flip_input)
    return pts_img3, pts, hm


def run_debug(fan, images, faces, input_range='255'):
    """One pass with the debug switch on -> (pts_img, pts, heatmaps, boxes, debug_views dict).  For tests."""
    pts_img, pts, hm, boxes, dbg = _forward(fan, images, faces, input_range, True)
    return pts_img, pts, hm, boxes, debug_views(dbg, hm.shape[0])


def kpt68_boxes(pts_img):
    """detectors.FAN.run's box of the 68 points (detectors.py:38-41): [B,4] float32 left, top, right, bottom = min x, min y, max x,
    max y, on the device, for deca.crop_matrix."""
    if not torch.is_tensor(pts_img) or pts_img.dim() != 3 or tuple(pts_img.shape[1:]) != (POINTS, 2) or pts_img.shape[0] < 1:
        raise ValueError('landmarks: expected [B,68,2] points, got %s' % (tuple(pts_img.shape) if torch.is_tensor(pts_img) else
                                                                          type(pts_img),))
    N.require_device(pts_img)
    p = N.f32c(pts_img.detach())
    boxes = torch.empty((p.shape[0], 4), dtype=torch.float32, device=p.device)
    N.call('sgdfr_fan_boxes_f32', N.ptr(p), p.shape[0], N.ptr(boxes), N.stream())
    return boxes

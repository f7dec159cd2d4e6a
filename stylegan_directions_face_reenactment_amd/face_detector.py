"""The S3FD face detector on the HIP kernels of csrc/s3fd.hip: the counterpart of libs/face_models/sfd/net_s3fd.py `s3fd`, of
detect.py batch_detect (:36-81) with bbox.py decode (:93-111) and nms (:44-66), of SFDDetector.detect_from_batch
(sfd_detector.py:31-47) and of the face choice in front of the landmark network (LandmarksEstimation.detect_landmarks,
landmarks_estimation.py:187-209; face_alignment's first box behind libs/DECA/decalib/datasets/detectors.py FAN.run).

    det = S3FD(); det.load_state_dict(torch.load('s3fd-619a316812.pth')); det = det.cuda()     # loads unchanged, strict=True
    boxes, kept, valid = detect(det, images)                    # [B,capacity,5], [B], [B] on the device, no synchronisation
    lists = detect_from_batch(det, images)                      # SFDDetector.detect_from_batch's lists (synchronises)
    pts_img, kpt_boxes, has_face = detect_landmarks(det, fan, images)           # image -> 68 landmarks -> deca.crop_matrix's box

`S3FD` has the module layout and the 65 state-dict keys of the reference's and holds the weights only, frozen at construction; the
kernels run it forward only: a box is a decision, nothing differentiates it.  Images are [B,3,H,W] float32 with 0..255 values, as
batch_detect takes them; `subtract_mean` (off by default) is the (104, 117, 123) subtraction that only the reference's unused
detect() applies.  The whole batch runs in one pass with per-image semantics: row b gives what the reference gives for image b
alone (at B > 1 the reference's candidate lists hold every position at which any image passes, once per passing image; the
duplicates and the rows at or below 0.05 vanish in its NMS and final filter, so its final lists are the per-image ones).  Candidate
lists, counts and boxes stay on the device: a list longer than `capacity` is cut and its row marked in `valid`.  `detect` thresholds
at 0.5 in front of the NMS (a box is never suppressed by a lower-scoring one, so the survivors above 0.5 are the same); `candidates`
keeps the reference's 0.05.  The device pack (~90 MB) is rebuilt whenever a parameter's storage or version changes.
"""
import ctypes
from collections import OrderedDict

import torch
from torch import nn

from . import _native as N
from . import landmarks as L
from .packs import PackedWeights, views

LEVELS = 6
CAPACITY = 1024
MEAN = (104.0, 117.0, 123.0)
RULES = ('first', 'last_above_0.99')
TRUNK = ('conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1',
         'conv5_2', 'conv5_3', 'fc6', 'fc7', 'conv6_1', 'conv6_2', 'conv7_1', 'conv7_2')
HEADS = ('conv3_3_norm', 'conv4_3_norm', 'conv5_3_norm', 'fc7', 'conv6_2', 'conv7_2')          # + '_mbox_conf' / '_mbox_loc'
DEBUG_TAPS = (('conv1_2', 64), ('conv2_2', 128), ('conv3_3', 256), ('conv4_3', 512), ('conv5_3', 512), ('fc6', 1024), ('fc7', 1024),
              ('conv6_2', 512), ('conv7_2', 256))


class L2Norm(nn.Module):
    """net_s3fd.py L2Norm: x / (sqrt(sum_c x^2) + 1e-10) * weight[c].  Weights only."""

    def __init__(self, n_channels, scale=1.0):
        super().__init__()
        self.n_channels, self.scale, self.eps = n_channels, scale, 1e-10
        self.weight = nn.Parameter(torch.full((n_channels,), float(scale)))


class S3FD(PackedWeights, nn.Module):
    """net_s3fd.s3fd: weights only.  forward(images [B,3,H,W], 0..255) -> the twelve maps [cls1, reg1, ..., cls6, reg6]."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_s3fd_prepack_f32', 'sgdfr_s3fd_pack_elems', N.S3FD_PARAMS
    # no TRAIN_ERROR: the network has no BatchNorm and no Dropout, train mode changes nothing
    GRAD_ERROR = ('S3FD: the HIP kernels are forward only and give no gradient for the weights; keep every parameter at '
                  'requires_grad=False')

    def __init__(self):
        super().__init__()
        c = nn.Conv2d
        self.conv1_1, self.conv1_2 = c(3, 64, 3, 1, 1), c(64, 64, 3, 1, 1)
        self.conv2_1, self.conv2_2 = c(64, 128, 3, 1, 1), c(128, 128, 3, 1, 1)
        self.conv3_1, self.conv3_2, self.conv3_3 = c(128, 256, 3, 1, 1), c(256, 256, 3, 1, 1), c(256, 256, 3, 1, 1)
        self.conv4_1, self.conv4_2, self.conv4_3 = c(256, 512, 3, 1, 1), c(512, 512, 3, 1, 1), c(512, 512, 3, 1, 1)
        self.conv5_1, self.conv5_2, self.conv5_3 = c(512, 512, 3, 1, 1), c(512, 512, 3, 1, 1), c(512, 512, 3, 1, 1)
        self.fc6, self.fc7 = c(512, 1024, 3, 1, 3), c(1024, 1024, 1, 1, 0)
        self.conv6_1, self.conv6_2 = c(1024, 256, 1, 1, 0), c(256, 512, 3, 2, 1)
        self.conv7_1, self.conv7_2 = c(512, 128, 1, 1, 0), c(128, 256, 3, 2, 1)
        self.conv3_3_norm, self.conv4_3_norm, self.conv5_3_norm = L2Norm(256, 10), L2Norm(512, 8), L2Norm(512, 5)
        for name, ch, conf in (('conv3_3_norm', 256, 4), ('conv4_3_norm', 512, 2), ('conv5_3_norm', 512, 2), ('fc7', 1024, 2),
                               ('conv6_2', 512, 2), ('conv7_2', 256, 2)):
            self.add_module(name + '_mbox_conf', c(ch, conf, 3, 1, 1))
            self.add_module(name + '_mbox_loc', c(ch, 4, 3, 1, 1))
        for p in self.parameters():
            p.requires_grad = False

    # ---- weights
    def folded(self, dtype=torch.float32):
        """The 50 tensors sgdfr_s3fd_prepack_f32 takes: the 19 trunk convs' w, b, then per level conf and loc concatenated to one
        conv's w [conf+4,C,3,3], b [conf+4], the L2Norm weight of levels 0-2 folded in per input channel in fp64."""
        out = []
        for name in TRUNK:
            m = getattr(self, name)
            out += [m.weight.detach().double(), m.bias.detach().double()]
        for name in HEADS:
            conf, loc = getattr(self, name + '_mbox_conf'), getattr(self, name + '_mbox_loc')
            w = torch.cat([conf.weight.detach().double(), loc.weight.detach().double()], 0)
            if name.endswith('_norm'):
                w = w * getattr(self, name).weight.detach().double().view(1, -1, 1, 1)
            out += [w, torch.cat([conf.bias.detach().double(), loc.bias.detach().double()], 0)]
        return [v.to(dtype).contiguous() for v in out]

    def forward(self, images):
        return network(self, images)


# ---------------------------------------------------------------------------------------------------------------- checks
def _check_images(images):
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError('face_detector: expected [B,3,H,W] images, got %s' % (tuple(images.shape) if torch.is_tensor(images) else
                                                                              type(images),))
    if images.shape[2] < 32 or images.shape[3] < 32:
        raise ValueError('face_detector: images of %dx%d are too small, each side must be at least 32' % tuple(images.shape[2:]))


def _check_capacity(capacity):
    if not isinstance(capacity, int) or isinstance(capacity, bool) or not 1 <= capacity <= 16384:
        raise ValueError('face_detector: capacity must be an integer in 1..16384, got %r' % (capacity,))


def _check_threshold(threshold):
    if not isinstance(threshold, (int, float)) or isinstance(threshold, bool) or not 0.0 <= float(threshold) < 1.0:
        raise ValueError('face_detector: threshold must be a number in [0, 1), got %r' % (threshold,))


def level_dims(H, W):
    """[(h, w)] of the six level maps for an H x W image (fc6's padding of 3 makes levels 3-5 larger than their stride implies)."""
    hw = (ctypes.c_int * (2 * LEVELS))()
    N.call('sgdfr_s3fd_level_dims', int(H), int(W), hw)
    return [(hw[2 * l], hw[2 * l + 1]) for l in range(LEVELS)]


def _workspace(rows, H, W, device):
    return N.workspace('sgdfr_s3fd_workspace_bytes', device, rows, H, W,
                       error='face_detector: unsupported batch of %d images of %dx%d (1..256 rows, each side 32..4096, '
                             'rows*H*W <= 2^24)' % (rows, H, W))


def map_views(maps, rows, H, W):
    """The flat map buffer as the twelve tensors of s3fd.forward: cls1 [B,2,h,w], reg1 [B,4,h,w], ..."""
    cut = views(maps, rows)
    out = [cut((c, h, w)) for h, w in level_dims(H, W) for c in (2, 4)]
    cut.done()
    return out


def debug_views(debug, rows, H, W):
    """The debug buffer as named views (csrc/s3fd.hip's DebugLayout): the nine trunk taps, then rnorm3, rnorm4, rnorm5 [B,h,w]."""
    dims = level_dims(H, W)
    h, w = H, W
    sizes = {}
    sizes['conv1_2'] = (h, w)
    sizes['conv2_2'] = (h // 2, w // 2)
    sizes['conv3_3'], sizes['conv4_3'], sizes['conv5_3'], sizes['fc7'], sizes['conv6_2'], sizes['conv7_2'] = dims
    sizes['fc6'] = dims[3]
    out, cut = OrderedDict(), views(debug, rows)
    for name, ch in DEBUG_TAPS:
        out[name] = cut((ch,) + sizes[name])
    for l, name in enumerate(('rnorm3', 'rnorm4', 'rnorm5')):
        out[name] = cut(dims[l])
    cut.done()
    return out


# ---------------------------------------------------------------------------------------------------------------- calls
def _prepare(det, images):
    det.check()
    _check_images(images)
    N.require_device(images)
    return N.f32c(images.detach())


def network(det, images, subtract_mean=False):
    """s3fd.forward for a batch: the twelve maps [cls1, reg1, ..., cls6, reg6] in float32 on the device; cls1 is returned after the
    max-out of its three background logits, as the reference returns it."""
    x = _prepare(det, images)
    B, _, H, W = x.shape
    ws, nbytes = _workspace(B, H, W, x.device)
    maps = torch.empty(N.load().sgdfr_s3fd_map_elems(B, H, W), dtype=torch.float32, device=x.device)
    N.call('sgdfr_s3fd_network_f32', N.ptr(x), B, H, W, int(bool(subtract_mean)), N.ptr(det.packed()), N.ptr(maps), None, N.ptr(ws),
           nbytes, N.stream())
    return map_views(maps, B, H, W)


def _forward(det, images, subtract_mean, threshold, capacity, select, want_maps, debug):
    x = _prepare(det, images)
    _check_threshold(threshold)
    _check_capacity(capacity)
    B, _, H, W = x.shape
    dev = x.device
    lib = N.load()
    ws, nbytes = _workspace(B, H, W, dev)
    cand = torch.zeros((B, capacity, 5), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    boxes = torch.empty((B, capacity, 5), dtype=torch.float32, device=dev) if select else None
    index = torch.empty((B, capacity), dtype=torch.int32, device=dev) if select else None
    kept = torch.empty(B, dtype=torch.int32, device=dev) if select else None
    maps = torch.empty(lib.sgdfr_s3fd_map_elems(B, H, W), dtype=torch.float32, device=dev) if want_maps else None
    dbg = torch.empty(lib.sgdfr_s3fd_debug_elems(B, H, W), dtype=torch.float32, device=dev) if debug else None
    N.call('sgdfr_s3fd_forward_f32', N.ptr(x), B, H, W, int(bool(subtract_mean)), N.ptr(det.packed()), float(threshold), capacity,
           N.ptr(cand), N.ptr(count), N.ptr(valid), N.ptr(boxes), N.ptr(index), N.ptr(kept), N.ptr(maps), N.ptr(dbg), N.ptr(ws), nbytes,
           N.stream())
    return {'cand': cand, 'count': count, 'valid': valid, 'boxes': boxes, 'index': index, 'kept': kept,
            'maps': None if maps is None else map_views(maps, B, H, W), 'debug': None if dbg is None else debug_views(dbg, B, H, W)}


def run_debug(det, images, subtract_mean=False, threshold=0.05, capacity=CAPACITY):
    """One pass with everything switched on -> dict: maps (the twelve), debug (debug_views), cand / count / valid at `threshold`,
    boxes / index / kept of the selection.  For tests."""
    return _forward(det, images, subtract_mean, threshold, capacity, True, True, True)


def candidates(det, images, threshold=0.05, capacity=CAPACITY, subtract_mean=False):
    """batch_detect's list per image: cand [B,capacity,5] = x1, y1, x2, y2, score of the positions with score > threshold in
    (level, y, x) order (zeros behind), count [B] int32 = the true number, valid [B] int32 = 0 where count > capacity."""
    r = _forward(det, images, subtract_mean, threshold, capacity, False, False, False)
    return r['cand'], r['count'], r['valid']


def candidates_from_heads(heads, threshold=0.05, capacity=CAPACITY):
    """The decode alone on six raw head outputs, level l [B, conf+4, h_l, w_l] with conf = 4 at level 0 and 2 behind it (conf
    channels first) -> (cand, count, valid) as `candidates`."""
    _check_threshold(threshold)
    _check_capacity(capacity)
    if len(heads) != LEVELS:
        raise ValueError('face_detector: expected six head outputs, got %d' % len(heads))
    B = heads[0].shape[0] if torch.is_tensor(heads[0]) and heads[0].dim() == 4 else 0
    hs = []
    for l, h in enumerate(heads):
        ch = (4 if l == 0 else 2) + 4
        if not torch.is_tensor(h) or h.dim() != 4 or h.shape[0] != B or B < 1 or h.shape[1] != ch or h.shape[2] < 1 or h.shape[3] < 1:
            raise ValueError('face_detector: level %d: expected [B,%d,h,w], got %s' % (l, ch, tuple(h.shape) if torch.is_tensor(h) else
                                                                                      type(h)))
        N.require_device(h)
        hs.append(N.f32c(h.detach()))
    dev = hs[0].device
    cand = torch.zeros((B, capacity, 5), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    ptrs = (ctypes.c_void_p * LEVELS)(*[h.data_ptr() for h in hs])
    hw = (ctypes.c_int * (2 * LEVELS))(*[int(v) for h in hs for v in h.shape[2:]])
    N.call('sgdfr_s3fd_candidates_f32', ptrs, hw, B, float(threshold), capacity, N.ptr(cand), N.ptr(count), N.ptr(valid), N.stream())
    return cand, count, valid


def nms(cand, count):
    """detect_from_batch's selection on candidate lists: cand [B,capacity,5], count [B] int32 (a count beyond capacity selects among
    the first `capacity`) -> boxes [B,capacity,5] in descending score order (zeros behind the kept ones), index [B,capacity] int32 =
    each kept box's candidate index (-1 behind), kept [B] int32."""
    if not torch.is_tensor(cand) or cand.dim() != 3 or cand.shape[2] != 5 or cand.shape[0] < 1:
        raise ValueError('face_detector: expected [B,capacity,5] candidates, got %s' % (tuple(cand.shape) if torch.is_tensor(cand) else
                                                                                       type(cand),))
    B, capacity = int(cand.shape[0]), int(cand.shape[1])
    _check_capacity(capacity)
    if not torch.is_tensor(count) or tuple(count.shape) != (B,):
        raise ValueError('face_detector: expected [%d] counts, got %s' % (B, tuple(count.shape) if torch.is_tensor(count) else type(count)))
    N.require_device(cand)
    N.require_device(count, dtype=torch.int32)
    c = N.f32c(cand.detach())
    n = N.f32c(count)
    boxes = torch.empty_like(c)
    index = torch.empty((B, capacity), dtype=torch.int32, device=c.device)
    kept = torch.empty(B, dtype=torch.int32, device=c.device)
    N.call('sgdfr_s3fd_nms_f32', N.ptr(c), N.ptr(n), B, capacity, N.ptr(boxes), N.ptr(index), N.ptr(kept), N.stream())
    return boxes, index, kept


def detect(det, images, capacity=CAPACITY, subtract_mean=False):
    """SFDDetector.detect_from_batch on the device: boxes [B,capacity,5] = x1, y1, x2, y2, score in descending score order (zeros
    behind the kept ones), kept [B] int32, valid [B] int32 (0: more than `capacity` positions passed 0.5 and the list was cut).
    No host synchronisation."""
    r = _forward(det, images, subtract_mean, 0.5, capacity, True, False, False)
    return r['boxes'], r['kept'], r['valid']


def detect_from_batch(det, images, capacity=CAPACITY, subtract_mean=False):
    """SFDDetector.detect_from_batch's result: per image a list of [x1, y1, x2, y2, score] float32 arrays in descending score order
    (an empty list where nothing is found).  SYNCHRONISES with the host (the lists have data-dependent lengths); raises if an
    image's list was cut at `capacity`."""
    boxes, kept, valid = detect(det, images, capacity, subtract_mean)
    boxes, kept, valid = boxes.cpu().numpy(), kept.cpu().tolist(), valid.cpu().tolist()
    if not all(valid):
        raise RuntimeError('face_detector: more than capacity=%d positions above 0.5 in image(s) %s' % (
            capacity, [b for b, v in enumerate(valid) if not v]))
    return [[boxes[b, i] for i in range(kept[b])] for b in range(len(kept))]


def select_face(boxes, kept, rule='first'):
    """One face per image from `detect`'s output -> (faces [B,5], has_face [B] bool), on the tensors' device without synchronisation.
    'first': the highest score, face_alignment's out[0] behind detectors.FAN.run.  'last_above_0.99': the last box in descending
    order whose score exceeds 0.99, what LandmarksEstimation.detect_landmarks (:203-207) leaves in landmarks[0].  Rows without such a
    face get has_face = False and a zero box."""
    if rule not in RULES:
        raise ValueError("face_detector: rule must be one of %s, got %r" % (RULES, rule))
    if not torch.is_tensor(boxes) or boxes.dim() != 3 or boxes.shape[2] != 5 or boxes.shape[1] < 1:
        raise ValueError('face_detector: expected [B,capacity,5] boxes, got %s' % (tuple(boxes.shape) if torch.is_tensor(boxes) else
                                                                                  type(boxes),))
    if not torch.is_tensor(kept) or tuple(kept.shape) != (boxes.shape[0],):
        raise ValueError('face_detector: expected [%d] kept counts, got %s' % (boxes.shape[0], tuple(kept.shape) if torch.is_tensor(kept)
                                                                              else type(kept)))
    n = kept.to(torch.int64)
    if rule == 'last_above_0.99':
        live = torch.arange(boxes.shape[1], device=boxes.device).view(1, -1) < n.view(-1, 1)
        n = ((boxes[:, :, 4] > 0.99) & live).sum(1)
        at = (n - 1).clamp(min=0)
    else:
        at = torch.zeros_like(n)
    has = n > 0
    faces = boxes.gather(1, at.view(-1, 1, 1).expand(-1, 1, 5))[:, 0]
    return faces * has.view(-1, 1).to(faces.dtype), has


def detect_landmarks(det, fan, images, rule='first', input_range='255', capacity=CAPACITY, flip_input=False, depth_net=None):
    """Image -> face box -> 68 landmarks -> 'kpt68' box on one stream with no host round trip: detect, select_face,
    landmarks.get_landmarks, landmarks.kpt68_boxes.  images [B,3,H,W] float32: 0..255 values (input_range='255') or GAN-range [-1,1]
    (input_range='gan': mapped to 0..255 in front of the detector, as in front of the landmark network).
    Returns (pts_img [B,68,2], boxes [B,4] for deca.crop_matrix, has_face [B] bool); rows with has_face False found no face under
    `rule` and their landmarks and boxes mean nothing.  flip_input adds the mirrored pass of the landmark network; with `depth_net`
    (landmarks.ResNetDepth) the landmarks are the 3D type's, pts_img [B,68,3], and the box comes from its first two columns."""
    if input_range not in L.RANGES:
        raise ValueError("face_detector: input_range must be '255' or 'gan', got %r" % (input_range,))
    _check_images(images)
    x255 = images if input_range == '255' else (images.clamp(-1, 1) + 1) / (2 + 1e-5) * 255.0
    boxes, kept, _ = detect(det, x255, capacity)
    faces, has = select_face(boxes, kept, rule)
    if depth_net is not None:
        pts_img, _, _ = L.get_landmarks_3d(fan, depth_net, images, faces, input_range=input_range, flip_input=flip_input)
        return pts_img, L.kpt68_boxes(pts_img[..., :2]), has
    pts_img, _, _ = L.get_landmarks(fan, images, faces, input_range=input_range, flip_input=flip_input)
    return pts_img, L.kpt68_boxes(pts_img), has

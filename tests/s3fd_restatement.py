"""Plain-torch / numpy restatement of the face-detector path (stylegan_directions_face_reenactment_amd/face_detector.py,
csrc/s3fd.hip): the S3FD network (VGG-16 trunk with floor max-pools, fc6 with padding 3, the two stride-2 extras, L2Norm on the
three shallow taps, one conf and one loc conv per level, max-out of level 0's background logits), the candidate decode (softmax
score, threshold, prior of stride 2^(l+2) and size 4 strides, variances 0.1 / 0.2, (level, y, x) order) and the selection (greedy
NMS at IoU 0.3 with "+ 1" areas in descending score order, then score > 0.5), with every decision exposed.  `network` runs in any
dtype on any device (fp64 on the CPU for the fixture checks, fp32 on the GPU as the MIOpen baseline); decode and selection run on
the CPU in the dtype of the maps."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

LEVELS = 6
MEAN = (104.0, 117.0, 123.0)
TRUNK = ('conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1',
         'conv5_2', 'conv5_3', 'fc6', 'fc7', 'conv6_1', 'conv6_2', 'conv7_1', 'conv7_2')
POOL_AFTER = ('conv1_2', 'conv2_2', 'conv3_3', 'conv4_3', 'conv5_3')
GEOMETRY = {'fc6': (1, 3), 'conv6_2': (2, 1), 'conv7_2': (2, 1)}          # (stride, padding) where not (1, kernel // 2)
HEADS = ('conv3_3_norm', 'conv4_3_norm', 'conv5_3_norm', 'fc7', 'conv6_2', 'conv7_2')
HEAD_TAPS = ('conv3_3', 'conv4_3', 'conv5_3', 'fc7', 'conv6_2', 'conv7_2')
TAPS = ('conv1_2', 'conv2_2', 'conv3_3', 'conv4_3', 'conv5_3', 'fc6', 'fc7', 'conv6_2', 'conv7_2', 'rnorm3', 'rnorm4', 'rnorm5')

# fixture cases: name -> (rows, H, W, subtract_mean).  72 x 104: 2*72*104 pixels are no multiple of the 64-pixel tile, the 9 x 13 map
# pools to 4 x 6 with a row and a column dropped, fc6 turns 2 x 3 into 6 x 7.  96 x 128: every pool is even.
CASES = OrderedDict([('a', (2, 72, 104, False)), ('b', (2, 96, 128, False)), ('m', (1, 72, 104, True))])
LEVEL_DIMS = {(72, 104): [(18, 26), (9, 13), (4, 6), (6, 7), (3, 4), (2, 2)], (96, 128): [(24, 32), (12, 16), (6, 8), (7, 8), (4, 4), (2, 2)]}


def images(S, seed, key, B, H, W):
    """Seeded [B,3,H,W] float32 images with 0..255 values under the counter key `key`: noise plus a smooth component."""
    x = S.counter_tensor(seed, key, (B, 3, H, W), 127.5, 60.0).clamp(0, 255)
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ph = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    x = (0.5 * x + 127.5 * (0.5 + 0.5 * torch.sin(6.0 * xx + 2.0 * yy + 1.7 * ph) * torch.cos(5.0 * yy - 0.9 * ph))).clamp(0, 255)
    return x.contiguous()


def fixture_inputs(S, seed, name):
    """(images [B,3,H,W] float32 with 0..255 values, subtract_mean) of a fixture case, regenerated from its counter key."""
    B, H, W, sub = CASES[name]
    return images(S, seed, 's3fd.case.%s.images' % name, B, H, W), sub


# ---------------------------------------------------------------------------------------------------------------- network
def network(state, x, subtract_mean=False):
    """The network as the module is written, in the dtype and on the device of x -> dict: the TAPS, 'heads' (per level the raw
    conf and loc outputs concatenated, [B, conf+4, h, w]) and 'maps' (the twelve outputs, cls1 after the max-out)."""
    P = {k: v.to(device=x.device, dtype=x.dtype) for k, v in state.items()}
    out = OrderedDict()
    h = x
    if subtract_mean:                  # detect(): img - mean in float64, then .float(): the network sees float32 values in any dtype
        h = (x.double() - torch.tensor(MEAN, dtype=torch.float64, device=x.device).view(1, 3, 1, 1)).float().to(x.dtype)
    for name in TRUNK:
        w = P[name + '.weight']
        stride, pad = GEOMETRY.get(name, (1, w.shape[2] // 2))
        h = F.relu(F.conv2d(h, w, P[name + '.bias'], stride=stride, padding=pad))
        out[name] = h
        if name in POOL_AFTER:
            h = F.max_pool2d(h, 2, 2)
    heads, maps = [], []
    for l, (head, tap) in enumerate(zip(HEADS, HEAD_TAPS)):
        f = out[tap]
        if l < 3:
            rn = 1.0 / (f.pow(2).sum(1).sqrt() + 1e-10)
            out['rnorm%d' % (l + 3)] = rn
            f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10) * P[head + '.weight'].view(1, -1, 1, 1)
        conf = F.conv2d(f, P[head + '_mbox_conf.weight'], P[head + '_mbox_conf.bias'], padding=1)
        loc = F.conv2d(f, P[head + '_mbox_loc.weight'], P[head + '_mbox_loc.bias'], padding=1)
        heads.append(torch.cat([conf, loc], 1))
        if l == 0:
            conf = torch.cat([conf[:, :3].max(1, keepdim=True).values, conf[:, 3:]], 1)
        maps += [conf, loc]
    taps = OrderedDict((k, out[k]) for k in TAPS)
    taps['heads'], taps['maps'] = heads, maps
    return taps


def tap_checksum(t):
    """(mean, mean |.|, an 8 x 8 window of row 0's first plane from the map's corner) of a tap in float64, as one vector of 66."""
    d = t.detach().double().cpu()
    plane = d[0, 0] if d.dim() == 4 else d[0]
    win = torch.zeros(8, 8, dtype=torch.float64)
    hh, ww = min(8, plane.shape[0]), min(8, plane.shape[1])
    win[:hh, :ww] = plane[:hh, :ww]
    return torch.cat([d.mean().view(1), d.abs().mean().view(1), win.flatten()]).numpy()


# ---------------------------------------------------------------------------------------------------------------- decode
def scores_of(maps):
    """Per level the softmax score of channel 1, [B, h, w]."""
    return [torch.softmax(maps[2 * l], dim=1)[:, 1] for l in range(LEVELS)]


def decode_image(maps, b, threshold=0.05):
    """The candidate list of image b in (level, y, x) order -> dict: dets [n,5] (x1, y1, x2, y2, score) as numpy in the maps' dtype,
    level / y / x [n], loc [n,4].  Arithmetic in the order of bbox.decode: centre = prior + loc * 0.1 * size, size * exp(loc * 0.2),
    corner = centre - size / 2, opposite corner = size + corner."""
    dets, lv, ys, xs, locs = [], [], [], [], []
    for l in range(LEVELS):
        cls, reg = maps[2 * l][b:b + 1].cpu(), maps[2 * l + 1][b].cpu()
        score = torch.softmax(cls, dim=1)[0, 1]
        stride = 2 ** (l + 2)
        for y, x in torch.nonzero(score > threshold).tolist():          # row-major
            loc = reg[:, y, x].contiguous().view(1, 4)
            prior = torch.tensor([[stride / 2 + x * stride, stride / 2 + y * stride]], dtype=torch.float32)
            size = torch.tensor([[stride * 4.0, stride * 4.0]], dtype=torch.float32)
            c = prior + loc[:, :2] * 0.1 * size
            wh = size * torch.exp(loc[:, 2:] * 0.2)
            lo = c - wh / 2
            hi = wh + lo
            dets.append(torch.cat([lo[0], hi[0], score[y, x].view(1).to(lo.dtype)]))
            lv.append(l), ys.append(y), xs.append(x), locs.append(loc[0])
    dt = maps[0].dtype
    n = len(dets)
    return {'dets': (torch.stack(dets) if n else torch.zeros(0, 5, dtype=dt)).numpy(),
            'level': np.array(lv, dtype=np.int64), 'y': np.array(ys, dtype=np.int64), 'x': np.array(xs, dtype=np.int64),
            'loc': (torch.stack(locs) if n else torch.zeros(0, 4, dtype=dt)).numpy()}


def iou_plus_one(a, b):
    """IoU of two boxes with the '+ 1' convention of bbox.nms, in the dtype of the boxes."""
    one = a.dtype.type(1)
    w = max(a.dtype.type(0), min(a[2], b[2]) - max(a[0], b[0]) + one)
    h = max(a.dtype.type(0), min(a[3], b[3]) - max(a[1], b[1]) + one)
    inter = w * h
    return inter / ((a[2] - a[0] + one) * (a[3] - a[1] + one) + (b[2] - b[0] + one) * (b[3] - b[1] + one) - inter)


def greedy_nms(dets, thresh=0.3):
    """Greedy suppression in descending score order (ties: lower index first) -> (order, keep, compared): the sorted candidate
    indices, the kept ones in that order, and every IoU the pass compared against `thresh` as (kept index, other index, IoU)."""
    order = sorted(range(len(dets)), key=lambda i: (-dets[i, 4], i))
    dead, keep, compared = set(), [], []
    for pos, i in enumerate(order):
        if i in dead:
            continue
        keep.append(i)
        for j in order[pos + 1:]:
            if j in dead:
                continue
            v = iou_plus_one(dets[i], dets[j])
            compared.append((i, j, float(v)))
            if v > dets.dtype.type(thresh):
                dead.add(j)
    return order, keep, compared


def select(dets, floor=None):
    """detect_from_batch for one image's candidate list: NMS at 0.3, then score > 0.5 -> (kept candidate indices in descending score
    order, boxes [k,5]).  floor: drop the candidates at or below it in front of the NMS (the device path's order of the two steps)."""
    ids = np.arange(len(dets)) if floor is None else np.nonzero(dets[:, 4] > floor)[0]
    _, keep, _ = greedy_nms(dets[ids])
    kept = [int(ids[i]) for i in keep if dets[ids[i], 4] > 0.5]
    return kept, dets[kept] if kept else np.zeros((0, 5), dtype=dets.dtype)


def batch_quirk_lists(maps, threshold=0.05):
    """What batch_detect builds at B > 1: `np.where(ocls[:, 1] > 0.05)` runs over the whole batch, so image j's list holds, per
    level, every position at which ANY image passes, once per passing image, with image j's own score and box."""
    B = maps[0].shape[0]
    score = scores_of([m.cpu() for m in maps])
    lists = [[] for _ in range(B)]
    for l in range(LEVELS):
        stride = 2 ** (l + 2)
        for _, y, x in torch.nonzero(score[l] > threshold).tolist():
            for j in range(B):
                loc = maps[2 * l + 1][j, :, y, x].cpu().view(1, 4)
                prior = torch.tensor([[stride / 2 + x * stride, stride / 2 + y * stride]], dtype=torch.float32)
                size = torch.tensor([[stride * 4.0, stride * 4.0]], dtype=torch.float32)
                c = prior + loc[:, :2] * 0.1 * size
                wh = size * torch.exp(loc[:, 2:] * 0.2)
                lo = c - wh / 2
                lists[j].append(torch.cat([lo[0], (wh + lo)[0], score[l][j, y, x].view(1).to(lo.dtype)]).numpy())
    return [np.stack(v) if v else np.zeros((0, 5)) for v in lists]


# ---------------------------------------------------------------------------------------------------------------- hand-made input
def handmade_heads(B=2, dims=((5, 7), (3, 4), (2, 3), (4, 3), (2, 2), (1, 2))):
    """Six raw head outputs with everything far below the threshold except chosen positions: level 0 carries one position per
    background channel holding the maximum (the score must come from max(bg0, bg1, bg2) against the face logit), every level passes
    at its first and its last pixel, and image 1 passes nowhere on levels 1-5.  float32, values exact in binary."""
    heads = []
    for l, (h, w) in enumerate(dims):
        conf = 4 if l == 0 else 2
        t = torch.zeros(B, conf + 4, h, w)
        t[:, :conf - 1] = 6.0                                # background logits
        t[:, conf - 1] = -6.0                                # face logit: score ~ 6e-6
        for b in range(B):
            if b == 1 and l > 0:
                continue
            for (y, x) in ((0, 0), (h - 1, w - 1)):
                t[b, :conf - 1, y, x] = -2.0
                t[b, conf - 1, y, x] = 1.0 + 0.25 * l + 0.125 * b
                t[b, conf:, y, x] = torch.tensor([0.5, -0.25, 0.125 * (l + 1), -0.375])
        if l == 0:
            for k, (y, x) in enumerate(((1, 2), (2, 4), (3, 1))):
                t[:, :3, y, x] = -3.0
                t[:, k, y, x] = 0.5 + 0.125 * k               # the maximum sits in background channel k
                t[:, 3, y, x] = 1.0
                t[:, 4:, y, x] = torch.tensor([-0.5, 0.25, 0.0, 0.5])
        heads.append(t)
    return heads


def maps_of_heads(heads):
    """The twelve maps of raw head outputs (max-out at level 0)."""
    maps = []
    for l, t in enumerate(heads):
        conf = t.shape[1] - 4
        c = t[:, :conf]
        if l == 0:
            c = torch.cat([c[:, :3].max(1, keepdim=True).values, c[:, 3:]], 1)
        maps += [c, t[:, conf:]]
    return maps

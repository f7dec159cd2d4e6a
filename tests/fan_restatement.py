"""Plain-torch restatement of the landmark path (stylegan_directions_face_reenactment_amd/landmarks.py, csrc/fan.hip): centre /
scale / integer window, the zero-padded window resized with F.interpolate, the 2D-FAN-4 network in two forms -- `network` with the
BatchNorms unfolded as the module is written (the stock form: fp64 on the CPU for the fixture checks, fp32 on the GPU as the MIOpen
baseline) and `network_folded`, the form the kernels compute (per-channel g, h applied in front of each conv behind its zero
padding, every conv writing its channel slice of the block output plus the residual slice, b1 after the lower branch with the
upsampled low3 added in the same step, bl and al as one product over the concatenated K) -- and the heatmap decode with its
decisions exposed.  Runs in any dtype on any device."""
import torch
import torch.nn.functional as F

STACKS, DEPTH, POINTS, CROP, MAP = 4, 4, 68, 256, 64
EPS = 1e-5

# fixture cases: name -> (rows, H, W, face boxes x0, y0, x1, y1).  'a': the window leaves the image on the left and at the top and is
# clipped at the right and the bottom edge as well (zero padding and clipping both active).  'b': one window larger than 256 (scaled
# down) and one smaller (scaled up).
CASES = {
    'a': (1, 256, 256, [[-20.0, -35.0, 245.0, 262.0]]),
    'b': (2, 200, 300, [[30.0, 10.0, 268.0, 196.0], [110.0, 60.0, 206.0, 171.0]]),
}


# geometries of the front beyond the fixture's (test_gpu_deca_fan_plans): name -> (rows, H, W, face boxes).  The integer windows
# (GEO_WINDOWS, what `windows` gives for them in float32): 'inside1024' lies wholly inside a large image (pure down-scaling by 3.5),
# 'small96' leaves a small image on every side, 'tiny_up' is 67 pixels wide (up-scaled by 3.8), 'wide' hangs half out of a 120 x 640
# strip, 'outside' misses the image (a zero crop: the heatmaps come from the biases alone), 'huge' holds the image as a speck.
GEO_CASES = {
    'inside1024': (1, 1024, 1024, [[300.0, 280.0, 700.0, 760.0]]),
    'small96': (2, 96, 80, [[20.0, 18.0, 61.0, 70.0], [-4.0, 30.0, 40.0, 90.0]]),
    'tiny_up': (1, 256, 256, [[100.0, 100.0, 130.0, 136.0]]),
    'wide': (1, 120, 640, [[200.0, 5.0, 330.0, 118.0]]),
    'outside': (1, 256, 256, [[900.0, 900.0, 1100.0, 1120.0]]),
    'huge': (1, 64, 64, [[-400.0, -380.0, 470.0, 520.0]]),
}


def images(S, seed, key, B, H, W):
    """Seeded [B,3,H,W] float32 images with 0..255 values under the counter key `key`: noise plus a smooth component, so that the
    crop is not white noise at every scale."""
    x = S.counter_tensor(seed, key, (B, 3, H, W), 127.5, 60.0).clamp(0, 255)
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    x = (0.5 * x + 127.5 * (0.5 + 0.5 * torch.sin(6.0 * xx + 2.0 * yy) * torch.cos(5.0 * yy))).clamp(0, 255)
    return x.contiguous()


def fixture_inputs(S, seed, name):
    """(images [B,3,H,W] float32 with 0..255 values, faces [B,4] float32), regenerated from counter keys."""
    B, H, W, faces = CASES[name]
    return images(S, seed, 'fan.case.%s.images' % name, B, H, W), torch.tensor(faces, dtype=torch.float32)


def geo_inputs(S, seed, name):
    """The same for a GEO_CASES geometry, under the key 'fan.geo.<name>.images'."""
    B, H, W, faces = GEO_CASES[name]
    return images(S, seed, 'fan.geo.%s.images' % name, B, H, W), torch.tensor(faces, dtype=torch.float32)


def to_255(x):
    """image_utils.torch_range_1_to_255."""
    return (x.clamp(-1, 1) + 1) / (2 + 1e-5) * 255.0


def to_gan(x255):
    """A [-1,1] image whose range map gives (about) x255: the 'gan' twin of a 0..255 fixture image."""
    return (x255 / 255.0 * (2 + 1e-5) - 1).clamp(-1, 1)


# ---------------------------------------------------------------------------------------------------------------- geometry
def centre_scale(faces):
    """landmarks_estimation.py:145-150 per row, in the dtype of `faces` (float32: the decisions; float64: the margins)."""
    f = faces
    cx = (f[:, 2] + f[:, 0]) / 2.0
    cy = (f[:, 3] + f[:, 1]) / 2.0
    cy = cy - (f[:, 3] - f[:, 1]) * 0.12
    scale = (f[:, 2] - f[:, 0] + f[:, 3] - f[:, 1]) / 195.0
    return torch.stack([cx, cy], 1), scale


def inv_transform_float(points, centre, scale, resolution):
    """fan_model/utils.py transform(..., invert=True) before its .int(): points [...,2] with centre [2] and scale [] of one row, the
    inverse of [[a,0,tx],[0,a,ty],[0,0,1]] in closed form, in the dtype of centre."""
    h = 200.0 * scale
    a = resolution / h
    t = resolution * (-centre / h + 0.5)
    ia = 1.0 / a
    return ia * points.to(centre.dtype) + (-t * ia)


def inv_transform(points, centre, scale, resolution):
    """... with the .int() truncation (toward zero), as int64."""
    return inv_transform_float(points, centre, scale, resolution).trunc().long()


def windows(faces):
    """Per row the integer window corners (l1x, l1y, l2x, l2y) of crop_torch: transform([1,1]) and transform([256,256]), inverted, in
    float32."""
    c, s = centre_scale(faces.float())
    out = []
    for b in range(faces.shape[0]):
        l1 = inv_transform(torch.tensor([1.0, 1.0]), c[b], s[b], 256.0)
        l2 = inv_transform(torch.tensor([256.0, 256.0]), c[b], s[b], 256.0)
        out.append([int(l1[0]), int(l1[1]), int(l2[0]), int(l2[1])])
    return out


def window_of(image, win):
    """The zero window of crop_torch with the clipped copy of the image [C,H,W] in it: pixel (wy, wx) is image (wy + l1y, wx + l1x)
    where that lies in the image, else 0."""
    l1x, l1y, l2x, l2y = win
    C, H, W = image.shape
    out = image.new_zeros((C, l2y - l1y, l2x - l1x))
    y0, y1, x0, x1 = max(l1y, 0), min(l2y, H), max(l1x, 0), min(l2x, W)
    if y1 > y0 and x1 > x0:
        out[:, y0 - l1y:y1 - l1y, x0 - l1x:x1 - l1x] = image[:, y0:y1, x0:x1]
    return out


def crop(images, faces, input_range='255'):
    """crop_torch per row + / 255 -> [B,3,256,256] in the dtype of `images`; the window decisions are always the float32 ones."""
    x = to_255(images) if input_range == 'gan' else images
    wins = windows(faces)
    out = []
    for b in range(x.shape[0]):
        w = window_of(x[b], wins[b])
        out.append(F.interpolate(w[None], size=(CROP, CROP), mode='bilinear', align_corners=False))
    return torch.cat(out) / 255.0


# ---------------------------------------------------------------------------------------------------------------- network
def _getter(sd, like):
    return lambda k: sd[k].to(device=like.device, dtype=like.dtype)


def _bn(g, p, x):
    return F.batch_norm(x, g(p + '.running_mean'), g(p + '.running_var'), g(p + '.weight'), g(p + '.bias'), False, 0.0, EPS)


def _conv_block(g, p, x, has_ds):
    o1 = F.conv2d(F.relu(_bn(g, p + '.bn1', x)), g(p + '.conv1.weight'), padding=1)
    o2 = F.conv2d(F.relu(_bn(g, p + '.bn2', o1)), g(p + '.conv2.weight'), padding=1)
    o3 = F.conv2d(F.relu(_bn(g, p + '.bn3', o2)), g(p + '.conv3.weight'), padding=1)
    res = x
    if has_ds:
        res = F.conv2d(F.relu(_bn(g, p + '.downsample.0', x)), g(p + '.downsample.2.weight'))
    return torch.cat([o1, o2, o3], 1) + res


def _hourglass(g, p, level, x):
    up1 = _conv_block(g, '%s.b1_%d' % (p, level), x, False)
    low1 = _conv_block(g, '%s.b2_%d' % (p, level), F.avg_pool2d(x, 2, stride=2), False)
    low2 = _hourglass(g, p, level - 1, low1) if level > 1 else _conv_block(g, '%s.b2_plus_%d' % (p, level), low1, False)
    low3 = _conv_block(g, '%s.b3_%d' % (p, level), low2, False)
    return up1 + F.interpolate(low3, scale_factor=2, mode='nearest')


def network(sd, crop_):
    """FAN(4).forward as written (BatchNorm in eval mode, unfolded).  Returns the debug taps of csrc/fan.hip: {'stem', 'conv4',
    'hg': [4], 'heatmaps': [4]}."""
    g = _getter(sd, crop_)
    x = F.relu(_bn(g, 'bn1', F.conv2d(crop_, g('conv1.weight'), g('conv1.bias'), stride=2, padding=3)))
    taps = {'stem': x, 'hg': [], 'heatmaps': []}
    x = F.avg_pool2d(_conv_block(g, 'conv2', x, True), 2, stride=2)
    x = _conv_block(g, 'conv3', x, False)
    prev = _conv_block(g, 'conv4', x, True)
    taps['conv4'] = prev
    for i in range(STACKS):
        hg = _hourglass(g, 'm%d' % i, DEPTH, prev)
        taps['hg'].append(hg)
        ll = _conv_block(g, 'top_m_%d' % i, hg, False)
        ll = F.relu(_bn(g, 'bn_end%d' % i, F.conv2d(ll, g('conv_last%d.weight' % i), g('conv_last%d.bias' % i))))
        hm = F.conv2d(ll, g('l%d.weight' % i), g('l%d.bias' % i))
        taps['heatmaps'].append(hm)
        if i + 1 < STACKS:
            prev = prev + F.conv2d(ll, g('bl%d.weight' % i), g('bl%d.bias' % i)) + F.conv2d(hm, g('al%d.weight' % i), g('al%d.bias' % i))
    return taps


def _gh(g, p):
    s = g(p + '.weight') * torch.rsqrt(g(p + '.running_var') + EPS)
    return s, g(p + '.bias') - g(p + '.running_mean') * s


def _pre(g, p, x):
    """What the conv's loader applies to every tap inside the map: max(0, x g[c] + h[c]); the conv pads with zeros behind it."""
    s, h = _gh(g, p)
    return torch.relu(x * s.view(1, -1, 1, 1) + h.view(1, -1, 1, 1))


def _block_folded(g, p, x, has_ds, up=None):
    """The three convs write their channel slices of the output, each with the residual's slice (and the upsampled `up`) added;
    conv2 and conv3 read the raw values of the conv before."""
    res = F.conv2d(_pre(g, p + '.downsample.0', x), g(p + '.downsample.2.weight')) if has_ds else x
    cout = res.shape[1]
    out = torch.empty_like(res)
    src, c0 = x, 0
    for j in (1, 2, 3):
        raw = F.conv2d(_pre(g, '%s.bn%d' % (p, j), src), g('%s.conv%d.weight' % (p, j)), padding=1)
        n = raw.shape[1]
        v = raw + res[:, c0:c0 + n]
        if up is not None:
            v = v + F.interpolate(up[:, c0:c0 + n], scale_factor=2, mode='nearest')
        out[:, c0:c0 + n] = v
        src, c0 = raw, c0 + n
    assert c0 == cout
    return out


def _hourglass_folded(g, p, level, x):
    low1 = _block_folded(g, '%s.b2_%d' % (p, level), F.avg_pool2d(x, 2, stride=2), False)
    low2 = _hourglass_folded(g, p, level - 1, low1) if level > 1 else _block_folded(g, '%s.b2_plus_%d' % (p, level), low1, False)
    low3 = _block_folded(g, '%s.b3_%d' % (p, level), low2, False)
    return _block_folded(g, '%s.b1_%d' % (p, level), x, False, up=low3)


def network_folded(sd, crop_):
    """The same function in the form the kernels compute; the same taps."""
    g = _getter(sd, crop_)
    s, h = _gh(g, 'bn1')
    x = torch.relu(F.conv2d(crop_, g('conv1.weight') * s.view(-1, 1, 1, 1), g('conv1.bias') * s + h, stride=2, padding=3))
    taps = {'stem': x, 'hg': [], 'heatmaps': []}
    x = F.avg_pool2d(_block_folded(g, 'conv2', x, True), 2, stride=2)
    x = _block_folded(g, 'conv3', x, False)
    prev = _block_folded(g, 'conv4', x, True)
    taps['conv4'] = prev
    for i in range(STACKS):
        hg = _hourglass_folded(g, 'm%d' % i, DEPTH, prev)
        taps['hg'].append(hg)
        top = _block_folded(g, 'top_m_%d' % i, hg, False)
        s, h = _gh(g, 'bn_end%d' % i)
        ll = torch.relu(F.conv2d(top, g('conv_last%d.weight' % i) * s.view(-1, 1, 1, 1), g('conv_last%d.bias' % i) * s + h))
        hm = F.conv2d(ll, g('l%d.weight' % i), g('l%d.bias' % i))
        taps['heatmaps'].append(hm)
        if i + 1 < STACKS:
            w = torch.cat([g('bl%d.weight' % i), g('al%d.weight' % i)], 1)          # K = 256 + 68
            prev = F.conv2d(torch.cat([ll, hm], 1), w, g('bl%d.bias' % i) + g('al%d.bias' % i)) + prev
    return taps


def tap_list(taps):
    """[(name, tensor)] in the order of the debug buffer."""
    out = [('stem', taps['stem']), ('conv4', taps['conv4'])]
    for i in range(STACKS):
        out += [('hg%d' % i, taps['hg'][i]), ('heatmaps%d' % i, taps['heatmaps'][i])]
    return out


def tap_checksum(t):
    """What the fixture keeps of a tap [B,C,H,W]: mean, mean |.| and the 8 x 8 window [20:28, 30:38] of row 0's middle channel (fp64)."""
    import numpy as np
    t = t.double()
    return np.concatenate([[float(t.mean()), float(t.abs().mean())], t[0, t.shape[1] // 2, 20:28, 30:38].reshape(-1).numpy()])


# ---------------------------------------------------------------------------------------------------------------- decode
def decode(hm, faces):
    """get_preds_fromhm (landmarks_estimation.py:50-88, the version with floor_) for hm [B,68,64,64] and face boxes [B,4] ->
    {'idx' [B,68] first maximum in row-major order, 'pts' [B,68,2] float32 crop pixels (preds * 4), 'pts_img' [B,68,2] float32 image
    pixels (truncated), 'pre' [B,68,2] the image coordinates before truncation in the dtype of the centre, 'boxes' [B,4]}."""
    B = hm.shape[0]
    flat = hm.reshape(B, POINTS, -1)
    top = flat.max(2).values
    pos = torch.arange(flat.shape[2], device=hm.device).view(1, 1, -1).expand_as(flat)
    idx = torch.where(flat == top.unsqueeze(2), pos, torch.full_like(pos, flat.shape[2])).min(2).values   # first index of the maximum
    px, py = idx % MAP, idx // MAP
    preds = torch.stack([px + 1, py + 1], 2).to(torch.float32)
    interior = (px > 0) & (px < MAP - 1) & (py > 0) & (py < MAP - 1)
    pxc, pyc = px.clamp(1, MAP - 2), py.clamp(1, MAP - 2)
    at = lambda yy, xx: flat.gather(2, (yy * MAP + xx).unsqueeze(2)).squeeze(2)
    dx = at(pyc, pxc + 1) - at(pyc, pxc - 1)
    dy = at(pyc + 1, pxc) - at(pyc - 1, pxc)
    step = torch.stack([torch.sign(dx), torch.sign(dy)], 2).to(torch.float32) * 0.25
    preds = preds + step * interior.unsqueeze(2).to(torch.float32) - 0.5
    c, s = centre_scale(faces.to(device=hm.device))
    pre = torch.stack([inv_transform_float(preds[b], c[b], s[b], 64.0) for b in range(B)])
    pts_img = pre.trunc().to(torch.float32)
    boxes = torch.cat([pts_img.min(1).values, pts_img.max(1).values], 1)
    return {'idx': idx, 'pts': preds * 4, 'pts_img': pts_img, 'pre': pre, 'boxes': boxes, 'interior': interior, 'dx': dx, 'dy': dy}


def safe_landmarks(hm64, faces, margin):
    """[B,68] bool: the landmarks whose decode cannot depend on a heatmap deviation below margin / 16 -- the rule the fixture's script
    (scripts/make_golden_fan.py) asserts for every landmark of kat13, per landmark: in fp64 the top-2 margin is >= `margin`, both
    neighbour differences of an interior maximum are >= `margin`, and both image coordinates are >= 1e-3 from an integer before
    the truncation (centre and scale in fp64)."""
    B = hm64.shape[0]
    d = decode(hm64, faces)
    top2 = hm64.reshape(B, POINTS, -1).topk(2, dim=2).values
    safe = (top2[..., 0] - top2[..., 1]) >= margin
    safe &= ~d['interior'] | (torch.minimum(d['dx'].abs(), d['dy'].abs()) >= margin)
    c64, s64 = centre_scale(faces.double())
    pre64 = torch.stack([inv_transform_float((d['pts'][b] / 4).double(), c64[b], s64[b], 64.0) for b in range(B)])
    safe &= ((pre64 - pre64.round()).abs() >= 1e-3).all(2)
    return safe


def handmade_heatmaps():
    """[2,68,64,64] heatmaps that walk through the decode's branches: border maxima on every edge and corner, interior maxima with
    every sign of the neighbour differences including zero, exact ties (the first index wins), a constant map."""
    hm = torch.zeros(2, POINTS, MAP, MAP)
    k = 0
    for b in range(2):
        for j in range(POINTS):
            m = hm[b, j]
            m += 0.001 * torch.sin(0.37 * torch.arange(MAP * MAP, dtype=torch.float32) + k).view(MAP, MAP)
            kind = k % 9
            y, x = 1 + (7 * k) % 62, 1 + (11 * k) % 62
            if kind == 0:
                y = 0
            elif kind == 1:
                x = 63
            elif kind == 2:
                y, x = 63, 0
            elif kind == 3:
                m[y, x + 1] = m[y, x - 1] = 0.5                       # zero difference in x: no step
                m[y + 1, x], m[y - 1, x] = 0.25, 0.75
            elif kind == 4:
                m[y, x + 1], m[y, x - 1] = 0.75, 0.25
                m[y + 1, x] = m[y - 1, x] = 0.125                     # zero difference in y
            elif kind == 5:
                m[(y + 9) % 64, (x + 5) % 64] = 1.0                   # an exact tie: the earlier one in row-major order wins
            elif kind == 6:
                m.fill_(0.25)                                         # constant: index 0
                y, x = 0, 0
            elif kind == 7:
                m[y, x + 1], m[y, x - 1], m[y + 1, x], m[y - 1, x] = 0.1, 0.9, 0.9, 0.1
            if kind != 6:
                m[y, x] = 1.0
            k += 1
    faces = torch.tensor([[40.0, 30.0, 221.0, 240.0], [10.5, 20.25, 300.0, 280.75]])
    return hm, faces

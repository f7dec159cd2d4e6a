"""fp64 restatement of the ArcFace identity loss (libs/criteria/id_loss.py:20-34, model_irse.py:9-48, helpers.py:57-121) for the
IDLoss tests: plain torch ops on CPU, returning every intermediate the HIP kernels keep, optionally with the PReLU / SE-ReLU
decisions taken from given masks (the HIP forward's), so that a gradient check does not depend on an fp32-vs-fp64 sign flip."""
import torch
import torch.nn.functional as F

UNITS = [(c, d, 2 if u == 0 else 1) for c, d, n in ((64, 64, 3), (64, 128, 4), (128, 256, 14), (256, 512, 3))
         for u, c in zip(range(n), [c] + [d] * (n - 1))]


def front(x, crop=True):
    """crop [35:223, 32:220] (slice clamping) -> AdaptiveAvgPool2d(112)."""
    if crop:
        x = x[:, :, 35:223, 32:220]
    return F.adaptive_avg_pool2d(x, (112, 112))


def _bn(P, a, pre):
    return F.batch_norm(a, P[pre + '.running_mean'], P[pre + '.running_var'], P[pre + '.weight'], P[pre + '.bias'], False, 0.0, 1e-5)


def _prelu(a, w, mask):
    return F.prelu(a, w) if mask is None else torch.where(mask, a, a * w.view(1, -1, 1, 1))


def backbone(sd, x, crop=True, masks=None):
    """x [B,3,H,W] -> dict: e [B,512], p0, per unit p1 / c2 / g / h / out, v (before l2_norm).  masks: {'p0': bool, 'p1': [24 bool],
    'h': [24 bool]} replacing the sign decisions of the stem PReLU, conv1's PReLU and the SE ReLU."""
    P = {k: v.detach().double().cpu() for k, v in sd.items() if not k.endswith('num_batches_tracked')}
    m = masks or {}
    a = front(x.double(), crop)
    p0 = _bn(P, F.conv2d(a, P['input_layer.0.weight'], padding=1), 'input_layer.1')
    a = _prelu(p0, P['input_layer.2.weight'], m.get('p0'))
    out = {'p0': p0, 'p1': [], 'c2': [], 'g': [], 'h': [], 'out': []}
    for i, (cin, d, s) in enumerate(UNITS):
        pre = 'body.%d.' % i
        p1 = F.conv2d(_bn(P, a, pre + 'res_layer.0'), P[pre + 'res_layer.1.weight'], padding=1)
        c1 = _prelu(p1, P[pre + 'res_layer.2.weight'], m['p1'][i] if 'p1' in m else None)
        c2 = _bn(P, F.conv2d(c1, P[pre + 'res_layer.3.weight'], stride=s, padding=1), pre + 'res_layer.4')
        hp = F.conv2d(c2.mean((2, 3), keepdim=True), P[pre + 'res_layer.5.fc1.weight'])
        h = F.relu(hp) if 'h' not in m else hp * m['h'][i].view(hp.shape)
        g = torch.sigmoid(F.conv2d(h, P[pre + 'res_layer.5.fc2.weight']))
        if cin == d:
            sc = a[:, :, ::s, ::s]
        else:
            sc = _bn(P, F.conv2d(a, P[pre + 'shortcut_layer.0.weight'], stride=s), pre + 'shortcut_layer.1')
        a = c2 * g + sc
        for k, v in (('p1', p1), ('c2', c2), ('g', g.flatten(1)), ('h', h.flatten(1)), ('out', a)):
            out[k].append(v)
    z = _bn(P, a, 'output_layer.0').flatten(1)
    v = F.linear(z, P['output_layer.3.weight'], P['output_layer.3.bias'])
    v = F.batch_norm(v, P['output_layer.4.running_mean'], P['output_layer.4.running_var'], P['output_layer.4.weight'],
                     P['output_layer.4.bias'], False, 0.0, 1e-5)
    out['v'] = v
    out['e'] = v / torch.norm(v, 2, 1, True)
    return out


def id_loss(sd, y_hat, y, crop=True, masks=None):
    """(1 - cos(e(y_hat), e(y).detach())).mean() with nn.CosineSimilarity(dim=1, eps=1e-6)."""
    ex = backbone(sd, y_hat, crop, masks)['e']
    ey = backbone(sd, y, crop)['e'].detach()
    return torch.mean(1 - F.cosine_similarity(ex, ey, dim=1, eps=1e-6))

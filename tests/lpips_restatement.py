"""fp64 restatement of LPIPS-alex v0.1 (libs/criteria/lpips/lpips.py:28-34, networks.py:53-63,78-85, utils.py:6-12) for the LPIPS
tests: plain torch ops on CPU, optionally with the ReLU masks and max-pool choices taken from given activations (the HIP forward's),
so that a gradient check does not depend on an fp32-vs-fp64 mask flip."""
import torch
import torch.nn.functional as F

CONVS = ((0, 4, 2), (3, 1, 2), (6, 1, 1), (8, 1, 1), (10, 1, 1))     # (state-dict index, stride, padding)


def _pool(a, like=None):
    if like is None:
        return F.max_pool2d(a, 3, 2)
    _, idx = F.max_pool2d(like.double(), 3, 2, return_indices=True)
    return a.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)


def taps(sd, x, fixed=None):
    """Five post-ReLU taps of x (fp64).  fixed: five activations whose (> 0) masks and pool argmaxes replace x's own."""
    P = {k: v.detach().double().cpu() for k, v in sd.items()}
    a = (x.double() - P['net.mean']) / P['net.std']
    out = []
    for t, (i, s, p) in enumerate(CONVS):
        if t in (1, 2):
            a = _pool(a, None if fixed is None else fixed[t - 1])
        a = F.conv2d(a, P['net.layers.%d.weight' % i], P['net.layers.%d.bias' % i], s, p)
        a = F.relu(a) if fixed is None else a * (fixed[t].double() > 0)
        out.append(a)
    return out


def normalize(f):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True) + 1e-9) + 1e-10)


def distance(sd, fx, fy):
    res = [F.conv2d((normalize(a) - normalize(b)) ** 2, sd['lin.%d.1.weight' % t].detach().double().cpu()).mean((2, 3), True)
           for t, (a, b) in enumerate(zip(fx, fy))]
    return torch.sum(torch.cat(res, 0)) / fx[0].shape[0]


def lpips(sd, x, y, fixed=None):
    return distance(sd, taps(sd, x, fixed), taps(sd, y))

"""Plain-torch restatement of the e4e W+ encoder (stylegan_directions_face_reenactment_amd/encoder.py, csrc/e4e.hip) that returns
every tap: Encoder4Editing(50, 'ir_se', R) in eval mode, written from the state dict as the module is written (stem, 24
bottleneck_IR_SE units, the two lateral convs with the bilinear resample at align_corners=True, the style heads as stride-2
conv3x3 + LeakyReLU(0.01) chains down to 1x1 and EqualLinear, w0 + delta).  Runs in any dtype on any device: fp64 on the CPU is
the yardstick of the GPU tests; tests/test_cpu_e4e_taps.py pins it to the fixture written from the reference's own module
(tests/golden/kat15_e4e_taps.npz, scripts/make_golden_e4e_taps.py)."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

KAT = 'kat15_e4e_taps.npz'
SEED = 20260929                     # the seed of kat6_e4e (oracle/make_golden.py)
TAPS = ('stem', 'u0', 'u3', 'c1', 'c2', 'c3', 'p2', 'p1', 'h_coarse', 'h_middle', 'h_fine', 'w')
TAP_UNITS = {0: 'u0', 3: 'u3', 6: 'c1', 20: 'c2', 23: 'c3'}
UNITS = 24
COARSE, MIDDLE = 3, 7
# fixture cases: name -> (rows, R, state seed, counter key of the images).  a and c are kat6's w64 and w256.
CASES = OrderedDict([('a', (3, 64, SEED + 1, 'e4e.x64')), ('b', (2, 96, SEED + 2, 'e4e.x96')), ('c', (2, 256, SEED, 'e4e.x'))])


# the plan sweep (tests/test_gpu_s3fd_e4e_plans.py): resolution -> case name.  64, 96 and 256 are the fixture cases; the others are
# seeded here in the same way and exist in no fixture: their yardstick is the fp32 restatement's own deviation from the fp64 one.
SWEEP_CASES = OrderedDict([('r32', (2, 32, SEED + 32, 'e4e.plan.x32')), ('r48', (3, 48, SEED + 48, 'e4e.plan.x48')),
                           ('r80', (2, 80, SEED + 80, 'e4e.plan.x80')), ('r128', (3, 128, SEED + 128, 'e4e.plan.x128'))])
SWEEP = OrderedDict([(32, 'r32'), (48, 'r48'), (64, 'a'), (80, 'r80'), (96, 'b'), (128, 'r128'), (256, 'c')])


def case(name):
    return CASES[name] if name in CASES else SWEEP_CASES[name]


def fixture_inputs(S, name):
    """Images [B,3,R,R] float32 in [-1,1] of a fixture case, regenerated from its counter key."""
    B, R, _, key = case(name)
    return S.counter_tensor(SEED, key, (B, 3, R, R), 0.0, 0.5).clamp_(-1, 1)


def fixture_state(S, name, template):
    """The seeded state of a fixture case; `template` is a state dict with the module's keys and shapes at that resolution."""
    return S.synthetic_encoder_state(template, seed=case(name)[2])


def _bn(P, k, x):
    return F.batch_norm(x, P[k + '.running_mean'], P[k + '.running_var'], P[k + '.weight'], P[k + '.bias'], False, 0.0, 1e-5)


def unit(P, i, x):
    k = 'body.%d' % i
    w1 = P[k + '.res_layer.1.weight']
    stride = 2 if (i == 0 or w1.shape[0] != w1.shape[1]) else 1           # the first unit of each stage
    if (k + '.shortcut_layer.0.weight') in P:
        short = _bn(P, k + '.shortcut_layer.1', F.conv2d(x, P[k + '.shortcut_layer.0.weight'], None, stride))
    else:
        short = x[:, :, ::stride, ::stride]                               # MaxPool2d(1, stride)
    y = F.prelu(F.conv2d(_bn(P, k + '.res_layer.0', x), w1, None, 1, 1), P[k + '.res_layer.2.weight'])
    y = _bn(P, k + '.res_layer.4', F.conv2d(y, P[k + '.res_layer.3.weight'], None, stride, 1))
    g = y.mean((2, 3), keepdim=True)
    g = torch.sigmoid(F.conv2d(F.relu(F.conv2d(g, P[k + '.res_layer.5.fc1.weight'])), P[k + '.res_layer.5.fc2.weight']))
    return y * g + short


def head_vector(P, j, f):
    """The head's [B,512] vector in front of its EqualLinear."""
    k, i = 'styles.%d' % j, 0
    while (k + '.convs.%d.weight' % i) in P:
        f = F.leaky_relu(F.conv2d(f, P[k + '.convs.%d.weight' % i], P[k + '.convs.%d.bias' % i], 2, 1), 0.01)
        i += 2
    assert f.shape[2] == 1 and f.shape[3] == 1, f.shape
    return f.reshape(f.shape[0], -1)


def forward(state, x):
    """All TAPS in the dtype and on the device of x."""
    P = {k: v.to(device=x.device, dtype=x.dtype) for k, v in state.items() if v.is_floating_point()}
    out = OrderedDict()
    h = F.prelu(_bn(P, 'input_layer.1', F.conv2d(x, P['input_layer.0.weight'], None, 1, 1)), P['input_layer.2.weight'])
    out['stem'] = h
    for i in range(UNITS):
        h = unit(P, i, h)
        if i in TAP_UNITS:
            out[TAP_UNITS[i]] = h
    c1, c2, c3 = out['c1'], out['c2'], out['c3']
    out['p2'] = F.interpolate(c3, size=c2.shape[2:], mode='bilinear', align_corners=True) + F.conv2d(c2, P['latlayer1.weight'],
                                                                                                    P['latlayer1.bias'])
    out['p1'] = F.interpolate(out['p2'], size=c1.shape[2:], mode='bilinear', align_corners=True) + F.conv2d(c1, P['latlayer2.weight'],
                                                                                                           P['latlayer2.bias'])
    n = 0
    while ('styles.%d.linear.weight' % n) in P:
        n += 1
    vec = [head_vector(P, j, c3 if j < COARSE else out['p2'] if j < MIDDLE else out['p1']) for j in range(n)]
    out['h_coarse'], out['h_middle'], out['h_fine'] = torch.stack(vec[:COARSE], 1), torch.stack(vec[COARSE:MIDDLE], 1), torch.stack(vec[MIDDLE:], 1)
    rows = []
    for j in range(n):
        wl = P['styles.%d.linear.weight' % j]
        rows.append(F.linear(vec[j], wl * (1.0 / math.sqrt(wl.shape[1])), P['styles.%d.linear.bias' % j]))
    out['w'] = torch.stack([rows[0]] + [rows[0] + d for d in rows[1:]], 1)
    return out

"""Deterministic synthetic generator parameters (no checkpoints exist offline).

The reference ships no weights (``pretrained_models/`` is git-ignored,
/root/reference/.gitignore:1-2), so parity tests, golden fixtures and the bench
all run on synthetic parameters.  The 99 MB state cannot be committed, so it is
regenerated bit-identically wherever it is needed from a counter-based
generator: ``value = f(seed, crc32(key), element_index)``.

Only integer hashing and exact IEEE add/mul are used (no libm transcendental),
so the same float32 values come out on any host CPU / numpy build:

  * 64-bit splitmix finaliser over ``seed ^ key_hash ^ (index+1)*golden``
  * the four 16-bit fields of the hash are summed (Irwin-Hall, n=4) and
    rescaled to zero mean / unit variance -> approximately N(0,1), |x| <= 3.47

Distributions follow the reference's default initialisation
(model.py:135,218-220,294,421: randn weights, randn/lr_mul for the mapping MLP)
except that parameters the reference initialises to *zero* (noise strengths
model.py:280, activation biases fused_act.py:77, ToRGB biases model.py:348) get
small non-zero values so every term of the forward pass is exercised.
"""
import zlib

import numpy as np
import torch

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _mix64(x):
    x = x.copy()
    x ^= x >> np.uint64(30)
    x *= _M1
    x ^= x >> np.uint64(27)
    x *= _M2
    x ^= x >> np.uint64(31)
    return x


def counter_normal(seed, key, n):
    """n approximately-N(0,1) float64 values for (seed, key); exact on any host."""
    kh = np.uint64(zlib.crc32(key.encode()) & 0xFFFFFFFF)
    base = (np.uint64(seed) << np.uint64(32)) ^ kh
    idx = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over='ignore'):
        h = _mix64(_mix64(idx * _GOLDEN + base) ^ (base * _M2))
    m = np.uint64(0xFFFF)
    s = ((h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m)
         + (h >> np.uint64(48))).astype(np.float64)
    # four U{0..65535}: mean 2*65535, var 4*(65536^2-1)/12
    return (s - 2.0 * 65535.0) * (1.0 / np.sqrt((65536.0 ** 2 - 1.0) / 3.0))


def counter_tensor(seed, key, shape, mean=0.0, std=1.0):
    n = int(np.prod(shape)) if len(shape) else 1
    v = counter_normal(seed, key, n) * std + mean
    return torch.from_numpy(v.astype(np.float32).reshape(tuple(shape)))


def _spec(key, lr_mlp):
    """(mean, std) for a Generator state_dict key; None -> keep constructor value."""
    if key.endswith('.kernel'):                       # FIR buffers: constructor values
        return None
    if key.startswith('style.'):
        if key.endswith('.weight'):
            return 0.0, 1.0 / lr_mlp                  # randn / lr_mul (model.py:135)
        return 0.0, 0.1 / lr_mlp                      # bias (zero in the reference) -> b*lr_mul ~ 0.1
    if key.startswith('noises.'):
        return 0.0, 1.0
    if key == 'input.input':
        return 0.0, 1.0
    if key.endswith('modulation.weight'):
        return 0.0, 1.0
    if key.endswith('modulation.bias'):
        return 1.0, 0.1                               # bias_init=1 (model.py:222)
    if key.endswith('conv.weight'):
        return 0.0, 1.0
    if key.endswith('noise.weight'):
        return 0.1, 0.05                              # zero in the reference
    if key.endswith('activate.bias'):
        return 0.0, 0.1                               # zero in the reference
    if key.endswith('.bias'):                         # to_rgb*.bias
        return 0.0, 0.1
    raise KeyError(key)


def synthetic_state_dict(template, seed=0, lr_mlp=0.01):
    """Fill a Generator-shaped state_dict (key -> tensor) with synthetic values.

    `template` is any mapping key -> tensor with the reference's key set
    (SURVEY.md §8 a14); returned tensors are fresh CPU float32.
    """
    out = {}
    for key, t in template.items():
        spec = _spec(key, lr_mlp)
        if spec is None:
            out[key] = t.detach().clone().float().cpu()
        else:
            out[key] = counter_tensor(seed, key, tuple(t.shape), *spec)
    return out


def trained_like_state_dict(template, seed=0, outlier_fraction=0.01, outlier_gain=30.0, bias_sigma=0.5):
    """synthetic_state_dict reshaped towards what a TRAINED g_ema looks like: heavy-tailed weights instead of
    N(0,1) everywhere --
      * every 3x3 conv weight: `outlier_fraction` of its INPUT channels (at least one) multiplied by `outlier_gain` (outlier
        channels that dominate the contraction; a gain on output channels would be undone by the demodulation);
      * every modulation bias of a 3x3 conv (constructor value 1, model.py:216): log-normal, exp(N(0, bias_sigma^2)) -- per-channel
        style magnitudes spread over several binades;
      * ToRGB weights (no demodulation) keep their scale.
    The fp16x3 range plan is calibrated on the first batch; this is the weight set its re-render rate is quoted on
    (tests/test_gpu_generator.py::test_range_plan_on_trained_like_weights, bench.py `range_plan_stress`)."""
    import torch
    out = synthetic_state_dict(template, seed)
    for key, t in out.items():
        if key.endswith('conv.weight') and t.dim() == 5 and t.shape[-1] == 3:
            cin = t.shape[2]
            n = max(1, int(round(outlier_fraction * cin)))
            pick = torch.from_numpy(counter_normal(seed, key + '.outliers', cin)).argsort()[:n]
            t[:, :, pick] *= outlier_gain
        elif key.endswith('conv.modulation.bias') and ('to_rgb' not in key):
            t.copy_(torch.exp(counter_tensor(seed, key + '.lognormal', tuple(t.shape), 0.0, bias_sigma)))
    return out


def synthetic_latents(seed, batch, n_latent=14, style_dim=512, key='wplus', std=1.0):
    """Random W+ codes [B, n_latent, 512] (bench config 2: 'random w+')."""
    return counter_tensor(seed, key, (batch, n_latent, style_dim), 0.0, std)


def synthetic_z(seed, batch, style_dim=512, key='z'):
    return counter_tensor(seed, key, (batch, style_dim))


def synthetic_direction_state(seed, input_dim=15, out_dim=512, num_layers=8, w_plus=True):
    """DirectionMatrix.linear parameters: N(0,0.03) weights (direction_matrix.py:31-32)."""
    rows = out_dim * num_layers if w_plus else out_dim
    return {
        'linear.weight': counter_tensor(seed, 'A.linear.weight', (rows, input_dim), 0.0, 0.03),
        'linear.bias': counter_tensor(seed, 'A.linear.bias', (rows,), 0.0, 0.02),
    }


def synthetic_shape_params(seed, key, n):
    """3DMM parameters shaped like the reference's `calculate_shapemodel` output (libs/utilities/generic.py:22-34):
    (angles [n,3] yaw/pitch/roll in degrees, {'pose': [n,6] (jaw = column 3), 'alpha_exp': [n,50]}) -- the inputs of the
    shift-vector construction; DECA itself is not available offline."""
    ang = counter_tensor(seed, key + '.ang', (n, 3), 0.0, 12.0)
    pose = counter_tensor(seed, key + '.pose', (n, 6), 0.03, 0.08)
    exp = counter_tensor(seed, key + '.exp', (n, 50), 0.1, 0.7)
    return ang, {'pose': pose, 'alpha_exp': exp}


def synthetic_encoder_state(template, seed=0):
    """Fill an Encoder4Editing-shaped state_dict (psp_encoders.py:122-160 key set) with synthetic values:
    conv filters ~ N(0, gain/fan_in) so activations stay O(1) through the 24 residual units and the style heads, BatchNorm statistics near
    (0, 1) with positive variances, PReLU slopes near 0.25, randn EqualLinear weights (lr_mul=1)."""
    out = {}
    for key, t in template.items():
        shape = tuple(t.shape)
        if key.endswith('num_batches_tracked'):
            out[key] = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith('running_var'):
            v = counter_normal(seed, key, int(np.prod(shape))) * 0.2 + 1.0
            out[key] = torch.from_numpy(np.maximum(v, 0.3).astype(np.float32).reshape(shape))
        elif key.endswith('running_mean'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.1)
        elif len(shape) == 4:                                     # conv filters [Cout,Cin/groups,kh,kw]
            fan_in = shape[1] * shape[2] * shape[3]
            gain = 2.0 if key.startswith('styles.') else 0.7     # heads: plain LeakyReLU chains; trunk: residual sums
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(gain / fan_in)))
        elif len(shape) == 2:                                     # EqualLinear weight
            out[key] = counter_tensor(seed, key, shape, 0.0, 1.0)
        elif '.linear.' in key:                                   # EqualLinear bias
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.1)
        elif key.endswith('.bias'):                               # BatchNorm shift / conv bias
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.05)
        elif key.endswith('.weight'):                             # 1-D: BatchNorm scale or PReLU slope
            is_prelu = key.endswith('input_layer.2.weight') or key.endswith('res_layer.2.weight')
            out[key] = counter_tensor(seed, key, shape, 0.25 if is_prelu else 1.0, 0.05 if is_prelu else 0.1)
        else:
            raise KeyError(key)
    return out


def synthetic_lpips_state(seed):
    """Seeded LPIPS-alex state dict in the reference's keys (lpips.LPIPS): conv weights at He scale, small biases, `lin` weights
    |N(0, 0.1)| -- non-negative like the trained heads; mean / std are the constants of networks.py:55-58."""
    from collections import OrderedDict
    chans = (3, 64, 192, 384, 256, 256)
    ks = (11, 5, 3, 3, 3)
    sd = OrderedDict()
    sd['net.mean'] = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    sd['net.std'] = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)
    for t, i in enumerate((0, 3, 6, 8, 10)):
        cin, cout, k = chans[t], chans[t + 1], ks[t]
        sd['net.layers.%d.weight' % i] = counter_tensor(seed, 'lpips.w%d' % i, (cout, cin, k, k), 0.0, (2.0 / (cin * k * k)) ** 0.5)
        sd['net.layers.%d.bias' % i] = counter_tensor(seed, 'lpips.b%d' % i, (cout,), 0.0, 0.01)
    for t in range(5):
        sd['lin.%d.1.weight' % t] = counter_tensor(seed, 'lpips.lin%d' % t, (1, chans[t + 1], 1, 1), 0.0, 0.1).abs()
    return sd


def synthetic_arcface_state(seed):
    """Seeded IR-SE-50 state dict in model_irse.Backbone(112, 50, 'ir_se')'s keys (id_loss.Backbone), scaled like
    synthetic_encoder_state: conv filters N(0, 0.7/fan_in), BatchNorm statistics near (0, 1), PReLU slopes near 0.25, SE
    filters N(0, 1/fan_in); the Linear 25088->512 N(0, 1/25088) with a small bias."""
    from collections import OrderedDict
    from .id_loss import Backbone
    out = OrderedDict()
    for key, t in Backbone().state_dict().items():
        shape = tuple(t.shape)
        if key.endswith('num_batches_tracked'):
            out[key] = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith('running_var'):
            v = counter_normal(seed, key, int(np.prod(shape))) * 0.2 + 1.0
            out[key] = torch.from_numpy(np.maximum(v, 0.3).astype(np.float32).reshape(shape))
        elif key.endswith('running_mean'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.1)
        elif len(shape) == 4:                                     # conv filters; SE fc1 / fc2 are 1x1 convs
            fan_in = shape[1] * shape[2] * shape[3]
            gain = 1.0 if '.res_layer.5.' in key else 0.7
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(gain / fan_in)))
        elif len(shape) == 2:                                     # output_layer.3: Linear 25088 -> 512
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(1.0 / shape[1])))
        elif key.endswith('.bias'):                               # BatchNorm shift, Linear bias
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.05)
        elif key.endswith('.weight'):                             # 1-D: BatchNorm scale or PReLU slope
            is_prelu = key == 'input_layer.2.weight' or key.endswith('res_layer.2.weight')
            out[key] = counter_tensor(seed, key, shape, 0.25 if is_prelu else 1.0, 0.05 if is_prelu else 0.1)
        else:
            raise KeyError(key)
    return out


def synthetic_deca_encoder_state(seed, outsize=236):
    """Seeded DECA coefficient-encoder state dict in encoders.ResnetEncoder(outsize=236)'s keys (deca.ResnetEncoder): He-scaled
    conv filters N(0, 2/fan_in), BatchNorm statistics near (0, 1), the scale of each bottleneck's last BatchNorm (bn3) and of the
    projection's around 0.5 -- so the residual sums stay O(1) through the 16 bottlenecks --, Linear weights N(0, 1/fan_in) with
    small biases.  103 MB: regenerated from the seed wherever it is needed, never stored."""
    from collections import OrderedDict
    from .deca import ResnetEncoder
    out = OrderedDict()
    for key, t in ResnetEncoder(outsize).state_dict().items():
        shape = tuple(t.shape)
        if key.endswith('num_batches_tracked'):
            out[key] = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith('running_var'):
            v = counter_normal(seed, key, int(np.prod(shape))) * 0.2 + 1.0
            out[key] = torch.from_numpy(np.maximum(v, 0.3).astype(np.float32).reshape(shape))
        elif key.endswith('running_mean'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.1)
        elif len(shape) == 4:
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))))
        elif len(shape) == 2:
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(1.0 / shape[1])))
        elif key.endswith('.bias'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.05)
        elif key.endswith('.weight'):                             # BatchNorm scale
            last = '.bn3.' in key or '.downsample.1.' in key
            out[key] = counter_tensor(seed, key, shape, 0.5 if last else 1.0, 0.05 if last else 0.1)
        else:
            raise KeyError(key)
    return out


def synthetic_deca_detail_encoder_state(seed):
    """Seeded E_detail state dict, encoders.ResnetEncoder(outsize=128)'s keys (deca.ResnetEncoder(128)): synthetic_deca_encoder_state
    with a 128-row last layer.  A key that E_flame has too gets the values it has there at the same seed: pass another seed for an
    encoder that differs from E_flame."""
    return synthetic_deca_encoder_state(seed, outsize=128)


# synthetic_detail_decoder_state: gain of the last conv's filter on N(0, 1/fan_in).  The five BatchNorms with eps = 0.8 each take a
# quarter off the spread, which reaches the last conv at 0.17; 64 puts the value in front of tanh at a spread of about 0.7.
DETAIL_DECODER_LAST_GAIN = 64.0


def synthetic_detail_decoder_state(seed):
    """Seeded D_detail state dict in the keys of decoders.Generator(181, 1, 0.01, 'bilinear') (detail.DetailDecoder): the Linear
    N(0, 1/fan_in), conv filters N(0, 2/fan_in), biases N(0, 0.05^2), BatchNorm scales near 1 and shifts near 0, running means
    N(0, 0.1^2) and running variances around 1 floored at 0.3 -- the five BatchNorm2d(C, 0.8) add their eps = 0.8 to those -- and the
    last conv scaled so that the value in front of tanh has a standard deviation between 0.3 and 1.5 for N(0, 1) latents
    (scripts/make_golden_detail.py asserts it): tanh is then neither flat nor linear.  8 MB: regenerated from the seed, never stored."""
    from collections import OrderedDict
    from .detail import DetailDecoder
    out = OrderedDict()
    for key, t in DetailDecoder().state_dict().items():
        shape = tuple(t.shape)
        if key.endswith('num_batches_tracked'):
            out[key] = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith('running_var'):
            v = counter_normal(seed, key, int(np.prod(shape))) * 0.2 + 1.0
            out[key] = torch.from_numpy(np.maximum(v, 0.3).astype(np.float32).reshape(shape))
        elif key.endswith('running_mean'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.1)
        elif len(shape) == 4:
            last = key == 'conv_blocks.21.weight'
            gain = DETAIL_DECODER_LAST_GAIN if last else 2.0
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(gain / (shape[1] * shape[2] * shape[3]))))
        elif len(shape) == 2:
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(1.0 / shape[1])))
        elif key.endswith('.bias'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.05)
        elif key.endswith('.weight'):                             # BatchNorm scale
            out[key] = counter_tensor(seed, key, shape, 1.0, 0.1)
        else:
            raise KeyError(key)
    return out


def synthetic_fan_state(seed):
    """Seeded 2D-FAN-4 state dict in the 1129 keys of fan_model/models.py FAN(4) (landmarks.FAN) that keeps activations in range
    through the ~100 residual blocks: conv filters behind a ReLU N(0, 2/fan_in), the 1x1 convs behind a sum (conv_last, l, al) and
    bl N(0, 1/fan_in) with bl and al quartered, BatchNorm statistics near (0, 1); the scale of every ConvBlock's first BatchNorm around
    0.2 -- each block then adds a few per cent to the variance its residual carries instead of doubling it -- and of bn_end around 0.3,
    which takes back the growth of an hourglass (up1 + up2 at four levels).  Plain He initialisation puts the last heatmaps at 2e7.
    95 MB: regenerated from the seed wherever it is needed, never stored."""
    from collections import OrderedDict
    from .landmarks import FAN
    out = OrderedDict()
    for key, t in FAN(4).state_dict().items():
        shape = tuple(t.shape)
        name = key.split('.')[0]
        if key.endswith('num_batches_tracked'):
            out[key] = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith('running_var'):
            v = counter_normal(seed, key, int(np.prod(shape))) * 0.2 + 1.0
            out[key] = torch.from_numpy(np.maximum(v, 0.3).astype(np.float32).reshape(shape))
        elif key.endswith('running_mean'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.1)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            if name.startswith(('conv_last', 'l', 'bl', 'al')):
                std = np.sqrt(1.0 / fan_in) * (0.25 if name.startswith(('bl', 'al')) else 1.0)
            else:
                std = np.sqrt(2.0 / fan_in)
            out[key] = counter_tensor(seed, key, shape, 0.0, float(std))
        elif key.endswith('.bias'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.05)
        elif key.endswith('.weight'):                             # BatchNorm scale
            if key.endswith('.bn1.weight'):                       # a ConvBlock's first (the stem's key is 'bn1.weight')
                out[key] = counter_tensor(seed, key, shape, 0.2, 0.02)
            elif name.startswith('bn_end'):
                out[key] = counter_tensor(seed, key, shape, 0.3, 0.03)
            else:
                out[key] = counter_tensor(seed, key, shape, 1.0, 0.1)
        else:
            raise KeyError(key)
    return out


FAN_DEPTH_FC = (10.0, 30.0, 10.0)      # synthetic_fan_depth_state: fc filter gain on N(0, 1/fan_in), fc bias mean and spread


def synthetic_fan_depth_state(seed):
    """Seeded ResNetDepth state dict in the 932 keys of fan_model/models.py ResNetDepth (landmarks.ResNetDepth) that keeps
    activations in range through the 50 bottlenecks: conv filters N(0, 2/fan_in), BatchNorm statistics near (0, 1) and scales near 1,
    but the scale of every bottleneck's last BatchNorm (bn3) around 0.2, so that a block adds a few per cent to the variance its
    shortcut carries instead of doubling it (plain He initialisation puts the depths at 2e8); the linear layer is scaled so that
    the 68 depths come out of order 1 to 100.  234 MB: regenerated from the seed wherever it is needed, never stored."""
    from collections import OrderedDict
    from .landmarks import ResNetDepth
    gain, bias_mean, bias_std = FAN_DEPTH_FC
    out = OrderedDict()
    for key, t in ResNetDepth().state_dict().items():
        shape = tuple(t.shape)
        if key.endswith('num_batches_tracked'):
            out[key] = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith('running_var'):
            v = counter_normal(seed, key, int(np.prod(shape))) * 0.2 + 1.0
            out[key] = torch.from_numpy(np.maximum(v, 0.3).astype(np.float32).reshape(shape))
        elif key.endswith('running_mean'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.1)
        elif len(shape) == 4:
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))))
        elif key == 'fc.weight':
            out[key] = counter_tensor(seed, key, shape, 0.0, float(gain * np.sqrt(1.0 / shape[1])))
        elif key == 'fc.bias':
            out[key] = counter_tensor(seed, key, shape, bias_mean, bias_std)
        elif key.endswith('.bias'):
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.05)
        elif key.endswith('.weight'):                             # BatchNorm scale
            out[key] = counter_tensor(seed, key, shape, 0.2, 0.02) if key.endswith('.bn3.weight') else counter_tensor(seed, key, shape, 1.0, 0.1)
        else:
            raise KeyError(key)
    return out


# synthetic_s3fd_state: per level (conf filter gain, loc filter gain, face-logit bias); gains multiply N(0, 1/fan_in).  The figures
# are tuned at seed 20261018 (scripts/make_golden_s3fd.py): behind the L2Norm most of a logit is a constant over the map (the taps
# are positive), so the conf gains of levels 0-2 are large to give the part that varies a spread of 4-5, and the biases centre it.
S3FD_EXTRA_GAIN = {'fc6': 0.02}                       # the trunk hands fc6 values of O(100): fc6 brings them to O(1) for levels 3-5
S3FD_HEADS = {'conv3_3_norm': (16.0, 0.9, -7.5), 'conv4_3_norm': (32.0, 0.9, -1.5), 'conv5_3_norm': (13.0, 0.9, -5.5),
              'fc7': (2.0, 0.45, -6.0), 'conv6_2': (3.0, 0.45, -5.4), 'conv7_2': (3.0, 0.45, -1.0)}


def synthetic_s3fd_state(seed):
    """Seeded S3FD state dict in the 65 keys of sfd/net_s3fd.py s3fd (face_detector.S3FD) whose detections are usable as a fixture.
    Trunk filters are He-scaled N(0, 2/fan_in) with small biases; a plain He state throughout saturates levels 4-5 at score 1.0 and
    puts |loc| of levels 3-5 at 50-350 (exp(0.2 loc) overflows), because only levels 0-2 are normalised.  So fc6 is scaled down to
    hand O(1) values to the un-normalised levels, the L2Norm weights stay at their constructor scales (10 / 8 / 5) with a few per
    cent of jitter, loc filters are scaled for |loc| of O(1), and conf filters are scaled up with a negative face-logit bias per
    level: the score distribution gets a heavy tail, so that most positions fall below 0.05, a few lie between 0.05 and 0.5 and a
    few above 0.5 on every level.  90 MB: regenerated from the seed wherever it is needed, never stored."""
    from collections import OrderedDict
    from .face_detector import S3FD
    out = OrderedDict()
    for key, t in S3FD().state_dict().items():
        shape = tuple(t.shape)
        name = key.rsplit('.', 1)[0]
        head = name.rsplit('_mbox_', 1)[0] if '_mbox_' in name else None
        if len(shape) == 4 and head is None:
            fan_in = shape[1] * shape[2] * shape[3]
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(2.0 / fan_in) * S3FD_EXTRA_GAIN.get(name, 1.0)))
        elif len(shape) == 4:
            conf_gain, loc_gain, _ = S3FD_HEADS[head]
            fan_in = shape[1] * shape[2] * shape[3]
            out[key] = counter_tensor(seed, key, shape, 0.0, float(np.sqrt(1.0 / fan_in) * (conf_gain if name.endswith('conf') else loc_gain)))
        elif name.endswith('_norm'):
            scale = {'conv3_3_norm': 10.0, 'conv4_3_norm': 8.0, 'conv5_3_norm': 5.0}[name]
            out[key] = counter_tensor(seed, key, shape, scale, 0.03 * scale)
        elif head is not None and name.endswith('conf'):
            b = counter_tensor(seed, key, shape, 0.0, 0.05)
            b[-1] += S3FD_HEADS[head][2]
            out[key] = b
        else:
            out[key] = counter_tensor(seed, key, shape, 0.0, 0.05)
    return out


def _counter_index(seed, key, shape, n):
    """Integers in 0..n-1 from the counter generator."""
    count = int(np.prod(shape))
    v = (np.abs(counter_normal(seed, key, count)) * 1e7).astype(np.int64) % n
    return torch.from_numpy(v.reshape(tuple(shape)))


def _counter_simplex(seed, key, shape, floor=0.0):
    """Non-negative rows that sum to 1 along the last axis."""
    v = np.abs(counter_normal(seed, key, int(np.prod(shape)))).reshape(tuple(shape)) + floor
    return torch.from_numpy((v / v.sum(-1, keepdims=True)).astype(np.float32))


def synthetic_flame_state(seed):
    """Seeded FLAME state dict of DECA's sizes in the keys of models/FLAME.py (flame.FLAME): template N(0, 0.08), blend-shape and
    pose-corrective bases N(0, 0.002), non-negative joint-regressor and skinning rows that sum to 1, valid face indices and
    barycentric triples that sum to 1.  24 MB: regenerated from the seed wherever it is needed, never stored."""
    from collections import OrderedDict
    from . import flame as FL
    V, Fc = FL.V, FL.FACES
    sd = OrderedDict()
    sd['faces_tensor'] = _counter_index(seed, 'flame.f', (Fc, 3), V)
    sd['v_template'] = counter_tensor(seed, 'flame.v_template', (V, 3), 0.0, 0.08)
    sd['shapedirs'] = counter_tensor(seed, 'flame.shapedirs', (V, 3, FL.N_SHAPE + FL.N_EXP), 0.0, 0.002)
    sd['posedirs'] = counter_tensor(seed, 'flame.posedirs', (FL.N_POSE_FEATURE, 3 * V), 0.0, 0.002)
    sd['J_regressor'] = _counter_simplex(seed, 'flame.J_regressor', (FL.JOINTS, V))
    sd['parents'] = torch.tensor(FL.PARENTS, dtype=torch.long)
    sd['lbs_weights'] = _counter_simplex(seed, 'flame.weights', (V, FL.JOINTS))
    sd['eye_pose'] = torch.zeros(1, 6)
    sd['neck_pose'] = torch.zeros(1, 3)
    sd['lmk_faces_idx'] = _counter_index(seed, 'flame.lmk', (FL.STATIC_LMK,), Fc)
    sd['lmk_bary_coords'] = _counter_simplex(seed, 'flame.lmk_b', (FL.STATIC_LMK, 3), 0.1)
    sd['dynamic_lmk_faces_idx'] = _counter_index(seed, 'flame.dyn', (FL.DYN_ROWS, FL.DYN_LMK), Fc)
    sd['dynamic_lmk_bary_coords'] = _counter_simplex(seed, 'flame.dyn_b', (FL.DYN_ROWS, FL.DYN_LMK, 3), 0.1)
    sd['full_lmk_faces_idx'] = _counter_index(seed, 'flame.full', (1, FL.LANDMARKS), Fc)
    sd['full_lmk_bary_coords'] = _counter_simplex(seed, 'flame.full_b', (1, FL.LANDMARKS, 3), 0.1)
    sd['neck_kin_chain'] = torch.tensor([1, 0], dtype=torch.long)
    return sd


def write_flame_files(state, directory):
    """Writes a FLAME state as the two files the reference's constructor reads -> (generic_model.pkl, landmark_embedding.npy):
    shapedirs spread to the 300 / 350 column split of the full model, posedirs as [V,3,36], the dynamic tables as torch tensors."""
    import os
    import pickle
    V = state['v_template'].shape[0]
    sd = state['shapedirs'].numpy()
    full = np.zeros((V, 3, 400), dtype=np.float32)
    full[:, :, :100] = sd[:, :, :100]
    full[:, :, 300:350] = sd[:, :, 100:]
    kin = np.zeros((2, 5), dtype=np.int64)
    kin[0] = [4294967295, 0, 1, 1, 1]
    kin[1] = np.arange(5)
    model = {'f': state['faces_tensor'].numpy(), 'v_template': state['v_template'].numpy(), 'shapedirs': full,
             'posedirs': np.ascontiguousarray(state['posedirs'].numpy().T).reshape(V, 3, -1),
             'J_regressor': state['J_regressor'].numpy(), 'kintree_table': kin, 'weights': state['lbs_weights'].numpy()}
    emb = {'static_lmk_faces_idx': state['lmk_faces_idx'].numpy(), 'static_lmk_bary_coords': state['lmk_bary_coords'].numpy(),
           'dynamic_lmk_faces_idx': state['dynamic_lmk_faces_idx'].clone(), 'dynamic_lmk_bary_coords': state['dynamic_lmk_bary_coords'].clone(),
           'full_lmk_faces_idx': state['full_lmk_faces_idx'].numpy(), 'full_lmk_bary_coords': state['full_lmk_bary_coords'].numpy()}
    pkl, npy = os.path.join(directory, 'generic_model.pkl'), os.path.join(directory, 'landmark_embedding.npy')
    with open(pkl, 'wb') as f:
        pickle.dump(model, f, protocol=2)
    np.save(npy, np.array(emb, dtype=object), allow_pickle=True)
    return pkl, npy


def synthetic_flame_coeffs(seed, key, rows, yaw=None):
    """3DMM coefficient sets shaped like DECA's codedict: shape N(0, 0.8), exp N(0, 0.6), pose N(0, 0.15) with the head's y
    rotation (column 1) replaced by `yaw` (radians, one per row) when given, cam near (8, 0, 0)."""
    pose = counter_tensor(seed, key + '.pose', (rows, 6), 0.0, 0.15)
    if yaw is not None:
        pose[:, 1] = torch.as_tensor(yaw, dtype=torch.float32)
    cam = counter_tensor(seed, key + '.cam', (rows, 3), 0.0, 0.05)
    cam[:, 0] += 8.0
    return {'shape': counter_tensor(seed, key + '.shape', (rows, 100), 0.0, 0.8), 'exp': counter_tensor(seed, key + '.exp', (rows, 50), 0.0, 0.6),
            'pose': pose, 'cam': cam}

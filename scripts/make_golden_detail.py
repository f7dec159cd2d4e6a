"""Writes tests/golden/kat22_deca_detail.npz from the reference's own detail networks: decalib/models/decoders.py Generator (D_detail)
and decalib/models/encoders.py ResnetEncoder(outsize=128) (E_detail) on the seeded synthetic states.

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_detail.py            (CPU only, a few minutes)
    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_detail.py --check    recompute and compare with the committed file

torchvision is stubbed as in make_golden_deca.py (models/resnet.py only copies matching keys from an empty state dict); cv2, skimage
and scipy are stubbed where decalib/utils/util.py imports them and they are not installed (generate_triangles uses none of them).

D_detail, for B = 1 ('b1') and B = 3 ('b3') latents N(0, 1) regenerated from keys: forward hooks on the reference module give the
seven stage outputs -- the first BatchNorm's output [B,128,8,8], the five LeakyReLU outputs, uv_z -- in fp64 and in fp32.  Per stage
s = 0..6 the file holds a strided sample sub_s (channels ::SUB[s][0], rows and columns ::SUB[s][1]), the border rows 0 and H-1 and
border columns 0 and W-1 in full length for the channels ::BORDER[s] (border_s [B,C',4,H]: top, bottom, left, right), the fp64 sum
of every [H,W] plane (sums_s [B,C]) and dev_s, the reference's own max |fp32 - fp64| over the whole stage.  Samples and borders are
the fp64 values rounded to float32 (half an ulp, 3e-8 relative: a tenth of the smallest dev_s relative to its stage's values); sums
and deviations are float64.
E_detail: the 128 detail codes of kat12's two cases (their images, boxes and crop, as make_golden_deca.py builds them), fp64, with
dev_codes.
The script asserts that the value in front of tanh has a standard deviation in [0.3, 1.5], that the state-dict key -> shape lists of
both reference modules equal those of this package's modules, and that util.generate_triangles(S, S) equals
tests/detail_restatement.py's for S = 16, 40 and 256.  The file stays below kat12_deca_encoder.npz in size.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
import deca_restatement as R                                                      # noqa: E402
import detail_restatement as RD                                                   # noqa: E402
from make_golden_deca import _stub_torchvision, to_255                            # noqa: E402

SEED = 20261201
KAT12_SEED = 20261101
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat22_deca_detail.npz')
LIMIT = os.path.join(ROOT, 'tests', 'golden', 'kat12_deca_encoder.npz')
STAGES = 7
SUB = ((4, 1), (8, 2), (8, 4), (8, 8), (8, 16), (4, 16), (1, 8))       # per stage: channel step, spatial step of the sample
BORDER = (16, 16, 8, 8, 8, 4, 1)                                       # per stage: channel step of the border rows and columns
BATCHES = (('b1', 1), ('b3', 3))


def latent(tag, rows):
    return S.counter_tensor(SEED, 'kat22.latent.' + tag, (rows, 181), 0.0, 1.0)


def sample(x, s):
    cs, ss = SUB[s]
    return x[:, ::cs, ::ss, ::ss]


def border(x, s):
    x = x[:, ::BORDER[s]]
    return torch.stack([x[:, :, 0, :], x[:, :, -1, :], x[:, :, :, 0], x[:, :, :, -1]], 2)


def _stub_missing(names):
    for name in names:
        try:
            __import__(name)
        except ImportError:
            parts = name.split('.')
            for i in range(len(parts)):
                key = '.'.join(parts[:i + 1])
                if key not in sys.modules:
                    sys.modules[key] = types.ModuleType(key)
                if i:
                    setattr(sys.modules['.'.join(parts[:i])], parts[i], sys.modules[key])
    for mod, attr in (('scipy.ndimage', 'morphology'), ('skimage.io', 'imsave')):
        if mod in sys.modules and not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, None)


def stages(G, z):
    """The seven stage outputs of one forward of the reference module (clones: its LeakyReLUs work in place)."""
    got, hooks = [], []
    for i in (0, 4, 8, 12, 16, 20):
        hooks.append(G.conv_blocks[i].register_forward_hook(lambda m, a, o: got.append(o.detach().clone())))
    pre = []
    hooks.append(G.conv_blocks[22].register_forward_hook(lambda m, a, o: pre.append(a[0].detach().clone())))
    with torch.no_grad():
        got.append(G(z))
    for h in hooks:
        h.remove()
    return got, pre[0]


def keys_of(module):
    return ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in module.state_dict().items()]


def compute():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    sys.path.insert(0, ref)
    _stub_torchvision()
    _stub_missing(('scipy.ndimage', 'skimage.io', 'cv2'))
    from libs.DECA.decalib.models.decoders import Generator
    from libs.DECA.decalib.models.encoders import ResnetEncoder
    from libs.DECA.decalib.utils import util
    from stylegan_directions_face_reenactment_amd import deca as D, detail as DT

    for n in (16, 40, 256):
        assert np.array_equal(util.generate_triangles(n, n), RD.generate_triangles(n, n)), n
        assert np.array_equal(util.generate_triangles(n, n), DT.dense_triangles(n, n)), n

    out = {'seed': np.int64(SEED), 'kat12_seed': np.int64(KAT12_SEED)}
    sd = S.synthetic_detail_decoder_state(SEED)
    G = Generator(latent_dim=181, out_channels=1, out_scale=0.01, sample_mode='bilinear')
    G.load_state_dict(sd, strict=True)
    G.eval()
    out['keys_decoder'] = np.array(keys_of(G))
    assert keys_of(G) == keys_of(DT.DetailDecoder()), 'D_detail keys differ from detail.DetailDecoder'
    for tag, rows in BATCHES:
        z = latent(tag, rows)
        s32, _ = stages(G.float(), z)
        s64, pre = stages(G.double(), z.double())
        std = float(pre.std())
        assert 0.3 <= std <= 1.5, 'the value in front of tanh has a standard deviation of %.3f' % std
        out['pre_tanh_std_' + tag] = np.asarray(std)
        for s in range(STAGES):
            a, b = s64[s], s32[s].double()
            out['sub_%d_%s' % (s, tag)] = sample(a, s).float().numpy()
            out['border_%d_%s' % (s, tag)] = border(a, s).float().numpy()
            out['sums_%d_%s' % (s, tag)] = a.sum((2, 3)).numpy()
            out['dev_%d_%s' % (s, tag)] = np.asarray(float((a - b).abs().max()))
            out['max_%d_%s' % (s, tag)] = np.asarray(float(a.abs().max()))

    se = S.synthetic_deca_detail_encoder_state(SEED)
    E = ResnetEncoder(outsize=128)
    E.load_state_dict(se, strict=True)
    E.eval()
    out['keys_encoder'] = np.array(keys_of(E))
    assert keys_of(E) == keys_of(D.ResnetEncoder(128)), 'E_detail keys differ from deca.ResnetEncoder(128)'
    for name in R.CASES:
        x, boxes, _ = R.fixture_inputs(S, KAT12_SEED, name)
        codes = {}
        for dtype in (torch.float32, torch.float64):
            model = E.to(dtype)
            img = to_255(x.to(dtype))
            rows = []
            with torch.no_grad():
                for b in range(x.shape[0]):
                    theta = torch.tensor(R.box_transform(boxes[b].tolist()), dtype=dtype)[None, :2]
                    rows.append(model(R.warp_affine_composed(img[b:b + 1], theta) / 255.0))
            codes[dtype] = torch.cat(rows).double()
        assert float(codes[torch.float64].abs().max()) > 0.1
        out['codes_' + name] = codes[torch.float64].numpy()
        out['dev_codes_' + name] = np.asarray(float((codes[torch.float32] - codes[torch.float64]).abs().max()))
    return out


def check(out):
    old = np.load(OUT, allow_pickle=False)
    assert sorted(old.files) == sorted(out), (sorted(set(old.files) ^ set(out)))
    worst = 0.0
    for k, v in out.items():
        a, b = np.asarray(old[k]), np.asarray(v)
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind in 'US' or a.dtype.kind == 'i':
            assert np.array_equal(a, b), k
        elif k.startswith('dev_'):
            assert b / 4 <= a <= b * 4, (k, float(a), float(b))            # a deviation is reproduced in size, not in digits
        else:
            err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-30))
            worst = max(worst, err)
            assert err <= 1e-6, (k, err)
    print('check: %s reproduced, largest relative difference %.2e' % (OUT, worst))


def main():
    out = compute()
    if '--check' in sys.argv[1:]:
        return check(out)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote', OUT, size, 'bytes', {k: (v.shape if v.ndim else v.item()) for k, v in out.items() if not k.startswith('keys')})
    assert size <= os.path.getsize(LIMIT), 'the fixture of %d bytes is larger than kat12_deca_encoder.npz' % size


if __name__ == '__main__':
    main()

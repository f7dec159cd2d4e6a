"""Writes tests/golden/kat23_deca_texture.npz from the reference's own FLAMETex.forward (decalib/models/FLAME.py:216-262).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_texture.py            (CPU only, about a minute, 2 GB)
    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_texture.py --check    recompute and compare with the committed file

models/FLAME.py imports without pytorch3d.  The module is made without its texture file: FLAMETex.__new__, nn.Module.__init__, and the
seeded synthetic texture_mean [1,1,512*512*3] and texture_basis [1,512*512*3,50] of tests/texture_restatement.synthetic_space
registered as its two buffers, at the real sizes.  Its forward runs in fp64 and in fp32 on codes N(0, 1) regenerated from keys, for
B = 1 ('b1') and B = 3 ('b3').  Per batch the file holds the strided sample sub (every 8th row and column of the [B,3,256,256]
albedo), the border rows 0 and 255 and border columns 0 and 255 in full length (border [B,3,4,256]: top, bottom, left, right), the
fp64 sum of every plane (sums [B,3]) and dev, the reference's own max |fp32 - fp64|.  Samples and borders are the fp64 values rounded
to float32; sums and deviations are float64.  The script asserts that tests/texture_restatement.py's two restatements reproduce the
reference's fp64 result to 1e-12, and that the buffer names and shapes equal those of texture.FlameTex.

utils/renderer.py cannot be imported (pytorch3d is absent), so the render side and the UV pass are held to the restatements of
tests/texture_restatement.py, as the shape and the detail render are.  The file holds data only and stays below
kat22_deca_detail.npz in size.
"""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
import texture_restatement as RT                                                  # noqa: E402

SEED = RT.KAT_SEED
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat23_deca_texture.npz')
LIMIT = os.path.join(ROOT, 'tests', 'golden', 'kat22_deca_detail.npz')
SOURCE, UV, N_TEX = 512, 256, 50


def code(tag, rows):
    return S.counter_tensor(SEED, 'kat23.tex.' + tag, (rows, N_TEX), 0.0, 1.0)


def compute():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    sys.path.insert(0, ref)
    from libs.DECA.decalib.models.FLAME import FLAMETex
    from stylegan_directions_face_reenactment_amd.texture import FlameTex

    mean, basis = RT.synthetic_space(S, SEED, SOURCE, N_TEX)
    T = FLAMETex.__new__(FLAMETex)
    nn.Module.__init__(T)
    T.register_buffer('texture_mean', mean)
    T.register_buffer('texture_basis', basis)
    ours = FlameTex(N_TEX, SOURCE, UV)
    assert [(k, tuple(v.shape)) for k, v in T.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ours.state_dict().items()]
    out = {'seed': np.int64(SEED), 'source': np.int64(SOURCE), 'uv': np.int64(UV), 'n_tex': np.int64(N_TEX)}
    for tag, rows in RT.KAT_BATCHES:
        c = code(tag, rows)
        with torch.no_grad():
            a32 = T.float()(c).double()
            a64 = T.double()(c.double())
        assert tuple(a64.shape) == (rows, 3, UV, UV)
        for name, fn in (('flametex', RT.flametex), ('flametex_kept', RT.flametex_kept)):
            err = float((fn(mean, basis, c, SOURCE, UV) - a64).abs().max())
            assert err <= 1e-12, (name, err)
        sub, brd, sums = RT.digest(a64)
        out['sub_' + tag], out['border_' + tag], out['sums_' + tag] = sub.float().numpy(), brd.float().numpy(), sums.numpy()
        out['dev_' + tag] = np.asarray(float((a32 - a64).abs().max()))
        out['max_' + tag] = np.asarray(float(a64.abs().max()))
    return out


def check(out):
    old = np.load(OUT, allow_pickle=False)
    assert sorted(old.files) == sorted(out), (sorted(set(old.files) ^ set(out)))
    worst = 0.0
    for k, v in out.items():
        a, b = np.asarray(old[k]), np.asarray(v)
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind == 'i':
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
    print('wrote', OUT, size, 'bytes', {k: (v.shape if v.ndim else v.item()) for k, v in out.items()})
    assert size <= os.path.getsize(LIMIT), 'the fixture of %d bytes is larger than kat22_deca_detail.npz' % size


if __name__ == '__main__':
    main()

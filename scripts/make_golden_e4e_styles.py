"""Writes tests/golden/kat24_e4e_styles.npz from the reference's own e4e encoder with more heads than its input side gives
(libs/gan/encoder4editing/psp_encoders.py Encoder4Editing(50, 'ir_se', image_resolution): style_count follows image_resolution,
:143-156; the input is whatever it is handed, :171-199).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_e4e_styles.py        (CPU only, a few minutes: case f runs 256 x 256 in fp64)

The module is imported through the shims of oracle/make_golden.py, loads the seeded state of synthetic.synthetic_encoder_state with
strict=True and runs on the CPU in fp32 and, as .double(), in fp64; the taps are those of scripts/make_golden_e4e_taps.py, collected
by its hooks.

Cases (tests/e4e_styles_cases.py CASES): d = B 2, input 32, image_resolution 1024 (18 heads); e = B 3, input 80, image_resolution
512 (16 heads); f = B 1, input 256, image_resolution 1024 (18 heads, the 1024 generator's encoder on the alignment crop).  The file
holds, per case, w_<case> (the fp64 W+ codes), max_w_<case> and per tap dev_<tap>_<case> = the reference's own max |fp32 - fp64| on
that tensor.  Weights and images are regenerated from the seeds, not stored.  The script asserts that the restatement
(tests/e4e_restatement.py forward, which counts the heads from the state's keys) equals the reference in fp64 on every tap.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.dont_write_bytecode = True

from oracle import make_golden as MG                                              # noqa: E402
from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
import e4e_restatement as R                                                       # noqa: E402
import e4e_styles_cases as C                                                      # noqa: E402
from make_golden_e4e_taps import run_reference                                    # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', C.KAT)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(16)
    MG.import_reference()
    from libs.gan.encoder4editing.psp_encoders import Encoder4Editing
    out = {'seed': np.int64(R.SEED)}
    for name, (B, side, res, seed, key) in C.CASES.items():
        enc = Encoder4Editing(50, 'ir_se', res).eval()
        assert len(enc.styles) == C.heads(name), (name, len(enc.styles))
        sd = C.fixture_state(S, name, enc.state_dict())
        enc.load_state_dict(sd, strict=True)
        x = C.fixture_inputs(S, name)
        t32 = run_reference(enc, x)
        t64 = run_reference(enc.double(), x.double())
        with torch.no_grad():
            mine = R.forward(sd, x.double())
        for k in R.TAPS:                                       # the restatement equals the reference
            d = float((mine[k] - t64[k]).abs().max())
            assert d <= 1e-10 * max(1.0, float(t64[k].abs().max())), (name, k, d)
        for k in R.TAPS:
            dev = float((t32[k].double() - t64[k]).abs().max())
            assert dev > 0, (name, k)
            out['dev_%s_%s' % (k, name)] = np.asarray(dev)
            print('case %s tap %-8s %-18s max |.| %.3f   max |fp32 - fp64| %.3e' % (name, k, tuple(t64[k].shape),
                                                                                  float(t64[k].abs().max()), dev))
        assert tuple(t64['w'].shape) == (B, C.heads(name), 512), (name, t64['w'].shape)
        out['max_w_' + name] = np.asarray(float(t64['w'].abs().max()))
        out['w_' + name] = t64['w'].numpy()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()

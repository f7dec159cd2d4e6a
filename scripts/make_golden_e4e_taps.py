"""Writes tests/golden/kat15_e4e_taps.npz from the reference's own e4e encoder (libs/gan/encoder4editing/psp_encoders.py
Encoder4Editing(50, 'ir_se', R)).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_e4e_taps.py        (CPU only, a few minutes: case c runs 256 x 256 in fp64)

The module is imported through the shims of oracle/make_golden.py, loads the seeded state of synthetic.synthetic_encoder_state with
strict=True and runs on the CPU in fp32 and, as .double(), in fp64.  The taps are collected with forward hooks: the stem, the
outputs of units 0, 3, 6 (c1), 20 (c2) and 23 (c3), the inputs of the first middle and the first fine style head (p2, p1) and the
input of every head's EqualLinear (h_coarse, h_middle, h_fine).

Cases (tests/e4e_restatement.py CASES): a = B 3, R 64 with the inputs and seed of kat6's w64 (asserted equal to it); b = B 2, R 96 with
new inputs; c = B 2, R 256 with kat6's w256 inputs (asserted equal to it).  The file holds, per case and tap, dev_<tap>_<case> = the
reference's own max |fp32 - fp64| on that tensor, max_w_<case>, and for a and b the fp64 W+ codes (w_<case>); case c stores
dev_w_c only, its codes are kat6's w256.  Weights and images are regenerated from the seeds, not stored.  The script asserts that the
restatement (tests/e4e_restatement.py) equals the reference in fp64 on every tap.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True

from oracle import make_golden as MG                                              # noqa: E402
from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
import e4e_restatement as R                                                       # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', R.KAT)
KAT6 = {'a': 'w64', 'c': 'w256'}


def run_reference(enc, x):
    """W+ and the taps of the reference module, by hooks."""
    taps, hooks, vec = {}, [], {}
    hooks.append(enc.input_layer.register_forward_hook(lambda m, a, o: taps.__setitem__('stem', o.detach())))
    body = list(enc.body)
    for i, name in R.TAP_UNITS.items():
        hooks.append(body[i].register_forward_hook(lambda m, a, o, name=name: taps.__setitem__(name, o.detach())))
    hooks.append(enc.styles[R.COARSE].register_forward_hook(lambda m, a, o: taps.__setitem__('p2', a[0].detach())))
    hooks.append(enc.styles[R.MIDDLE].register_forward_hook(lambda m, a, o: taps.__setitem__('p1', a[0].detach())))
    for j, head in enumerate(enc.styles):
        hooks.append(head.linear.register_forward_hook(lambda m, a, o, j=j: vec.__setitem__(j, a[0].detach())))
    with torch.no_grad():
        w = enc(x)
    for h in hooks:
        h.remove()
    n = len(enc.styles)
    taps['h_coarse'] = torch.stack([vec[j] for j in range(R.COARSE)], 1)
    taps['h_middle'] = torch.stack([vec[j] for j in range(R.COARSE, R.MIDDLE)], 1)
    taps['h_fine'] = torch.stack([vec[j] for j in range(R.MIDDLE, n)], 1)
    taps['w'] = w.detach()
    return taps


def main():
    torch.manual_seed(0)
    torch.set_num_threads(16)
    MG.import_reference()
    from libs.gan.encoder4editing.psp_encoders import Encoder4Editing
    kat6 = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat6_e4e.npz'), allow_pickle=False)
    out = {'seed': np.int64(R.SEED)}
    for name, (B, res, seed, key) in R.CASES.items():
        enc = Encoder4Editing(50, 'ir_se', res).eval()
        sd = R.fixture_state(S, name, enc.state_dict())
        enc.load_state_dict(sd, strict=True)
        x = R.fixture_inputs(S, name)
        t32 = run_reference(enc, x)
        t64 = run_reference(enc.double(), x.double())
        if name in KAT6:                                       # the fp32 codes are the ones kat6 holds
            assert np.array_equal(t32['w'].numpy(), kat6[KAT6[name]]), name
        if res <= 96:                                          # the restatement equals the reference
            with torch.no_grad():
                mine = R.forward(sd, x.double())
            for k in R.TAPS:
                d = float((mine[k] - t64[k]).abs().max())
                assert d <= 1e-10 * max(1.0, float(t64[k].abs().max())), (name, k, d)
        for k in R.TAPS:
            dev = float((t32[k].double() - t64[k]).abs().max())
            assert dev > 0, (name, k)
            out['dev_%s_%s' % (k, name)] = np.asarray(dev)
            if name != 'c' or k == 'w':
                print('case %s tap %-8s %-18s max |.| %.3f   max |fp32 - fp64| %.3e' % (name, k, tuple(t64[k].shape),
                                                                                      float(t64[k].abs().max()), dev))
        out['max_w_' + name] = np.asarray(float(t64['w'].abs().max()))
        if name == 'c':
            for k in R.TAPS:
                if k != 'w':
                    del out['dev_%s_%s' % (k, name)]           # only dev_w is kept at 256
        else:
            out['w_' + name] = t64['w'].numpy()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()

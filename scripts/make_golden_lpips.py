"""Writes tests/golden/kat9_lpips.npz from the reference's own LPIPS code (libs/criteria/lpips/lpips.py, networks.py, utils.py).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_lpips.py        (CPU only, seconds)

torchvision and the URL download of the `lin` weights are not needed: `torchvision.models.alexnet` is stubbed with a module of
the torchvision `features` layout (the only part networks.py reads) and `lpips.get_state_dict` with the seeded `lin` weights of
synthetic.synthetic_lpips_state -- the shim pattern SURVEY Appendix E uses for the generator.  The reference's `.to("cuda")` calls
are mapped to the CPU.  The file holds the seed, two small inputs, the reference loss and dL/dx (an fp64 run of the reference
code), nothing else.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
from stylegan_directions_face_reenactment_amd.lpips import _alexnet_features      # noqa: E402

SEED = 20261016
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat9_lpips.npz')
SHAPES = {'a': (2, 3, 64, 64), 'b': (1, 3, 80, 72)}


def import_reference_lpips(sd):
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    sys.path.insert(0, ref)

    class _Alex:
        def __init__(self):
            self.features = _alexnet_features()
            with torch.no_grad():
                for i in (0, 3, 6, 8, 10):
                    self.features[i].weight.copy_(sd['net.layers.%d.weight' % i])
                    self.features[i].bias.copy_(sd['net.layers.%d.bias' % i])

    tv = types.ModuleType('torchvision')
    tv.models = types.ModuleType('torchvision.models')
    tv.models.alexnet = lambda pretrained=False: _Alex()
    tv.transforms = types.ModuleType('torchvision.transforms')
    sys.modules.update({'torchvision': tv, 'torchvision.models': tv.models, 'torchvision.transforms': tv.transforms})
    from libs.criteria.lpips import lpips as L
    L.get_state_dict = lambda net_type='alex', version='0.1': {'%d.1.weight' % t: sd['lin.%d.1.weight' % t] for t in range(5)}
    return L


def main():
    sd = S.synthetic_lpips_state(SEED)
    to = torch.nn.Module.to
    torch.nn.Module.to = lambda self, *a, **k: self if a[:1] == ('cuda',) else to(self, *a, **k)
    try:
        L = import_reference_lpips(sd)
        model = L.LPIPS(net_type='alex', version='0.1')
    finally:
        torch.nn.Module.to = to
    out = {'seed': np.int64(SEED)}
    for name, shape in SHAPES.items():
        x = S.counter_tensor(SEED, 'kat9.x.' + name, shape, 0.0, 0.5).clamp(-1, 1)
        y = S.counter_tensor(SEED, 'kat9.y.' + name, shape, 0.0, 0.5).clamp(-1, 1)
        out['x_' + name], out['y_' + name] = x.numpy(), y.numpy()
        m = model.double()
        xr = x.double().requires_grad_(True)
        loss = m(xr, y.double())
        loss.backward()
        out['loss_' + name] = np.asarray(loss.item(), dtype=np.float64)
        out['dx_' + name] = xr.grad.numpy()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, {k: (v.shape if v.ndim else float(v)) for k, v in out.items()})


if __name__ == '__main__':
    main()

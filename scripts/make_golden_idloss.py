"""Writes tests/golden/kat10_idloss.npz from the reference's own identity loss (libs/criteria/id_loss.py, model_irse.py, helpers.py).

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_idloss.py        (CPU only, about a minute)

The seeded IR-SE-50 state of synthetic.synthetic_arcface_state is saved to a temporary .pth, which the reference's IDLoss loads
itself (id_loss.py:11-15); the loss then runs in fp64 on the CPU.  The file holds the seed, the keys the inputs are regenerated
from (synthetic.counter_tensor), the embeddings, the loss and dL/dx in float32 -- inside the 188x188 crop window only for the
cropped case -- and the reference Backbone's key -> shape list; no input image.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402

SEED = 20261017
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat10_idloss.npz')
CASES = {'crop': ((1, 3, 256, 256), True), 'nocrop': ((2, 3, 120, 112), False)}
WINDOW = (slice(35, 223), slice(32, 220))


def inputs(seed, name, shape):
    """The fixture's images, regenerated from the seed (the npz stores only the keys)."""
    x = S.counter_tensor(seed, 'kat10.x.' + name, shape, 0.0, 0.5).clamp(-1, 1)
    y = S.counter_tensor(seed, 'kat10.y.' + name, shape, 0.0, 0.5).clamp(-1, 1)
    return x, y


def main():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    sys.path.insert(0, ref)
    from libs.criteria import id_loss as L
    sd = S.synthetic_arcface_state(SEED)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'model_ir_se50.pth')
        torch.save(sd, path)
        model = L.IDLoss(pretrained_model_path=path).double()
    model.eval()
    out = {'seed': np.int64(SEED),
           'keys': np.array(['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in model.facenet.state_dict().items()])}
    for name, (shape, crop) in CASES.items():
        x, y = inputs(SEED, name, shape)
        out['x_key_' + name] = np.array('kat10.x.' + name)
        out['y_key_' + name] = np.array('kat10.y.' + name)
        xr = x.double().requires_grad_(True)
        loss = model(xr, y.double(), crop=crop)
        loss.backward()
        lv = loss.item()
        assert 0.05 <= lv <= 1.5, lv                # no bar is measured against a loss near 0
        with torch.no_grad():
            out['ex_' + name] = model.extract_feats(x.double(), crop).float().numpy()
            out['ey_' + name] = model.extract_feats(y.double(), crop).float().numpy()
        g = xr.grad
        if crop:
            outside = g.clone()
            outside[:, :, WINDOW[0], WINDOW[1]] = 0
            assert int(torch.count_nonzero(outside)) == 0
            g = g[:, :, WINDOW[0], WINDOW[1]]
        out['loss_' + name] = np.asarray(lv, dtype=np.float64)
        out['dx_' + name] = g.float().numpy()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes', {k: (v.shape if v.ndim else v.item()) for k, v in out.items() if k != 'keys'})


if __name__ == '__main__':
    main()

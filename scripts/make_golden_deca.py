"""Writes tests/golden/kat12_deca_encoder.npz from the reference's own DECA coefficient encoder (libs/DECA/decalib/models/encoders.py,
models/resnet.py) and its rotation_converter.

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_deca.py        (CPU only, a few minutes)

The reference's ResnetEncoder is imported with a stub `torchvision` in sys.modules whose models.resnet50(pretrained=True)
.state_dict() is empty (models/resnet.py:21,175 only copy matching keys from it), loads the seeded state of
synthetic.synthetic_deca_encoder_state and runs in fp64 on the CPU, one row at a time as extract_DECA_params does.  The crop in
front of it restates TestData.get_image_tensor with tests/deca_restatement.py's similarity fit and its affine_grid + grid_sample
composition (neither skimage nor kornia is needed; the composition is unverified against kornia), after the range map of
image_utils.torch_range_1_to_255.  The file holds the seed, the reference module's key -> shape list, the boxes, and per case the
236 parameters, the angles of every row, the reference's own fp32-vs-fp64 deviation of both (dev_parameters, dev_angles: largest
absolute difference), dL/dx for the seeded dL/dparameters on a 128 x 128 window of row 0 and every row's sum |dL/dx|.  Images are
regenerated from keys, not stored.
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

SEED = 20261101
OUT = os.path.join(ROOT, 'tests', 'golden', 'kat12_deca_encoder.npz')


def _stub_torchvision():
    tv, models = types.ModuleType('torchvision'), types.ModuleType('torchvision.models')

    class _Empty:
        def state_dict(self):
            return {}

    models.resnet50 = models.resnet101 = models.resnet152 = lambda pretrained=False: _Empty()
    tv.models = models
    sys.modules['torchvision'], sys.modules['torchvision.models'] = tv, models


def to_255(image):
    """image_utils.torch_range_1_to_255 (libs/utilities/image_utils.py:87-94), out of place so that autograd can pass."""
    return (image.clamp(min=-1, max=1) + 1) / (1 - (-1) + 1e-5) * 255.0


def run(model, RC, x, boxes, dtype):
    """extract_DECA_params' loop: per row the crop, the encoder, the angles -> (params [B,236], angles [B,3])."""
    params, angles = [], []
    img = to_255(x.to(dtype))
    for b in range(x.shape[0]):
        theta = torch.tensor(R.box_transform(boxes[b].tolist()), dtype=dtype)[None, :2]
        crop = R.warp_affine_composed(img[b:b + 1], theta) / 255.0
        p = model(crop)
        params.append(p)
        angles.append(RC.rad2deg(RC.batch_axis2euler(p[:, 200:203].detach())).to(torch.float64))
    return torch.cat(params), torch.cat(angles)


def main():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    sys.path.insert(0, ref)
    _stub_torchvision()
    from libs.DECA.decalib.models.encoders import ResnetEncoder
    from libs.DECA.decalib.utils import rotation_converter as RC
    sd = S.synthetic_deca_encoder_state(SEED)
    model = ResnetEncoder(outsize=236)
    model.load_state_dict(sd, strict=True)
    model.eval()
    out = {'seed': np.int64(SEED),
           'keys': np.array(['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in model.state_dict().items()])}
    for name in R.CASES:
        x, boxes, g = R.fixture_inputs(S, SEED, name)
        with torch.no_grad():
            p32, a32 = run(model.float(), RC, x, boxes, torch.float32)
        xr = x.double().requires_grad_(True)
        p64, a64 = run(model.double(), RC, xr, boxes, torch.float64)
        (p64 * g.double()).sum().backward()
        dx = xr.grad
        assert float(p64.abs().max()) > 0.5 and float(dx.abs().max()) > 0
        wy, wx = R.window(name)
        out['boxes_' + name] = boxes.numpy()
        out['params_' + name] = p64.detach().numpy()
        out['angles_' + name] = a64.numpy()
        out['dev_parameters_' + name] = np.asarray(float((p32.double() - p64.detach()).abs().max()))
        out['dev_angles_' + name] = np.asarray(float((a32 - a64).abs().max()))
        out['dx_window_' + name] = dx[0, :, wy, wx].float().numpy()
        out['dx_abs_sum_' + name] = dx.abs().sum((1, 2, 3)).numpy()
        out['dx_max_' + name] = np.asarray(float(dx.abs().max()))
        assert int(torch.count_nonzero(dx[x.abs().expand_as(dx) > 1])) == 0      # the clamp's mask
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes', {k: (v.shape if v.ndim else v.item()) for k, v in out.items() if k != 'keys'})


if __name__ == '__main__':
    main()

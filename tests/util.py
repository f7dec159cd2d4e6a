"""Shared helpers for the test-suite (oracle access is allowed here: tests are the checker)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import sg2_oracle as O                                     # noqa: E402
from stylegan_directions_face_reenactment_amd import synthetic as S    # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SEED = 20260929   # seed used by oracle/make_golden.py


def golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def t(a):
    return torch.from_numpy(np.asarray(a))


def maxabs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


_STATE_CACHE = {}


def synthetic_state(size, cm, seed=SEED):
    """Synthetic generator state_dict on CPU (cached per process)."""
    key = (size, cm, seed)
    if key not in _STATE_CACHE:
        _STATE_CACHE[key] = S.synthetic_state_dict(O.template_state(size, 512, 8, cm), seed=seed)
    return _STATE_CACHE[key]


def hip_generator(size, cm, seed=SEED):
    from stylegan_directions_face_reenactment_amd.model import Generator
    G = Generator(size, 512, 8, channel_multiplier=cm)
    G.load_state_dict(synthetic_state(size, cm, seed), strict=True)
    return G.eval().cuda()


def composed(x, panels, P, swap_rb, out):
    """The frames of the video entries from the two launches that do not share their kernel: sgdfr_sweep_frames_f32 (pooled, anchored
    on the float64 restatement of tests/test_gpu_sweeps.py) -> sgdfr_grid_to_u8_f32 (the host assembly of tests/dense_refs.py)."""
    from stylegan_directions_face_reenactment_amd.reenact import grid_frames_uint8, pool_images
    return grid_frames_uint8(list(panels) + [pool_images(x, P)], swap_rb=swap_rb, out=out)


def image_digest(img, stride=4):
    d = img.detach().double().cpu()
    return {'sub': img.detach().cpu()[:, :, ::stride, ::stride].numpy(), 'rowsum': d.sum(3).numpy(),
            'colsum': d.sum(2).numpy()}

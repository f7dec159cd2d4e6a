"""Writes tests/golden/kat25_locality.npz from the reference's OWN Space_Regulizer.ball_holder_loss_lazy
(libs/criteria/PTI/localitly_regulizer.py:27-50), on the CPU.

    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_locality.py            (CPU only, under a minute)
    SGDFR_REFERENCE=<reference checkout> python scripts/make_golden_locality.py --check    recompute and compare with the committed file

What the reference method is handed: `Generator(size)`, the oracle's generator (oracle/sg2_oracle.py) behind the three calls the
method makes -- get_latent, mean_latent, forward -- for sizes 32 and 64 and n = 1 and 3 samples (tests/locality_restatement.py CASES,
which also builds the seeded states); global_config.device = 'cpu'; torchvision as a stub module (the method imports its utils and
never uses them); np.random.seed fixed per case; `lpips_net` = locality_restatement.lpips_net (the reference's LPIPS downloads
weights; the HIP LPIPS is pinned by kat9).  The generators have ZERO noise strengths, so whatever noise a forward would draw cannot
matter.  mean_latent returns the case's fixed truncation latent: the first stated deviation (the reference redraws it per call).
space_regulizer_loss cannot be called through calc_loss (base_coach.py:38 passes use_wandb, a TypeError): the method is called directly.

Recorded per case, arrays only, float32 as the reference computes them: z, w_z, pivot, trunc, the morphed codes, r (recomputed with
the reference's own get_morphed_w_code expression on the same w_z), the loss, dLoss/d(new image) of every sample and dLoss/d(the last
styled conv's bias of new_G).  The script then asserts that the fp64 restatement meets all of it at the tests' bars.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import sg2_oracle as O                                                # noqa: E402
from stylegan_directions_face_reenactment_amd import synthetic as S               # noqa: E402
import locality_restatement as R                                                  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'kat25_locality.npz')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


class Generator(torch.nn.Module):
    """The oracle's generator of one size behind the reference module's interface; keeps the images it hands out (with their
    gradients retained) so that dLoss/d(image) can be read after the backward."""

    def __init__(self, size, P, trunc, grad_key=None):
        super().__init__()
        self.size, self.trunc, self.handed = size, trunc, []
        self.P = {k: v.clone() for k, v in P.items()}
        if grad_key is not None:
            self.P[grad_key].requires_grad_(True)

    def get_latent(self, z):
        return O.mapping(self.P, z)

    def mean_latent(self, n):
        return self.trunc

    def forward(self, styles, return_latents=False, truncation=1, truncation_latent=None, input_is_latent=False):
        img, lat = O.generator_forward(self.P, styles, return_latents=return_latents, truncation=truncation,
                                       truncation_latent=truncation_latent, input_is_latent=input_is_latent)
        if img.requires_grad:
            img.retain_grad()
        self.handed.append(img)
        return img, lat


def reference_modules(ref):
    sys.path.insert(0, ref)
    tv = types.ModuleType('torchvision')
    tv.utils = types.ModuleType('torchvision.utils')
    sys.modules.setdefault('torchvision', tv)
    sys.modules.setdefault('torchvision.utils', tv.utils)
    from libs.criteria.PTI import global_config, hyperparameters
    from libs.criteria.PTI.localitly_regulizer import Space_Regulizer
    global_config.device = 'cpu'
    assert (hyperparameters.regulizer_alpha, hyperparameters.regulizer_l2_lambda, hyperparameters.regulizer_lpips_lambda) == \
        (R.ALPHA, R.L2_LAMBDA, R.LPIPS_LAMBDA)
    return Space_Regulizer


def compute():
    ref = os.environ.get('SGDFR_REFERENCE')
    if not ref:
        raise SystemExit('set SGDFR_REFERENCE to the reference checkout')
    Space_Regulizer = reference_modules(ref)
    out = {'seed': np.int64(R.SEED)}
    for idx, (tag, size, n) in enumerate(R.CASES):
        old, new, pivot, trunc = R.case_states(S, size)
        key = R.grad_key(size)
        G_old, G_new = Generator(size, old, trunc), Generator(size, new, trunc, key)
        reg = Space_Regulizer(G_old, R.lpips_net)
        np.random.seed(R.SEED % (2 ** 31) + idx)
        state = np.random.get_state()
        loss = reg.ball_holder_loss_lazy(G_new, n, pivot)
        loss.backward()
        np.random.set_state(state)
        z = torch.from_numpy(np.random.randn(n, 512)).float()                     # the draw of :31-33, repeated
        with torch.no_grad():
            w_z = G_old.get_latent(z)
            codes = torch.cat([reg.get_morphed_w_code(w.unsqueeze(0), pivot) for w in w_z])
            r = torch.stack([torch.norm(w.unsqueeze(0) - pivot, p=2) for w in w_z])
        assert len(G_new.handed) == n and len(G_old.handed) == n
        out.update({'z_' + tag: z.numpy(), 'w_z_' + tag: w_z.numpy(), 'pivot_' + tag: pivot.numpy(), 'trunc_' + tag: trunc.numpy(),
                    'codes_' + tag: codes.numpy(), 'r_' + tag: r.numpy(), 'loss_' + tag: np.asarray(loss.item(), dtype=np.float32),
                    'dimg_' + tag: torch.cat([im.grad for im in G_new.handed]).numpy(), 'dparam_' + tag: G_new.P[key].grad.numpy()})
        assert loss.item() > 1e-4 and float(out['dparam_' + tag].__abs__().max()) > 0
    return out


def check(out):
    old = np.load(OUT, allow_pickle=False)
    assert sorted(old.files) == sorted(out), sorted(set(old.files) ^ set(out))
    worst = 0.0
    for k, v in out.items():
        a, b = np.asarray(old[k]), np.asarray(v)
        assert a.shape == b.shape and a.dtype == b.dtype, k
        err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-30))
        worst = max(worst, err)
        assert err <= 1e-5, (k, err)
    print('check: %s reproduced, largest relative difference %.2e' % (OUT, worst))


def main():
    out = compute()
    R.meets(out, S)
    if '--check' in sys.argv[1:]:
        return check(out)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    limit = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != os.path.basename(OUT))
    print('wrote', OUT, size, 'bytes', {k: (v.shape if v.ndim else v.item()) for k, v in out.items()})
    assert size <= limit, 'the fixture of %d bytes is larger than the largest one already there (%d)' % (size, limit)


if __name__ == '__main__':
    main()

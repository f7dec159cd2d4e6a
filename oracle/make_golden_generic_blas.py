"""ORACLE tooling -- KAT-4's cm=1 latents from the REAL reference on MKL's generic x86 code path (tests/golden/kat4_generic_blas.npz).

Run:  MKL_CBWR=COMPATIBLE python oracle/make_golden_generic_blas.py      (needs the reference checkout: SGDFR_REFERENCE; CPU only)

kat4_generator256.npz was captured where MKL runs its AVX-512 kernels; on hosts where MKL takes its generic path (AMD EPYC,
or MKL_CBWR=COMPATIBLE) the fp32 mapping network sums in another order and its latents move by ~12 ulp, past KAT-4's 1e-6
bar although oracle and reference still agree on that path.  This capture is the reference on the generic path, checked
against the oracle on the same path at the same 1e-6, so tests/test_cpu_oracle.py holds the oracle to the reference of
either path.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import make_golden as MG                                   # noqa: E402
from oracle import sg2_oracle as O                                     # noqa: E402
from stylegan_directions_face_reenactment_amd import synthetic as S   # noqa: E402


def main():
    import numpy as np
    if os.environ.get('MKL_CBWR') != 'COMPATIBLE':
        raise SystemExit('run with MKL_CBWR=COMPATIBLE (MKL reads it before its first call)')
    M = MG.import_reference()[0]
    G, sd = MG.build_ref_generator(M, 256, 1, MG.SEED)
    torch.set_num_threads(8)
    with torch.no_grad():
        trunc_r = G.style(S.synthetic_z(MG.SEED, 64, key='kat4.ztrunc')).mean(0, keepdim=True)
        MG.check('cm1 mean_latent', O.mean_latent_from(sd, S.synthetic_z(MG.SEED, 64, key='kat4.ztrunc')), trunc_r, 1e-6)
        z = S.synthetic_z(MG.SEED, 2, key='kat4.z')
        _, lat_z = G([z], return_latents=True, truncation=0.7, truncation_latent=trunc_r)
        _, ol_z = O.generator_forward(sd, [z], return_latents=True, truncation=0.7, truncation_latent=trunc_r)
        MG.check('cm1 z-path latent', ol_z, lat_z, 1e-6)
    np.savez_compressed(os.path.join(MG.OUT, 'kat4_generic_blas.npz'), seed=np.array(MG.SEED), **{'cm1.trunc': MG.npy(trunc_r),
                                                                                                   'cm1.lat_z': MG.npy(lat_z)})


if __name__ == '__main__':
    main()

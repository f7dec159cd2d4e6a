"""CPU: the host side of the pooled PTI loss: the C ABI's declarations and refusals, what pool_loss.PoolMse and
finetune.PooledPtiLoss refuse before any launch, and the restatement's own arithmetic."""
import os
import re

import pytest
import torch

from util import ROOT
import pool_loss_restatement as PR


def test_c_abi_declares_the_pool_mse_entries_and_refuses_bad_shapes():
    from stylegan_directions_face_reenactment_amd import _native
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    declared = set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header))
    names = {'sgdfr_pool_mse_f32', 'sgdfr_pool_mse_bwd_f32', 'sgdfr_pool_mse_workspace_bytes'}
    assert names <= declared and {'sgdfr_pool_mse_f32', 'sgdfr_pool_mse_bwd_f32'} <= set(_native.SIGNATURES)
    assert _native.SIZE_QUERIES['sgdfr_pool_mse_workspace_bytes'] == 2
    lib = _native.load()
    # one float per block of 256 output pixels, at most 65536 blocks
    assert lib.sgdfr_pool_mse_workspace_bytes(1, 6) == 4 and lib.sgdfr_pool_mse_workspace_bytes(2, 5) == 4
    assert lib.sgdfr_pool_mse_workspace_bytes(1, 256) == 4 * 256 and lib.sgdfr_pool_mse_workspace_bytes(3, 16) == 4 * 3
    assert lib.sgdfr_pool_mse_workspace_bytes(4096, 8192) == 4 * 65536
    for B, P in ((0, 8), (4097, 8), (1, 0), (1, 8193)):
        assert lib.sgdfr_pool_mse_workspace_bytes(B, P) == -1
        assert lib.sgdfr_pool_mse_f32(None, None, B, P, 2, None, None, None, 0, None) != 0 and b'bad shape' in lib.sgdfr_last_error()
        assert lib.sgdfr_pool_mse_bwd_f32(None, None, None, None, B, P, 2, None, None) != 0 and b'bad shape' in lib.sgdfr_last_error()
    for f in (0, 3, 8):
        assert lib.sgdfr_pool_mse_f32(None, None, 1, 8, f, None, None, None, 0, None) != 0 and b'pooling factor' in lib.sgdfr_last_error()
        assert lib.sgdfr_pool_mse_bwd_f32(None, None, None, None, 1, 8, f, None, None) != 0 and b'pooling factor' in lib.sgdfr_last_error()
    assert lib.sgdfr_pool_mse_f32(None, None, 1, 8, 2, None, None, None, 0, None) != 0 and b'null' in lib.sgdfr_last_error()
    assert lib.sgdfr_pool_mse_bwd_f32(None, None, None, None, 1, 8, 2, None, None) != 0 and b'null' in lib.sgdfr_last_error()


def test_pool_mse_refuses_on_the_host():
    from stylegan_directions_face_reenactment_amd.pool_loss import PoolMse, pool_mse_backward
    x, real = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match=r'square RGB images \[B,3,S,S\]'):
        PoolMse.apply(torch.zeros(2, 3, 16, 12), real, 8)
    with pytest.raises(ValueError, match=r'square RGB images'):
        PoolMse.apply(torch.zeros(2, 1, 16, 16), real, 8)
    with pytest.raises(ValueError, match=r'square RGB images'):
        PoolMse.apply(torch.zeros(3, 16, 16), real, 8)
    with pytest.raises(ValueError, match=r'must be \[2,3,8,8\]'):
        PoolMse.apply(x, torch.zeros(1, 3, 8, 8), 8)
    with pytest.raises(ValueError, match=r'must be \[2,3,4,4\]'):             # P * f mismatch: real is 8 x 8, P says 4
        PoolMse.apply(x, real, 4)
    with pytest.raises(ValueError, match='factor of 1, 2 or 4'):              # f = 3
        PoolMse.apply(torch.zeros(2, 3, 24, 24), real, 8)
    with pytest.raises(ValueError, match='factor of 1, 2 or 4'):              # f = 8
        PoolMse.apply(torch.zeros(2, 3, 64, 64), real, 8)
    with pytest.raises(ValueError, match='factor of 1, 2 or 4'):              # not a divisor
        PoolMse.apply(torch.zeros(2, 3, 20, 20), real, 8)
    with pytest.raises(ValueError, match='P must be an int'):
        PoolMse.apply(x, real, 8.0)
    with pytest.raises(ValueError, match='no gradient'):
        PoolMse.apply(x, real.clone().requires_grad_(True), 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        PoolMse.apply(x, real, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pool_mse_backward(None, real, real, torch.ones(1), 2)


class _Lpips:
    """Stands where the LPIPS head stands: PooledPtiLoss asks it for the target features at construction."""

    class _Target:
        source_version = 0

    def target(self, y):
        t = self._Target()
        t.source_version = y._version
        return t


def test_pooled_pti_loss_refuses_on_the_host():
    from stylegan_directions_face_reenactment_amd.finetune import PooledPtiLoss
    real = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match=r'must be \[B,3,8,8\]'):
        PooledPtiLoss(_Lpips(), torch.zeros(1, 3, 16, 16), 8)
    with pytest.raises(ValueError, match=r'must be \[B,3,256,256\]'):        # P defaults to 256
        PooledPtiLoss(_Lpips(), real)
    with pytest.raises(ValueError, match='positive int'):
        PooledPtiLoss(_Lpips(), real, 0)
    loss = PooledPtiLoss(_Lpips(), real, 8, pt_lpips_lambda=2)
    assert loss.P == 8 and loss.pt_lpips_lambda == 2.0 and loss.real.data_ptr() == real.data_ptr()
    with pytest.raises(RuntimeError, match='different real image'):
        loss(torch.zeros(1, 3, 16, 16), real.clone(), 100)
    with pytest.raises(ValueError, match='factor of 1, 2 or 4'):
        loss(torch.zeros(1, 3, 24, 24), real, 100)
    with pytest.raises(ValueError, match=r'must be \[2,3,8,8\]'):
        loss(torch.zeros(2, 3, 16, 16), real, 100)
    with pytest.raises(RuntimeError, match='no CPU path'):
        loss(torch.zeros(1, 3, 16, 16), real, 100)
    real.add_(1.0)
    with pytest.raises(RuntimeError, match='modified in place'):
        loss(torch.zeros(1, 3, 16, 16), real, 100)


def test_restatement_is_the_formula_of_the_backward_kernel():
    """dx = (g_pooled + g_mse 2 (pooled - real) / (3 B P^2)) / f^2 on every pixel of a window, in fp64."""
    torch.manual_seed(3)
    B, P, f = 2, 5, 2
    x, real = torch.randn(B, 3, P * f, P * f, dtype=torch.float64), torch.randn(B, 3, P, P, dtype=torch.float64)
    gp, gm = torch.randn(B, 3, P, P, dtype=torch.float64), torch.tensor(0.7, dtype=torch.float64)
    pooled, mse = PR.forward(x, real, P)
    assert torch.allclose(pooled, x.view(B, 3, P, f, P, f).mean((3, 5)), rtol=0, atol=1e-15)
    assert abs(float(mse) - float(((pooled - real) ** 2).sum() / (3 * B * P * P))) < 1e-15
    for a, b in ((gp, gm), (gp, None), (None, gm)):
        want = ((0 if a is None else a) + (0 if b is None else b) * 2 * (pooled - real) / (3 * B * P * P)) / (f * f)
        want = want.repeat_interleave(f, 2).repeat_interleave(f, 3)
        assert torch.allclose(PR.backward(x, real, P, a, b), want, rtol=0, atol=1e-15)

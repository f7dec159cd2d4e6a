"""CPU: the hold policy of reenact.Reenactor (reenact.hold_failed_rows) against a plain Python loop, and the host contract of the
reenactment pipeline: what is refused before anything is launched.  The pipeline itself runs in tests/test_gpu_reenactor.py."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from util import ROOT, golden


def hold_loop(sv, ok, carry, carry_valid):
    """The policy as a loop: a failed row takes the last good vector seen so far (the carry first), zeros if there is none."""
    last = carry.clone() if carry_valid else None
    out = []
    for r in range(sv.shape[0]):
        if ok[r]:
            last = sv[r].clone()
            out.append(sv[r].clone())
        else:
            out.append(last.clone() if last is not None else torch.zeros_like(sv[r]))
    out = torch.stack(out) if out else sv.clone()
    return out, (last if last is not None else torch.zeros_like(carry)), last is not None


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rows(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    sv = torch.randn(n, D, generator=g)
    sv[::3, 0] = -0.0                                                     # bit patterns a float comparison would not tell apart
    return sv


def check(sv, ok, carry, valid):
    from stylegan_directions_face_reenactment_amd.reenact import hold_failed_rows
    poisoned = sv.clone()
    poisoned[~ok] = float('nan')                                          # what a failed row holds means nothing
    got, c, v = hold_failed_rows(poisoned, ok, carry, torch.tensor(valid))
    want, wc, wv = hold_loop(sv, ok.tolist(), carry, valid)
    assert bits(got, want), (ok.tolist(), valid)
    assert bits(got[ok], sv[ok])                                          # ok rows pass through bit for bit
    assert v.dtype == torch.bool and v.dim() == 0 and bool(v) == wv
    assert bits(c, wc) and c.shape == carry.shape
    return got, c, v


@pytest.mark.parametrize('valid', [False, True])
def test_hold_equals_the_loop_for_every_mask_up_to_six_rows(valid):
    D = 15
    carry = rows(1, D, 99)[0] + 5.0
    count = 0
    for n in range(1, 7):
        sv = rows(n, D, n)
        for mask in itertools.product([False, True], repeat=n):
            check(sv, torch.tensor(mask), carry, valid)
            count += 1
    assert count == 2 + 4 + 8 + 16 + 32 + 64


@pytest.mark.parametrize('D', [12, 15])
def test_hold_on_a_thousand_rows_and_across_two_calls(D):
    from stylegan_directions_face_reenactment_amd.reenact import hold_failed_rows
    n = 1000
    sv = rows(n, D, D)
    ok = torch.rand(n, generator=torch.Generator().manual_seed(7)) < 0.6
    ok[:3] = False                                                        # the head of the call reads the carry
    carry = rows(1, D, 5)[0]
    for valid in (False, True):
        whole, c, v = check(sv, ok, carry, valid)
        # two consecutive calls are one call on the concatenation, wherever the cut falls
        for cut in (1, 2, 3, 4, 500, 999):
            a, ca, va = hold_failed_rows(sv[:cut], ok[:cut], carry, torch.tensor(valid))
            b, cb, vb = hold_failed_rows(sv[cut:], ok[cut:], ca, va)
            assert bits(torch.cat([a, b]), whole) and bits(cb, c) and bool(vb) == bool(v), cut
    # no ok row at all and no carry: zeros, and the carry stays invalid
    none = torch.zeros(4, dtype=torch.bool)
    got, c, v = hold_failed_rows(sv[:4], none, carry, torch.tensor(False))
    assert (got == 0).all() and not bool(v) and (c == 0).all()
    got, c, v = hold_failed_rows(sv[:4], none, carry, torch.tensor(True))
    assert bits(got, carry.expand(4, D)) and bool(v) and bits(c, carry)
    empty, c, v = hold_failed_rows(sv[:0], none[:0], carry, torch.tensor(True))
    assert empty.shape == (0, D) and bits(c, carry) and bool(v)


def cpu_parts():
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.model import Generator
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    G = Generator(32, 512, 8, channel_multiplier=1)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    shifts = ShiftVectors('voxceleb', 15, 6.0, ranges=golden('kat8_shift.npz')['ranges_voxceleb'])
    return G, A, shifts


def test_reenactor_refuses_cpu_frames_and_unknown_options():
    from stylegan_directions_face_reenactment_amd import reenact
    G, A, shifts = cpu_parts()
    r = reenact.Reenactor(G, A, None, None, None, None, shifts, truncation=1.0)
    frame = torch.zeros(1, 96, 128, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        r.set_source(frame, optimize=False)
    with pytest.raises(RuntimeError, match='no CPU path'):
        r.reenact(frame)
    with pytest.raises(RuntimeError, match='LPIPS'):                      # optimize=True is the default
        r.set_source(frame)
    with pytest.raises(RuntimeError, match='on_fail'):
        r.reenact(frame, on_fail='skip')
    with pytest.raises(RuntimeError, match='output'):
        r.reenact(frame, output='grid')
    with pytest.raises(RuntimeError, match='truncation'):
        reenact.Reenactor(G, A, None, None, None, None, shifts)           # truncation 0.7 without the truncation latent
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    with pytest.raises(RuntimeError, match='directions'):
        reenact.Reenactor(G, A, None, None, None, None, ShiftVectors('ffhq', 12, 6.0, ranges=golden('kat8_shift.npz')['ranges_ffhq']), truncation=1.0)
    assert r.pool_to is None and reenact.ON_FAIL == ('hold', 'source', 'raise') and reenact.OUTPUTS == ('video', 'images')


def test_session_pool_to_takes_factors_of_one_two_and_four_only():
    from stylegan_directions_face_reenactment_amd.reenact import ReenactmentSession
    G, A, _ = cpu_parts()
    code = torch.zeros(1, G.n_latent, 512)
    for pool_to, f in ((None, 1), (32, 1), (16, 2), (8, 4)):
        s = ReenactmentSession(G, A, code, truncation=1.0, pool_to=pool_to)
        assert s.pool_f == f and s.pool_to == (pool_to if f > 1 else None)
    for bad in (4, 5, 0, -16, 64, 16.0, '16', True):
        with pytest.raises(RuntimeError, match='pool_to'):
            ReenactmentSession(G, A, code, truncation=1.0, pool_to=bad)


def test_video_frames_entry_refuses_cpu_tensors_and_bad_arguments_before_any_launch():
    from stylegan_directions_face_reenactment_amd import _native as N, reenact
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        reenact.video_frames_uint8(x, [], 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        reenact.pool_images(x, 4)
    lib = N.load()
    fake = ctypes.c_void_p(64)                                            # never dereferenced: every case is refused first
    ptrs, strides = (ctypes.c_void_p * 3)(64, None, 64), (ctypes.c_int64 * 3)(0, 0, 192)
    assert lib.sgdfr_video_frames_f32(fake, 1, 8, 3, ptrs, strides, 3, fake, 0, None) != 0 and b'1, 2 or 4' in lib.sgdfr_last_error()
    assert lib.sgdfr_video_frames_f32(fake, 1, 8, 1, ptrs, strides, 4, fake, 0, None) != 0 and b'left panels' in lib.sgdfr_last_error()
    assert lib.sgdfr_video_frames_f32(fake, 1, 8, 1, None, None, 1, fake, 0, None) != 0 and b'arrays' in lib.sgdfr_last_error()
    strides[2] = 191
    assert lib.sgdfr_video_frames_f32(fake, 1, 8, 1, ptrs, strides, 3, fake, 0, None) != 0 and b'stride' in lib.sgdfr_last_error()
    strides[2] = 192
    assert lib.sgdfr_video_frames_f32(fake, 1, 8, 1, ptrs, strides, 3, None, 0, None) != 0 and b'null' in lib.sgdfr_last_error()
    assert lib.sgdfr_video_frames_f32(None, 0, 8, 1, ptrs, strides, 3, None, 0, None) == 0          # nothing to do
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    assert 'sgdfr_video_frames_f32' in set(re.findall(r'\b(sgdfr_[a-z0-9_]+)\s*\(', header)) and 'sgdfr_video_frames_f32' in N.SIGNATURES
    assert N.ABI_VERSION == 23 and lib.sgdfr_abi_version() == 23          # one symbol added, nothing moved

"""CPU: PTI's locality regulariser, pinned off the device: the fp64 restatement (tests/locality_restatement.py) against the
reference's own ball_holder_loss_lazy results (kat25, scripts/make_golden_locality.py), and the extent of the norm for a 2-D and a 3-D
pivot.

Bars.  Codes and r: locality_restatement.code_bar / norm_bar, from fp32's unit roundoff and the depth of the sum (for the reference's
fp32 torch.norm, whose order is torch's own, the number of terms).  Loss: 1e-3 absolute, the image bar; gradients: 5e-4 of the
largest element, the gradient bar (README "Parity").  The figures are printed."""
import torch

from util import S, golden
import locality_restatement as R


def test_restatement_meets_the_reference_results_of_kat25():
    g = golden('kat25_locality.npz')
    assert int(g['seed']) == R.SEED
    worst = R.meets({k: g[k] for k in g.files}, S)
    assert sorted(worst) == sorted(tag for tag, _, _ in R.CASES)
    for tag, size, n in R.CASES:
        assert g['codes_' + tag].shape == (n, 2 * (size.bit_length() - 1) - 2, 512) and g['r_' + tag].shape == (n,)


def test_a_2d_pivot_takes_the_norm_over_512_elements_a_3d_pivot_over_all_rows():
    L, D = 8, 512
    w = S.counter_tensor(R.SEED, 'loc.w', (2, D)).double()
    p2 = S.counter_tensor(R.SEED, 'loc.p2', (1, D)).double()
    p3 = p2.unsqueeze(1).repeat(1, L, 1)                                  # the same W code in every row
    c2, r2 = R.morph(w, p2)
    c3, r3 = R.morph(w, p3)
    assert c2.shape == (2, D) and c3.shape == (2, L, D)
    # L identical rows: the norm over L * D elements is sqrt(L) x the norm over D, so the 3-D codes sit sqrt(L) x closer to the pivot
    assert torch.allclose(r3, r2 * L ** 0.5, rtol=1e-14, atol=0)
    assert torch.allclose((c3 - p3)[:, 0] * L ** 0.5, c2 - p2, rtol=1e-12, atol=1e-13)
    for c, p in ((c2, p2), (c3, p3)):                                     # every sample lies on the ball of radius alpha
        dist = (c - p).flatten(1).norm(dim=1)
        assert torch.allclose(dist, torch.full_like(dist, R.ALPHA), rtol=1e-13, atol=0)
    # a sample equal to the pivot: 0 / 0, NaN in its rows only
    c, r = R.morph(torch.cat([p2, w[:1]]), p2)
    assert float(r[0]) == 0.0 and bool(torch.isnan(c[0]).all()) and bool(torch.isfinite(c[1]).all())
    # the bars are what their derivations say
    assert R.norm_bar(12) == 2 * (15 / 2 + 1) * 2.0 ** -24
    assert R.code_bar(12, 10.0, 4.0) == 10.0 * (3 * 2.0 ** -24 + R.norm_bar(12)) + 4.0 * 2.0 ** -24

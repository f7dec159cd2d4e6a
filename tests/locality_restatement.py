"""PTI's locality regulariser (libs/criteria/PTI/localitly_regulizer.py ball_holder_loss_lazy) written out in any dtype on any
device: fp64 on the CPU is the yardstick of tests/test_cpu_locality.py, against the reference's own results (kat25), and the
statement a device port of the term is to be held to.

The generator is the oracle's (oracle/sg2_oracle.py generator_forward) on a state dict `P`; `lpips_net` below is the small stand-in
scripts/make_golden_locality.py hands the reference (the real LPIPS needs weights nobody can fetch offline; the HIP LPIPS is pinned by
kat9).  The two stated deviations hold here too: `trunc` is an argument, and the mapped samples `w_z` are.
"""
import math

import torch
import torch.nn.functional as F

from oracle import sg2_oracle as O

ALPHA, L2_LAMBDA, LPIPS_LAMBDA, TRUNCATION = 10.0, 0.1, 0.1, 0.7       # hyperparameters.py:7-11, localitly_regulizer.py:37
U = 2.0 ** -24                                                          # unit roundoff of fp32: half its epsilon
IMAGE_BAR, GRAD_BAR = 1e-3, 5e-4                                        # README "Parity": absolute on images, relative on gradients


def morph(w_z, pivot, alpha=ALPHA):
    """get_morphed_w_code per sample (:15-22, :34): w_z [n,D], pivot [1,D] or [1,L,D] -> (codes [n,D] or [n,L,D], r [n]).
    d = w_z[i][None] - pivot broadcasts over the pivot's rows; r is ONE norm over all of d."""
    codes, rs = [], []
    for w in w_z:
        d = w.unsqueeze(0) - pivot
        r = torch.sqrt((d * d).sum())
        codes.append(pivot + alpha * d / r)
        rs.append(r)
    return torch.cat(codes), torch.stack(rs)


def norm_bar(depth):
    """Relative bar of r = sqrt(sum d^2) computed in fp32 from fp32 inputs, against exact arithmetic: every d carries one rounding
    (u), so every d^2 carries 2u and one more for the product; a sum of non-negative terms along chains of `depth` additions adds
    depth * u; the square root halves the total and adds its own u.  Twice that, for the second-order terms and a sum that rounds
    upwards all the way."""
    return 2 * ((3 + depth) / 2 + 1) * U


def code_bar(depth, alpha, out_max):
    """Absolute bar of a code pivot + alpha * d / r in fp32: |d| / r <= 1, so the quotient is at most alpha and carries d's
    rounding, the product's, the division's and r's relative error (norm_bar); the final add rounds the result (out_max) once."""
    return alpha * (3 * U + norm_bar(depth)) + out_max * U


def lpips_net(x, y):
    """A small LPIPS-shaped distance [N,1,1,1]: four 3x3 features from fixed taps, normalised over the channels as LPIPS does
    (networks.py normalize_activation), squared difference, mean over channels and pixels.  Symmetric and differentiable.  The 0.1 under the root (LPIPS adds
    1e-10 outside it, to post-ReLU features) keeps the gradient well conditioned where all four features vanish: with 1e-10 the
    reference's own fp32 gradient is off by 1e-3 of its maximum from fp64 at such pixels, twice the gradient bar."""
    i = torch.arange(4 * 3 * 3 * 3, dtype=torch.float64)
    k = torch.cos(0.7 * i + 0.3).reshape(4, 3, 3, 3).to(x.dtype).to(x.device) / 3.0
    fx, fy = F.conv2d(x, k, padding=1), F.conv2d(y, k, padding=1)
    fx = fx / torch.sqrt((fx * fx).sum(1, keepdim=True) + 0.1)
    fy = fy / torch.sqrt((fy * fy).sum(1, keepdim=True) + 0.1)
    return ((fx - fy) ** 2).mean((1, 2, 3), keepdim=True)


def images(P, codes, trunc, truncation=TRUNCATION):
    return O.generator_forward(P, [codes], truncation=truncation, truncation_latent=trunc, input_is_latent=True)[0]


def pair_loss(old, new, lpips=lpips_net, l2_lambda=L2_LAMBDA, lpips_lambda=LPIPS_LAMBDA):
    """:41-48 for one pair of image batches."""
    return l2_lambda * F.mse_loss(old, new) + lpips_lambda * torch.mean(torch.squeeze(lpips(old, new)))


def ball_holder_loss(P_new, P_old, w_z, pivot, trunc, alpha=ALPHA, lpips=lpips_net, truncation=TRUNCATION):
    """:27-50 after the draw: (loss, [new image of every sample], codes, r); the new images are graph leaves' children, so
    torch.autograd.grad(loss, new_images + [P_new[key]]) gives what kat25 records."""
    codes, r = morph(w_z, pivot, alpha)
    loss, news = 0.0, []
    for i in range(codes.shape[0]):
        w = codes[i:i + 1]
        new = images(P_new, w, trunc, truncation)
        with torch.no_grad():
            old = images(P_old, w, trunc, truncation)
        loss = loss + pair_loss(old, new, lpips)
        news.append(new)
    return loss / codes.shape[0], news, codes, r


# ---- the cases of kat25: seeded states, shared by scripts/make_golden_locality.py and the tests
SEED = 20261215
CASES = (('g32n1', 32, 1), ('g32n3', 32, 3), ('g64n1', 64, 1), ('g64n3', 64, 3))


def grad_key(size):
    """The small parameter tensor whose gradient kat25 records: the bias of the last styled conv."""
    return 'convs.%d.activate.bias' % (2 * (int(math.log2(size)) - 2) - 1)


def case_states(S, size):
    """(P_old, P_new, pivot [1,L,512], trunc [1,512]) in fp32: the seeded synthetic generator with ZERO noise strengths (the noise
    draw of a forward cannot matter), the tuned copy = the original with every styled conv's bias and the ToRGB weights moved."""
    old = S.synthetic_state_dict(O.template_state(size, 512, 8, 1), seed=SEED)
    for k in old:
        if k.endswith('.noise.weight'):
            old[k] = torch.zeros_like(old[k])
    new = {k: v.clone() for k, v in old.items()}
    for k in new:
        if k.endswith('.activate.bias') or (k.startswith('to_rgb') and k.endswith('.conv.weight')):
            new[k] = new[k] + S.counter_tensor(SEED, 'kat25.move.%d.%s' % (size, k), tuple(new[k].shape), 0.0, 0.3)
    n_latent = 2 * int(math.log2(size)) - 2
    pivot = S.synthetic_latents(SEED, 1, n_latent=n_latent, key='kat25.pivot.%d' % size)
    trunc = S.counter_tensor(SEED, 'kat25.trunc.%d' % size, (1, 512))
    return old, new, pivot, trunc


def meets(out, S):
    """The fp64 restatement against the recorded results, at the bars of tests/test_cpu_locality.py (which calls this too; S: the package's synthetic module)."""
    worst = {}
    for tag, size, n in CASES:
        g = {k[:-len(tag) - 1]: torch.as_tensor(out[k]) for k in out if k.endswith('_' + tag)}
        old, new, pivot, trunc = case_states(S, size)
        assert torch.equal(pivot, g['pivot']) and torch.equal(trunc, g['trunc'])
        P_old, P_new = O.cast_state(old, torch.float64), O.cast_state(new, torch.float64)
        key = grad_key(size)
        P_new[key].requires_grad_(True)
        loss, news, codes, r = ball_holder_loss(P_new, P_old, g['w_z'].double(), pivot.double(), trunc.double())
        grads = torch.autograd.grad(loss, news + [P_new[key]])
        dimg, dparam = torch.cat(grads[:-1]), grads[-1]
        M = pivot.numel()
        # the reference's norm runs in fp32 in an order of torch's choosing: no chain is longer than the M terms themselves
        e_r = float(((r - g['r'].double()).abs() / r).max())
        e_c = float((codes - g['codes'].double()).abs().max())
        e_l = abs(loss.item() - g['loss'].item())
        e_i = float((dimg - g['dimg'].double()).abs().max() / dimg.abs().max())
        e_p = float((dparam - g['dparam'].double()).abs().max() / dparam.abs().max())
        bar_r, bar_c = norm_bar(M), code_bar(M, ALPHA, float(codes.abs().max()))
        print('%s: r %.3e (bar %.3e)  codes %.3e (bar %.3e)  loss %.6f off by %.3e (bar %.0e)  dL/dimage %.3e  dL/d%s %.3e (bar %.0e)' % (
            tag, e_r, bar_r, e_c, bar_c, loss.item(), e_l, IMAGE_BAR, e_i, key, e_p, GRAD_BAR))
        assert e_r <= bar_r and e_c <= bar_c and e_l <= IMAGE_BAR and e_i <= GRAD_BAR and e_p <= GRAD_BAR, tag
        worst[tag] = (e_r, e_c, e_l, e_i, e_p)
    return worst

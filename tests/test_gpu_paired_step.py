"""GPU: the paired and the real-image direction-training steps and the validation metrics (train_step.py: PairedLosses,
PairedTrainer, DirectionTrainer.step_real, evaluation_metrics, evaluate_pairs) on the HIP heads.

B = 2 frames, 256 x 256, channel multiplier 1; all seven networks carry synthetic weights, built as tests/test_gpu_train_step.py
builds them (its Rig).  The "real frames" are renders of W+ codes next to the ones handed to the step, so that a frame and the
render of its code differ, as an inverted frame and its inversion do.

Bars.  Each step is compared with the same sequence written out from public calls plus STOCK torch ops for what pair_loss.py
replaces (the 0..255 transform and the two L1 terms).  The FLAME and identity terms are the same kernels on the same numbers: equal
bits.  loss_pixel_wise / loss_w_reg: 2e-6 relative (tests/test_cpu_pair_loss.py).  loss_perceptual: 1e-5 relative -- its input t(x)
may differ from stock torch's by an ulp where torch's device kernel multiplies by a reciprocal and ours divides; the test prints
how many values differ (measured on an MI355X: 63 of 393216 values, by 1.5e-5; the term itself came out equal to the last bit, but
its input is not bit-equal, so the bar stays).  dL/dA: 1e-5 of its largest element, the bar of tests/test_gpu_train_step.py, for its reason (fp32 atomics in
the generator backward).  Every test prints the figures it asserts on.
"""
import numpy as np
import pytest
import torch

from util import S, SEED, golden
from test_gpu_train_step import Rig, _bits, _rel

pytestmark = pytest.mark.gpu

B = 2
GRAD_BAR, MEAN_REL, LPIPS_REL = 1e-5, 2e-6, 1e-5
LAMBDAS7 = {'lambda_shape': 1.0, 'lambda_mouth_shape': 0.7, 'lambda_eye_shape': 1.3, 'lambda_identity': 10.0, 'lambda_perceptual': 6.0,
            'lambda_pixel_wise': 0.01, 'lambda_w_reg': 0.3}
LAMBDAS5 = {k: LAMBDAS7[k] for k in list(LAMBDAS7)[:5]}


class PairedRig(Rig):
    def __init__(self):
        super().__init__()
        from stylegan_directions_face_reenactment_amd.generic import generate_image
        n = self.G.n_latent
        self.ws = S.synthetic_latents(SEED, B, n_latent=n, key='paired.ws').cuda()
        self.wt = S.synthetic_latents(SEED, B, n_latent=n, key='paired.wt').cuda()
        near = lambda w, key: w + 0.25 * S.synthetic_latents(SEED, B, n_latent=n, key=key).cuda()
        with torch.no_grad():                                              # the frames: close to, not equal to, the codes' renders
            self.source_img = generate_image(self.G, near(self.ws, 'paired.ds'), 0.7, self.trunc, input_is_latent=True).clone()
            self.target_img = generate_image(self.G, near(self.wt, 'paired.dt'), 0.7, self.trunc, input_is_latent=True).clone()
        self.z_target = S.synthetic_z(SEED, 2 * B, key='paired.zt').cuda()
        self.z_syn = S.synthetic_z(SEED, B, key='paired.zsyn').cuda()

    def paired_losses(self, lambdas=LAMBDAS7):
        from stylegan_directions_face_reenactment_amd.train_step import PairedLosses
        return PairedLosses(self.flame, self.id_loss, self.lpips, lambdas)

    def paired_trainer(self, A, lambdas=LAMBDAS7):
        from stylegan_directions_face_reenactment_amd.train_step import PairedTrainer
        return PairedTrainer(self.G, A, self.det, self.fan, self.E, self.paired_losses(lambdas), self.shifts, truncation=0.7, trunc=self.trunc)


@pytest.fixture(scope='module')
def rig():
    return PairedRig()


def stock_255(image):
    """image_utils.py:87-94 in stock torch ops (out of place: autograd must see them)."""
    return image.clone().clamp(min=-1, max=1).add(1).div(1 - (-1) + 1e-5).mul(255.0)


def _close(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_paired_step_equals_the_sequence_written_out(rig):
    """trainer.py:352-383 with utils_train.py:435-499, line by line, against PairedTrainer.step.  The seven lambdas are non-zero and
    pairwise different: a swapped term or a swapped image shows."""
    from stylegan_directions_face_reenactment_amd import pair_loss as PL
    from stylegan_directions_face_reenactment_amd.flame import ShapeLoss
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.train_step import PAIRED_LOSS_KEYS, shape_params, to_host
    assert len(set(LAMBDAS7.values())) == 7 and all(v != 0 for v in LAMBDAS7.values())
    G, lam = rig.G, LAMBDAS7

    # ---- the step under test
    A1 = rig.direction_matrix()
    before = [p.detach().clone() for p in A1.parameters()]
    images_before = PL.COUNTERS['images_255']
    loss1, dict1 = rig.paired_trainer(A1).step(rig.ws, rig.source_img, rig.wt, rig.target_img)
    g1 = [p.grad.clone() for p in A1.parameters()]
    assert PL.COUNTERS['images_255'] == images_before + 2                                                 # t(x) and t(y), once each

    # ---- the same sequence, written out
    A2 = rig.direction_matrix()
    opt = torch.optim.Adam(A2.parameters(), lr=1e-4, weight_decay=5e-4)                                   # trainer.py:325
    with torch.no_grad():
        params_source, angles_source = shape_params(rig.det, rig.fan, rig.E, rig.source_img)              # :360
        params_target, angles_target = shape_params(rig.det, rig.fan, rig.E, rig.target_img)              # :366
    shift_vector = rig.shifts.make_shift_vector(params_source, params_target, angles_source, angles_target)   # :370
    shift = A2(shift_vector)
    imgs_shifted, shifted_latents = generate_image(G, rig.ws, 0.7, rig.trunc, shift_code=shift, input_is_latent=True,
                                                   return_latents=True)                                  # :372
    params_shifted, angles_shifted = shape_params(rig.det, rig.fan, rig.E, imgs_shifted)                  # :375
    x255, y255 = stock_255(imgs_shifted), stock_255(rig.target_img)                                       # utils_train :438-439
    gt = {'pose': params_target['pose'], 'exp': params_target['alpha_exp'], 'shape': params_target['alpha_shp']}          # :444-449
    reen = {'pose': params_shifted['pose'], 'shape': params_shifted['alpha_shp'], 'exp': params_shifted['alpha_exp']}     # :455-457
    loss2, terms = ShapeLoss(rig.flame)(gt, reen, lam['lambda_shape'], lam['lambda_mouth_shape'], lam['lambda_eye_shape'])   # :464-473
    loss_identity = lam['lambda_identity'] * rig.id_loss(imgs_shifted, rig.target_img.detach())           # :477
    loss_perceptual = lam['lambda_perceptual'] * rig.lpips(x255, y255.detach())                           # :483
    loss_pixel_wise = lam['lambda_pixel_wise'] * torch.nn.L1Loss()(y255.detach(), x255)                   # :488, losses.py:16
    loss_w_reg = lam['lambda_w_reg'] * torch.nn.L1Loss()(shifted_latents, rig.wt)                         # :494
    loss2 = loss2 + loss_identity + loss_perceptual + loss_pixel_wise + loss_w_reg
    A2.zero_grad()                                                                                        # trainer.py:381-383
    loss2.backward()
    opt.step()
    g2 = [p.grad.clone() for p in A2.parameters()]
    dict2 = {'loss_shape': terms['loss_shape'], 'loss_eye': terms['loss_eye'], 'loss_mouth': terms['loss_mouth'],
             'loss_identity': loss_identity, 'loss_perceptual': loss_perceptual, 'loss_pixel_wise': loss_pixel_wise,
             'loss_w_reg': loss_w_reg, 'loss': loss2}

    host = to_host(dict1)
    print('paired step: %s' % ', '.join('%s %.6g' % (k, host[k]) for k in PAIRED_LOSS_KEYS))
    print('paired step: faces found in %s of the source, %s of the target, %s of the shifted rows' % tuple(
        int((a[:, 0] != -180).sum()) for a in (angles_source, angles_target, angles_shifted)))
    assert tuple(dict1) == PAIRED_LOSS_KEYS and all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in dict1.values())
    assert all(0 < v < float('inf') for v in host.values())                                               # every term is live
    for k in ('loss_shape', 'loss_eye', 'loss_mouth', 'loss_identity'):
        assert _bits(dict1[k], dict2[k].detach()), (k, float(dict1[k]), float(dict2[k]))
    # how far is our t(x) from stock torch's on this device?
    with torch.no_grad():
        ours = PL.torch_range_1_to_255(imgs_shifted.detach())
        differ, far = int((ours != x255.detach()).sum()), float((ours - x255.detach()).abs().max())
    rp, rx, rw, rl = (_close(dict1[k], dict2[k].detach()) for k in ('loss_perceptual', 'loss_pixel_wise', 'loss_w_reg', 'loss'))
    print('paired step: t(x) differs from stock torch in %d of %d values (max %.3e); loss_perceptual rel %.3e (bar %.0e), loss_pixel_wise '
          'rel %.3e, loss_w_reg rel %.3e (bar %.0e), loss rel %.3e' % (differ, ours.numel(), far, rp, LPIPS_REL, rx, rw, MEAN_REL, rl))
    assert rp <= LPIPS_REL and rx <= MEAN_REL and rw <= MEAN_REL and rl <= LPIPS_REL and _bits(loss1, dict1['loss'])
    assert bool((angles_shifted[:, 0] != -180).any()) and bool((angles_target[:, 0] != -180).any())      # the shape terms carry gradient
    ra, rb = _rel(g1[0], g2[0]), _rel(g1[1], g2[1])
    print('paired step: dL/dA.weight rel %.3e, dL/dA.bias rel %.3e (bar %.0e); max |dL/dA.weight| %.3e' % (ra, rb, GRAD_BAR, float(g2[0].abs().max())))
    assert float(g2[0].abs().max()) > 0 and ra <= GRAD_BAR and rb <= GRAD_BAR
    assert all(not torch.equal(p.detach(), q) for p, q in zip(A1.parameters(), before))                  # the optimizer stepped
    assert G.saturated_pairs() == 0

    # ---- the callers' cam rows are not written to (the reference overwrites both with (8, 0, 0), :446-448, :458-460)
    with torch.no_grad():
        cams = (params_target['cam'].clone(), params_shifted['cam'].detach().clone())
        _, dict3 = rig.paired_losses().calculate_losses_paired({k: v.detach() for k, v in params_shifted.items()}, params_target,
                                                               imgs_shifted.detach(), rig.target_img, shifted_latents.detach(), rig.wt)
    assert _bits(params_target['cam'], cams[0]) and _bits(params_shifted['cam'].detach(), cams[1])
    assert float(cams[0].abs().max()) > 0 and not bool((cams[0][:, 1:] == 0).all())                       # ... and they were not (8, 0, 0) already
    assert all(_bits(dict3[k], dict1[k]) for k in PAIRED_LOSS_KEYS)


def test_terms_with_a_zero_lambda_are_dropped(rig):
    from stylegan_directions_face_reenactment_amd import pair_loss as PL
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.train_step import PAIRED_LOSS_KEYS, PairedLosses, shape_params
    with torch.no_grad():
        imgs_shifted, latents = generate_image(rig.G, rig.ws, 0.7, rig.trunc, input_is_latent=True, return_latents=True)
        params_shifted, _ = shape_params(rig.det, rig.fan, rig.E, imgs_shifted)
        params_target, _ = shape_params(rig.det, rig.fan, rig.E, rig.target_img)
        args = (params_shifted, params_target, imgs_shifted, rig.target_img, latents, rig.wt)
        _, full = rig.paired_losses().calculate_losses_paired(*args)
        drops = {'lambda_shape': ('loss_shape', 'loss_eye', 'loss_mouth'), 'lambda_mouth_shape': ('loss_mouth',), 'lambda_eye_shape': ('loss_eye',),
                 'lambda_identity': ('loss_identity',), 'lambda_perceptual': ('loss_perceptual',), 'lambda_pixel_wise': ('loss_pixel_wise',),
                 'lambda_w_reg': ('loss_w_reg',)}
        for name, gone in drops.items():
            before = PL.COUNTERS['images_255']
            _, d = rig.paired_losses(dict(LAMBDAS7, **{name: 0.0})).calculate_losses_paired(*args)
            assert tuple(d) == tuple(k for k in PAIRED_LOSS_KEYS if k not in gone), (name, tuple(d))
            made = PL.COUNTERS['images_255'] - before
            assert made == (0 if name == 'lambda_perceptual' else 2), (name, made)       # no LPIPS: no 0..255 image is written
            assert all(_bits(d[k], full[k]) for k in d if k in ('loss_identity', 'loss_perceptual', 'loss_pixel_wise', 'loss_w_reg')), name
        # heads of dead lambdas may be absent; an absent head of a live lambda, an unknown name and all-zero lambdas are refused
        _, d = PairedLosses(None, None, None, {'lambda_pixel_wise': 1.0}).calculate_losses_paired(*args)
        assert tuple(d) == ('loss_pixel_wise', 'loss') and _bits(d['loss'], d['loss_pixel_wise'])
    for bad in ({'lambda_shape': 1.0}, {'lambda_identity': 1.0}, {'lambda_perceptual': 1.0}, {'lambda_pixelwise': 1.0}, {}):
        with pytest.raises(ValueError):
            PairedLosses(None, None, None, bad)
    # the pixel-wise term with perceptual off: no image in a whole step either
    A = rig.direction_matrix()
    before = PL.COUNTERS['images_255']
    _, d = rig.paired_trainer(A, dict(LAMBDAS7, lambda_perceptual=0.0)).step(rig.ws, rig.source_img, rig.wt, rig.target_img)
    assert PL.COUNTERS['images_255'] == before and 'loss_perceptual' not in d and 'loss_pixel_wise' in d


def test_w_reg_alone_reaches_A(rig):
    """lambda_w_reg the only live lambda: the gradient of A comes through the returned latent alone and equals the stock chain's."""
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.train_step import shape_params
    A1, A2 = rig.direction_matrix(), rig.direction_matrix()
    loss1, d = rig.paired_trainer(A1, {'lambda_w_reg': 0.3}).step(rig.ws, rig.source_img, rig.wt, rig.target_img)
    assert tuple(d) == ('loss_w_reg', 'loss')
    with torch.no_grad():
        ps, as_ = shape_params(rig.det, rig.fan, rig.E, rig.source_img)
        pt, at = shape_params(rig.det, rig.fan, rig.E, rig.target_img)
    shift = A2(rig.shifts.make_shift_vector(ps, pt, as_, at))
    _, latents = generate_image(rig.G, rig.ws, 0.7, rig.trunc, shift_code=shift, input_is_latent=True, return_latents=True)
    loss2 = 0.3 * torch.nn.L1Loss()(latents, rig.wt)
    loss2.backward()
    g1, g2 = A1.linear.weight.grad, A2.linear.weight.grad
    rl, rg = _close(loss1, loss2.detach()), _rel(g1, g2)
    print('w_reg alone: loss rel %.3e (bar %.0e); dL/dA.weight rel %.3e (bar %.0e), max %.3e' % (rl, MEAN_REL, rg, GRAD_BAR, float(g2.abs().max())))
    assert float(g1.abs().max()) > 0 and rl <= MEAN_REL and rg <= GRAD_BAR


@pytest.mark.parametrize('synthetic_rows', [False, True], ids=['real', 'real_synthetic'])
def test_step_real_equals_the_sequence_written_out(rig, synthetic_rows):
    """trainer.py:250-296 with utils_train.py:376-433 against DirectionTrainer.step_real with the same injected draws; with
    source_z_syn the batch is 2 real + 2 synthetic rows (an even batch of 4 for make_shift_vector_50)."""
    from stylegan_directions_face_reenactment_amd.flame import ShapeLoss
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.train_step import LOSS_KEYS, shape_params
    G, lam = rig.G, LAMBDAS5
    rows = 2 * B if synthetic_rows else B
    z_syn = rig.z_syn if synthetic_rows else None
    z_target = rig.z_target[:rows]
    which, u = ([1, 5], torch.tensor([0.3, 0.8]).cuda()) if synthetic_rows else ([5], torch.tensor([0.8]).cuda())

    A1 = rig.direction_matrix()
    loss1, dict1 = rig.trainer(A1, LAMBDAS5).step_real(rig.ws, rig.source_img, z_target, source_z_syn=z_syn, target_indices=which, u=u)
    g1 = [p.grad.clone() for p in A1.parameters()]

    A2 = rig.direction_matrix()
    source_w, source_real_img = rig.ws, rig.source_img
    with torch.no_grad():
        if synthetic_rows:
            source_w_syn = G.get_latent(z_syn).unsqueeze(1).repeat(1, G.n_latent, 1)                                    # :262-263
            source_w = torch.cat((source_w, source_w_syn), dim=0)                                                        # :264
            source_real_img = torch.cat((source_real_img, generate_image(G, source_w_syn, 0.7, rig.trunc, input_is_latent=True)), dim=0)
        params_source, angles_source = shape_params(rig.det, rig.fan, rig.E, source_real_img)                            # :268
        imgs_target = generate_image(G, z_target, 0.7, rig.trunc, input_is_latent=False)                                 # :274
        params_target, angles_target = shape_params(rig.det, rig.fan, rig.E, imgs_target)
        render = generate_image(G, source_w, 0.7, rig.trunc, input_is_latent=True)                                       # what `step` would compare with
    shift_vector, target_indices = rig.shifts.make_shift_vector_50(params_source, params_target, angles_source, angles_target,
                                                                   target_indices=which, u=u)                           # :279
    shift = A2(shift_vector)
    imgs_shifted, _ = generate_image(G, source_w, 0.7, rig.trunc, shift_code=shift, input_is_latent=True, return_latents=True)   # :285
    params_shifted, angles_shifted = shape_params(rig.det, rig.fan, rig.E, imgs_shifted)
    gt = rig.shifts.get_params_gt_reenacted(params_source, params_target, shift_vector, target_indices, angles_source)
    gt['shape'] = params_source['alpha_shp']
    reen = {'pose': params_shifted['pose'], 'shape': params_shifted['alpha_shp'], 'exp': params_shifted['alpha_exp']}
    loss2, terms = ShapeLoss(rig.flame)(gt, reen, lam['lambda_shape'], lam['lambda_mouth_shape'], lam['lambda_eye_shape'])
    loss_identity = lam['lambda_identity'] * rig.id_loss(imgs_shifted, source_real_img.detach())                         # :288-289 -> utils_train :423
    loss_perceptual = lam['lambda_perceptual'] * rig.lpips(imgs_shifted, source_real_img.detach())                       # :428
    loss2 = loss2 + loss_identity + loss_perceptual
    loss2.backward()
    g2 = [p.grad.clone() for p in A2.parameters()]
    dict2 = {'loss_shape': terms['loss_shape'], 'loss_eye': terms['loss_eye'], 'loss_mouth': terms['loss_mouth'],
             'loss_identity': loss_identity, 'loss_perceptual': loss_perceptual, 'loss': loss2}
    print('step_real (%d rows): %s' % (rows, ', '.join('%s %.6g' % (k, float(dict1[k])) for k in LOSS_KEYS)))
    assert tuple(dict1) == LOSS_KEYS and tuple(imgs_shifted.shape) == (rows, 3, 256, 256)
    for k in LOSS_KEYS:
        assert _bits(dict1[k], dict2[k].detach()), (k, float(dict1[k]), float(dict2[k]))
    assert _bits(loss1, loss2.detach()) and all(0 < float(v) < float('inf') for v in dict1.values())
    ra, rb = _rel(g1[0], g2[0]), _rel(g1[1], g2[1])
    print('step_real (%d rows): dL/dA.weight rel %.3e, dL/dA.bias rel %.3e (bar %.0e); max |dL/dA.weight| %.3e' % (rows, ra, rb, GRAD_BAR,
                                                                                                                 float(g2[0].abs().max())))
    assert float(g2[0].abs().max()) > 0 and ra <= GRAD_BAR and rb <= GRAD_BAR
    # the identity and LPIPS terms are taken against the real FRAME: against the render of its code they come out different
    with torch.no_grad():
        id_render = lam['lambda_identity'] * rig.id_loss(imgs_shifted.detach(), render)
        lp_render = lam['lambda_perceptual'] * rig.lpips(imgs_shifted.detach(), render)
    print('step_real (%d rows): identity %.6g against the frame, %.6g against the render; LPIPS %.6g, %.6g'
          % (rows, float(dict1['loss_identity']), float(id_render), float(dict1['loss_perceptual']), float(lp_render)))
    assert _close(id_render, dict1['loss_identity']) > 1e-3 and _close(lp_render, dict1['loss_perceptual']) > 1e-3
    assert G.saturated_pairs() == 0


def _metrics_written_out(shifts, params_shifted, params_target, angles_shifted, angles_target, row=0):
    """utils_train.py:697-725 in numpy float64 for one row."""
    f = lambda v: v.detach().cpu().numpy().astype(np.float64)
    exp_r, exp_t = f(params_shifted['alpha_exp'])[row], f(params_target['alpha_exp'])[row]
    jaw_r, jaw_t = f(params_shifted['pose'])[row, 3], f(params_target['pose'])[row, 3]
    errs = []
    for j in range(shifts.learned_directions - shifts.count_pose):
        hi, lo = shifts.directions_exp[j]['max_shift'], shifts.directions_exp[j]['min_shift']
        errs.append(abs((exp_r[j] - lo) / (hi - lo) - (exp_t[j] - lo) / (hi - lo)))
    errs.append(abs((jaw_r - shifts.min_jaw) / (shifts.max_jaw - shifts.min_jaw) - (jaw_t - shifts.min_jaw) / (shifts.max_jaw - shifts.min_jaw)))
    ar, at = f(angles_shifted)[row], f(angles_target)[row]
    return (abs(ar[0] - at[0]) + abs(ar[1] - at[1]) + abs(ar[2] - at[2])) / 3, float(np.mean(errs))


def test_evaluation_metrics_and_evaluate_pairs(rig):
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    from stylegan_directions_face_reenactment_amd.train_step import evaluate_pairs, evaluation_metrics, shape_params
    G, A = rig.G, rig.direction_matrix()
    zs, zt = rig.zs[:B], rig.zt[:B]
    trainer = rig.trainer(A, LAMBDAS5)
    got = evaluate_pairs(trainer, zs, zt, False)
    with torch.no_grad():                                                                                 # utils_train.py:756-768
        imgs_source = generate_image(G, zs, 0.7, rig.trunc, input_is_latent=False)
        params_source, angles_source = shape_params(rig.det, rig.fan, rig.E, imgs_source)
        imgs_target = generate_image(G, zt, 0.7, rig.trunc, input_is_latent=False)
        params_target, angles_target = shape_params(rig.det, rig.fan, rig.E, imgs_target)
        shift_vector = rig.shifts.make_shifts_interpolation(params_source, params_target, angles_source, angles_target)
        assert _bits(shift_vector, rig.shifts.make_shift_vector(params_source, params_target, angles_source, angles_target))
        imgs_shifted = generate_image(G, zs, 0.7, rig.trunc, shift_code=A(shift_vector), input_is_latent=False)
        params_shifted, angles_shifted = shape_params(rig.det, rig.fan, rig.E, imgs_shifted)
        csim, pose, exp_error = evaluation_metrics(rig.shifts, rig.id_loss, params_shifted, params_target, angles_shifted, angles_target,
                                                   imgs_shifted, imgs_source)
        id_value = rig.id_loss(imgs_shifted, imgs_source)
    assert all(v.is_cuda and tuple(v.shape) == (B,) and v.dtype == torch.float32 for v in (csim, pose, exp_error))
    assert all(_bits(a, b) for a, b in zip(got, (csim, pose, exp_error)))                                 # evaluate_pairs is that sequence
    parts = {'G': G, 'A': A, 'det': rig.det, 'fan': rig.fan, 'E': rig.E, 'shifts': rig.shifts, 'id_loss': rig.id_loss, 'truncation': 0.7,
             'trunc': rig.trunc}
    assert all(_bits(a, b) for a, b in zip(evaluate_pairs(parts, zs, zt, False), got))
    with pytest.raises(ValueError, match='lack'):
        evaluate_pairs({'G': G}, zs, zt, False)
    for row in range(B):
        want_pose, want_exp = _metrics_written_out(rig.shifts, params_shifted, params_target, angles_shifted, angles_target, row)
        dp, de = abs(float(pose[row]) - want_pose), abs(float(exp_error[row]) - want_exp)
        print('metrics row %d: csim %.6f, pose %.6g (off by %.2e), exp_error %.6g (off by %.2e) (bar 1e-5 relative)'
              % (row, float(csim[row]), want_pose, dp, want_exp, de))
        assert dp <= 1e-5 * want_pose and de <= 1e-5 * want_exp
    dc = abs(float(csim.mean()) - (1 - float(id_value)))
    print('metrics: csim.mean() %.7f against 1 - id_loss %.7f: %.2e (bar 1e-6)' % (float(csim.mean()), 1 - float(id_value), dc))
    assert dc <= 1e-6 and bool((csim.abs() <= 1 + 1e-6).all())
    # the ffhq tables have no roll direction (-1): roll still counts in `pose` (:724)
    ffhq = ShiftVectors('ffhq', 15, 6.0, ranges=golden('kat8_shift.npz')['ranges_ffhq'])
    assert ffhq.roll_direction == -1
    moved = angles_shifted.clone()
    moved[:, 2] += 9.0
    _, pose_f, exp_f = evaluation_metrics(ffhq, rig.id_loss, params_shifted, params_target, moved, angles_target, imgs_shifted, imgs_source)
    want_pose, want_exp = _metrics_written_out(ffhq, params_shifted, params_target, moved, angles_target, 0)
    print('metrics, ffhq tables, roll moved by 9 degrees: pose %.6g (written out %.6g; %.6g before)' % (float(pose_f[0]), want_pose, float(pose[0])))
    assert abs(float(pose_f[0]) - want_pose) <= 1e-5 * want_pose and abs(float(exp_f[0]) - want_exp) <= 1e-5 * want_exp
    assert abs(float(pose_f[0]) - float(pose[0])) > 1.0


def test_new_steps_make_no_synchronising_torch_call(rig):
    """After two warm-up steps each (weight packs, the ShapeLoss camera, Adam's state, the generator's graph capture) one more
    PairedTrainer.step and one more step_real (with synthetic rows, draws made on the device) run under
    torch.cuda.set_sync_debug_mode('error').  As in tests/test_gpu_train_step.py this sees synchronisations made through torch only."""
    paired = rig.paired_trainer(rig.direction_matrix())
    real = rig.trainer(rig.direction_matrix(), LAMBDAS5)
    zt = rig.z_target
    for _ in range(2):
        paired.step(rig.ws, rig.source_img, rig.wt, rig.target_img)
        real.step_real(rig.ws, rig.source_img, zt, source_z_syn=rig.z_syn)
    torch.cuda.synchronize()
    probe = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                                   # the mode is honoured by this build of torch
        loss_p, dp = paired.step(rig.ws, rig.source_img, rig.wt, rig.target_img)
        loss_r, dr = real.step_real(rig.ws, rig.source_img, zt, source_z_syn=rig.z_syn)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for loss, d in ((loss_p, dp), (loss_r, dr)):
        assert loss.is_cuda and float(loss) == float(d['loss']) and float(loss) == float(loss)
    assert rig.G.saturated_pairs() == 0

"""The direction-learning steps of the reference's three training methods (synthetic; real / real_synthetic; paired), from latents
or frames to the updated direction matrix A, on this package's HIP heads -- DESIGN.md sections 4.20 and 4.22.  Counterparts, same
names and argument order:

  * ``shape_params``                        libs/utilities/generic.py:22-34 calculate_shapemodel for GAN-range images with
                                            libs/DECA/estimate_DECA.py:30-53 extract_DECA_params (the failed-row rule)
  * ``DirectionLosses.calculate_losses``    libs/utilities/utils_train.py:376-433
  * ``DirectionTrainer.step``               the loop body of libs/trainer.py:153-189 (Trainer.train, the synthetic method)
  * ``DirectionTrainer.step_real``          the loop body of libs/trainer.py:250-296 (Trainer.train_real: `real`, `real_synthetic`)
  * ``PairedLosses.calculate_losses_paired``  libs/utilities/utils_train.py:435-499
  * ``PairedTrainer.step``                  the loop body of libs/trainer.py:352-383 (Trainer.train_paired)
  * ``evaluation_metrics``, ``evaluate_pairs``  libs/utilities/utils_train.py:695-732 and the batch body of :756-768

    losses = DirectionLosses(flame, id_loss, lpips, shifts, {'lambda_shape': 1.0, 'lambda_mouth_shape': 1.0, 'lambda_eye_shape': 1.0,
                                                             'lambda_identity': 10.0, 'lambda_perceptual': 10.0})
    trainer = DirectionTrainer(G, A, det, fan, E, losses, truncation=0.7, trunc=trunc)
    loss, loss_dict = trainer.step(source_z, target_z)               # 0-d device tensors; to_host(loss_dict) for logging

Nothing in the step's own code synchronises with the host: the face boxes, the has_face mask, the drawn directions, the
ground-truth coefficients (shift.ShiftVectors.get_params_gt_reenacted) and every loss term stay device tensors, where the
reference reads int(target_indices[count]) once per row and calls .item() six times per step.  One head does wait: a no-grad
render through generic.generate_image is verified against the generator's fp16 range plan before it is handed back
(generic.VERIFY_RANGE; model.Generator.forward), which the no-grad renders of a step go through (the paired step has none).
The paired step's own arithmetic -- the 0..255 transform, the pixel-wise L1 and the latent L1 -- is pair_loss.py (DESIGN.md section
4.22).  The datasets, logging, checkpoints and wandb are not here.
"""
import torch

from . import deca as DECA
from . import face_detector as FD
from . import id_loss as ID
from . import pair_loss as PL
from .flame import ShapeLoss
from .generic import generate_image

LOSS_KEYS = ('loss_shape', 'loss_eye', 'loss_mouth', 'loss_identity', 'loss_perceptual', 'loss')
LAMBDAS = ('lambda_shape', 'lambda_mouth_shape', 'lambda_eye_shape', 'lambda_identity', 'lambda_perceptual')
PAIRED_LOSS_KEYS = ('loss_shape', 'loss_eye', 'loss_mouth', 'loss_identity', 'loss_perceptual', 'loss_pixel_wise', 'loss_w_reg', 'loss')
PAIRED_LAMBDAS = LAMBDAS + ('lambda_pixel_wise', 'lambda_w_reg')
FAILED_ANGLE = -180.0                           # estimate_DECA.py:48-51


def shape_params(det, fan, E, images, boxes=None, has_face=None):
    """generic.calculate_shapemodel(deca, images) for GAN-range images [B,3,H,W] as the trainer calls it:
    ({'pose' [B,6], 'alpha_exp' [B,50], 'alpha_shp' [B,100], 'cam' [B,3]}, angles [B,3] degrees).

    face_detector.detect_landmarks(input_range='gan') -> deca.crop_matrix -> deca.calculate_shapemodel, then the failed-row rule
    of extract_DECA_params: a row without a face gets zero pose, alpha_exp, alpha_shp and cam and angles of -180.  The rule is a
    select on the device by the has_face mask; such a row's box is replaced by the whole image in front of the crop, so the
    encoder sees finite numbers, and no gradient reaches its image.  `boxes` [B,4] ('kpt68' boxes [left, top, right, bottom]) and
    `has_face` [B] may be given (a caller with precomputed boxes): detection is then skipped, and has_face defaults to all
    True.  Gradient reaches `images` through the crop and the encoder only, as in deca.py; the boxes are decisions."""
    B, dev = images.shape[0], images.device
    if boxes is None:
        with torch.no_grad():
            _, boxes, found = FD.detect_landmarks(det, fan, images.detach(), input_range='gan')
        has_face = found if has_face is None else has_face
    boxes = torch.as_tensor(boxes, dtype=torch.float32).to(dev)
    if has_face is None:
        has_face = torch.ones(B, dtype=torch.bool, device=dev)
    has = torch.as_tensor(has_face).to(device=dev, dtype=torch.bool).view(-1, 1)
    if tuple(boxes.shape) != (B, 4) or has.shape[0] != B:
        raise ValueError('shape_params: expected [%d,4] boxes and [%d] has_face, got %s and %s'
                         % (B, B, tuple(boxes.shape), tuple(has.shape[:1])))
    whole = torch.zeros(4, dtype=torch.float32, device=dev)           # [0, 0, W, H] by fill launches: an upload, which `whole[2] = W`
    whole[2].fill_(float(images.shape[3]))                            # is too, would wait for the device
    whole[3].fill_(float(images.shape[2]))
    M = DECA.crop_matrix(torch.where(has, boxes, whole), images.shape[2:])
    params, angles = DECA.calculate_shapemodel(E, images, M)
    params = {k: torch.where(has, v, torch.zeros((), dtype=v.dtype, device=dev)) for k, v in params.items()}
    angles = torch.where(has, angles, torch.full((), FAILED_ANGLE, dtype=angles.dtype, device=dev))
    return params, angles


def to_host(loss_dict):
    """{key: float} of a loss_dict of 0-d device tensors with ONE device->host copy (the reference's six .item() calls)."""
    keys = list(loss_dict)
    if not keys:
        return {}
    values = torch.stack([loss_dict[k].detach().float() for k in keys]).cpu().tolist()
    return dict(zip(keys, values))


class DirectionLosses:
    """Utilities_train.calculate_losses on the HIP heads.  `flame` is a flame.FLAME (wrapped in a flame.ShapeLoss) or a ShapeLoss,
    `id_loss` an id_loss.IDLoss, `lpips` an lpips.LPIPS, `shifts` the shift.ShiftVectors of the run, `lambdas` a mapping with the
    reference's parameter names (lambda_shape, lambda_mouth_shape, lambda_eye_shape, lambda_identity, lambda_perceptual; a missing one
    is 0).  A head whose lambda is 0 may be None."""

    def __init__(self, flame, id_loss, lpips, shifts, lambdas, disentanglement_50=True):
        self.shape_loss = flame if (flame is None or isinstance(flame, ShapeLoss)) else ShapeLoss(flame)
        self.id_loss, self.lpips, self.shifts = id_loss, lpips, shifts
        unknown = set(lambdas) - set(LAMBDAS)
        if unknown:
            raise ValueError('DirectionLosses: unknown lambdas %s (known: %s)' % (sorted(unknown), ', '.join(LAMBDAS)))
        self.lambdas = {k: float(lambdas.get(k, 0.0)) for k in LAMBDAS}
        self.disentanglement_50 = bool(disentanglement_50)
        for lam, head, name in ((self.lambdas['lambda_shape'] > 0, self.shape_loss, 'flame'),
                                (self.lambdas['lambda_identity'] != 0, id_loss, 'id_loss'),
                                (self.lambdas['lambda_perceptual'] != 0, lpips, 'lpips')):
            if lam and head is None:
                raise ValueError('DirectionLosses: %s is None but its lambda is not 0' % name)

    def coefficients_gt(self, params_source, params_target, shift_vector, target_indices, angles_source):
        """The ground-truth set of utils_train.py:384-395: source identity, target pose and expression -- with disentanglement_50,
        one facial attribute of the target only in the second half of the batch (get_params_gt_reenacted)."""
        if self.disentanglement_50:
            gt = self.shifts.get_params_gt_reenacted(params_source, params_target, shift_vector, target_indices, angles_source)
        else:
            gt = {'pose': params_target['pose'], 'exp': params_target['alpha_exp']}
        gt['shape'] = params_source['alpha_shp']
        return gt

    def calculate_losses(self, params_source, angles_source, params_shifted, angles_shifted, params_target, angles_target, shift_vector,
                         target_indices, imgs_source, imgs_shifted):
        """(loss, loss_dict) as utils_train.py:376-433; loss_dict holds 0-d DEVICE tensors (detached) under the reference's keys,
        to_host(loss_dict) fetches them in one copy.  A term whose lambda is 0 is neither computed nor listed.  Both coefficient
        sets are decoded with cam = (8, 0, 0) by ShapeLoss itself: params_shifted['cam'] is not written to."""
        lam = self.lambdas
        loss_dict, loss = {}, None
        if lam['lambda_shape'] > 0:
            gt = self.coefficients_gt(params_source, params_target, shift_vector, target_indices, angles_source)
            reen = {'pose': params_shifted['pose'], 'shape': params_shifted['alpha_shp'], 'exp': params_shifted['alpha_exp']}
            loss, terms = self.shape_loss(gt, reen, lam['lambda_shape'], lam['lambda_mouth_shape'], lam['lambda_eye_shape'])
            loss_dict['loss_shape'] = terms['loss_shape'].detach()
            loss_dict['loss_eye'] = terms['loss_eye'].detach()
            loss_dict['loss_mouth'] = terms['loss_mouth'].detach()
        if lam['lambda_identity'] != 0:
            loss_identity = lam['lambda_identity'] * self.id_loss(imgs_shifted, imgs_source.detach())
            loss_dict['loss_identity'] = loss_identity.detach()
            loss = loss_identity if loss is None else loss + loss_identity
        if lam['lambda_perceptual'] != 0:
            loss_perceptual = lam['lambda_perceptual'] * self.lpips(imgs_shifted, imgs_source.detach())
            loss_dict['loss_perceptual'] = loss_perceptual.detach()
            loss = loss_perceptual if loss is None else loss + loss_perceptual
        if loss is None:
            raise ValueError('calculate_losses: every lambda is 0, there is nothing to minimise')
        loss_dict['loss'] = loss.detach()
        return loss, loss_dict


class DirectionTrainer:
    """The body of Trainer.train's loop (libs/trainer.py:153-189) for the direction matrix `A` (direction_matrix.DirectionMatrix).

    `G` is used as given: the trainer does not freeze it.  Only A is optimised (trainer.py:144), so a generator whose parameters
    all have requires_grad=False is the fast path -- its backward then computes dL/dlatent alone and skips every weight
    gradient.  `det`, `fan`, `E` are the face detector, the landmark network and the DECA encoder of
    shape_params; `losses` a DirectionLosses; `trunc` the truncation latent (default: G.mean_latent(4096), trainer.py:113);
    `optimizer` defaults to Adam(A.parameters(), lr, weight_decay=5e-4) (trainer.py:144)."""

    def __init__(self, G, A, det, fan, E, losses, truncation=0.7, trunc=None, optimizer=None, lr=1e-4):
        self.G, self.A, self.det, self.fan, self.E, self.losses = G, A, det, fan, E, losses
        self.truncation = truncation
        if trunc is None:
            with torch.no_grad():
                trunc = G.mean_latent(4096).detach().clone()
        self.trunc = trunc
        self.optimizer = torch.optim.Adam(A.parameters(), lr=lr, weight_decay=5e-4) if optimizer is None else optimizer

    def shape_params(self, images):
        return shape_params(self.det, self.fan, self.E, images)

    def step(self, source_z, target_z, input_is_latent=False, target_indices=None, u=None):
        """One optimisation step -> (loss, loss_dict).  source_z / target_z: [B,512] z codes, or -- input_is_latent=True -- W or
        W+ codes ([B,512] / [B,n_latent,512]: the synthetic leg of the `real` method).  target_indices [B/2] / u [B/2], the draws
        of make_shift_vector_50, may be given; by default they are drawn on the device."""
        G, losses = self.G, self.losses
        with torch.no_grad():
            imgs_source = generate_image(G, source_z, self.truncation, self.trunc, input_is_latent=input_is_latent)
            params_source, angles_source = self.shape_params(imgs_source)
            imgs_target = generate_image(G, target_z, self.truncation, self.trunc, input_is_latent=input_is_latent)
            params_target, angles_target = self.shape_params(imgs_target)
        if losses.disentanglement_50:
            shift_vector, target_indices = losses.shifts.make_shift_vector_50(params_source, params_target, angles_source, angles_target,
                                                                              target_indices=target_indices, u=u)
        else:
            target_indices = None
            shift_vector = losses.shifts.make_shift_vector(params_source, params_target, angles_source, angles_target)
        shift = self.A(shift_vector)
        imgs_shifted, _ = generate_image(G, source_z, self.truncation, self.trunc, shift_code=shift, input_is_latent=input_is_latent,
                                         return_latents=True)
        params_shifted, angles_shifted = self.shape_params(imgs_shifted)
        loss, loss_dict = losses.calculate_losses(params_source, angles_source, params_shifted, angles_shifted, params_target,
                                                  angles_target, shift_vector, target_indices, imgs_source, imgs_shifted)
        self.A.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.detach(), loss_dict

    def step_real(self, source_w, source_real_img, target_z, source_z_syn=None, target_indices=None, u=None):
        """One optimisation step of the `real` / `real_synthetic` methods (trainer.py:250-296) -> (loss, loss_dict).  source_w
        [B,n_latent,512]: the inverted W+ codes of the real frames source_real_img [B,3,256,256] (GAN range); target_z [rows,512]
        z codes, one per source row.  With source_z_syn [Bs,512] (`real_synthetic`, :259-266) Bs synthetic sources join the
        batch: their W codes (G.get_latent) repeated to W+ follow source_w, their renders follow the real frames, rows = B + Bs.
        The source FRAME stands where `step` has the source render: in shape_params and in the identity and LPIPS terms.  The
        synthetic rows are rendered without a graph: nothing A drives lies in front of them."""
        G, losses = self.G, self.losses
        with torch.no_grad():
            if source_z_syn is not None:
                source_w_syn = G.get_latent(source_z_syn).unsqueeze(1).repeat(1, G.n_latent, 1)                     # :262-263
                source_w = torch.cat((source_w, source_w_syn), dim=0)                                                # :264
                imgs_source = generate_image(G, source_w_syn, self.truncation, self.trunc, input_is_latent=True)     # :265
                source_real_img = torch.cat((source_real_img, imgs_source), dim=0)                                   # :266
            params_source, angles_source = self.shape_params(source_real_img)                                        # :268
            imgs_target = generate_image(G, target_z, self.truncation, self.trunc, input_is_latent=False)            # :274
            params_target, angles_target = self.shape_params(imgs_target)
        if losses.disentanglement_50:
            shift_vector, target_indices = losses.shifts.make_shift_vector_50(params_source, params_target, angles_source, angles_target,
                                                                              target_indices=target_indices, u=u)
        else:
            target_indices = None
            shift_vector = losses.shifts.make_shift_vector(params_source, params_target, angles_source, angles_target)
        shift = self.A(shift_vector)
        imgs_shifted, _ = generate_image(G, source_w, self.truncation, self.trunc, shift_code=shift, input_is_latent=True,
                                         return_latents=True)
        params_shifted, angles_shifted = self.shape_params(imgs_shifted)
        loss, loss_dict = losses.calculate_losses(params_source, angles_source, params_shifted, angles_shifted, params_target,
                                                  angles_target, shift_vector, target_indices, source_real_img, imgs_shifted)
        self.A.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.detach(), loss_dict


class PairedLosses:
    """Utilities_train.calculate_losses_paired (utils_train.py:435-499) on the HIP heads.  `flame`, `id_loss`, `lpips` as in
    DirectionLosses; `lambdas` a mapping with the reference's names (PAIRED_LAMBDAS; a missing one is 0).  A head whose lambda is 0 may
    be None.  What differs from calculate_losses: the ground-truth FLAME set is the TARGET's pose, expression and shape; identity is
    taken against the target frame; LPIPS and the pixel-wise L1 run on the 0..255 images (pair_loss.pixel_wise_255: both transforms,
    the L1 and its backward are one launch each way); the latent regulariser is L1Loss(shifted_latents, target_w)."""

    def __init__(self, flame, id_loss, lpips, lambdas):
        self.shape_loss = flame if (flame is None or isinstance(flame, ShapeLoss)) else ShapeLoss(flame)
        self.id_loss, self.lpips = id_loss, lpips
        unknown = set(lambdas) - set(PAIRED_LAMBDAS)
        if unknown:
            raise ValueError('PairedLosses: unknown lambdas %s (known: %s)' % (sorted(unknown), ', '.join(PAIRED_LAMBDAS)))
        self.lambdas = {k: float(lambdas.get(k, 0.0)) for k in PAIRED_LAMBDAS}
        lam = self.lambdas
        for live, head, name in ((lam['lambda_shape'] > 0, self.shape_loss, 'flame'), (lam['lambda_identity'] != 0, id_loss, 'id_loss'),
                                 (lam['lambda_perceptual'] != 0, lpips, 'lpips')):
            if live and head is None:
                raise ValueError('PairedLosses: %s is None but its lambda is not 0' % name)
        if not (lam['lambda_shape'] > 0 or any(lam[k] != 0 for k in PAIRED_LAMBDAS[3:])):
            raise ValueError('PairedLosses: every lambda is 0, there is nothing to minimise')

    def calculate_losses_paired(self, params_shifted, params_target, imgs_shifted, imgs_target, shifted_latents, target_w):
        """(loss, loss_dict) as utils_train.py:435-499; loss_dict holds 0-d DEVICE tensors (detached) under the reference's keys in
        its order of insertion (PAIRED_LOSS_KEYS), to_host(loss_dict) fetches them in one copy.  A term whose lambda is 0 is neither
        computed nor listed, and the 0..255 images are written only when LPIPS reads them.  Both coefficient sets are decoded with
        cam = (8, 0, 0) by ShapeLoss itself: neither params_target['cam'] nor params_shifted['cam'] is written to (the reference
        overwrites both in place, :446-448, :458-460)."""
        lam = self.lambdas
        loss_dict, loss = {}, None
        if lam['lambda_shape'] > 0:
            gt = {'pose': params_target['pose'], 'exp': params_target['alpha_exp'], 'shape': params_target['alpha_shp']}       # :444-449
            reen = {'pose': params_shifted['pose'], 'shape': params_shifted['alpha_shp'], 'exp': params_shifted['alpha_exp']}
            loss, terms = self.shape_loss(gt, reen, lam['lambda_shape'], lam['lambda_mouth_shape'], lam['lambda_eye_shape'])
            loss_dict['loss_shape'] = terms['loss_shape'].detach()
            if lam['lambda_eye_shape'] != 0:                 # (the one launch of ShapeLoss forms all three; a term scaled by 0 is not listed)
                loss_dict['loss_eye'] = terms['loss_eye'].detach()
            if lam['lambda_mouth_shape'] != 0:
                loss_dict['loss_mouth'] = terms['loss_mouth'].detach()
        if lam['lambda_identity'] != 0:
            loss_identity = lam['lambda_identity'] * self.id_loss(imgs_shifted, imgs_target.detach())
            loss_dict['loss_identity'] = loss_identity.detach()
            loss = loss_identity if loss is None else loss + loss_identity
        want_images = lam['lambda_perceptual'] != 0
        if want_images or lam['lambda_pixel_wise'] != 0:
            pixel_wise, x255, y255 = PL.pixel_wise_255(imgs_shifted, imgs_target.detach(), want_images)
        if want_images:
            loss_perceptual = lam['lambda_perceptual'] * self.lpips(x255, y255.detach())
            loss_dict['loss_perceptual'] = loss_perceptual.detach()
            loss = loss_perceptual if loss is None else loss + loss_perceptual
        if lam['lambda_pixel_wise'] != 0:
            loss_pixel_wise = lam['lambda_pixel_wise'] * pixel_wise
            loss_dict['loss_pixel_wise'] = loss_pixel_wise.detach()
            loss = loss_pixel_wise if loss is None else loss + loss_pixel_wise
        if lam['lambda_w_reg'] != 0:
            loss_w_reg = lam['lambda_w_reg'] * PL.l1_mean(shifted_latents, target_w.detach())
            loss_dict['loss_w_reg'] = loss_w_reg.detach()
            loss = loss_w_reg if loss is None else loss + loss_w_reg
        if loss is None:
            raise ValueError('calculate_losses_paired: every lambda is 0, there is nothing to minimise')
        loss_dict['loss'] = loss.detach()
        return loss, loss_dict


class PairedTrainer:
    """The body of Trainer.train_paired's loop (libs/trainer.py:352-383) for the direction matrix `A`: source and target are two
    real frames of one video, each with its inverted W+ code.  `shifts` is the shift.ShiftVectors of the run (the plain
    make_shift_vector); `losses` a PairedLosses; the rest as DirectionTrainer.  No frame is rendered without a graph here, so the
    step never waits for a verified render."""

    def __init__(self, G, A, det, fan, E, losses, shifts, truncation=0.7, trunc=None, optimizer=None, lr=1e-4):
        self.G, self.A, self.det, self.fan, self.E, self.losses, self.shifts = G, A, det, fan, E, losses, shifts
        self.truncation = truncation
        if trunc is None:
            with torch.no_grad():
                trunc = G.mean_latent(4096).detach().clone()
        self.trunc = trunc
        self.optimizer = torch.optim.Adam(A.parameters(), lr=lr, weight_decay=5e-4) if optimizer is None else optimizer

    def shape_params(self, images):
        return shape_params(self.det, self.fan, self.E, images)

    def step(self, source_w, source_img, target_w, target_img):
        """One optimisation step -> (loss, loss_dict).  source_w / target_w: [B,n_latent,512] W+ codes of the frames source_img /
        target_img [B,3,256,256] (GAN range)."""
        with torch.no_grad():
            params_source, angles_source = self.shape_params(source_img)                                             # :360
            params_target, angles_target = self.shape_params(target_img)                                             # :366
        shift_vector = self.shifts.make_shift_vector(params_source, params_target, angles_source, angles_target)    # :370
        shift = self.A(shift_vector)
        imgs_shifted, shifted_latents = generate_image(self.G, source_w, self.truncation, self.trunc, shift_code=shift,
                                                       input_is_latent=True, return_latents=True)                    # :372
        params_shifted, _ = self.shape_params(imgs_shifted)
        loss, loss_dict = self.losses.calculate_losses_paired(params_shifted, params_target, imgs_shifted, target_img, shifted_latents,
                                                              target_w)                                              # :377
        self.A.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.detach(), loss_dict


def _metric_ranges(shifts, device):
    """(lo [E+1], span [E+1]) float64 on the device: the (min, max - min) of the num_expressions expression coefficients, then the
    jaw's (utils_train.py:711-720); uploaded once per ShiftVectors and device."""
    cache = shifts.__dict__.setdefault('_metric_range_cache', {})
    if device not in cache:
        lo = [float(e['min_shift']) for e in shifts.directions_exp] + [float(shifts.min_jaw)]
        hi = [float(e['max_shift']) for e in shifts.directions_exp] + [float(shifts.max_jaw)]
        lo, hi = torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64)
        cache[device] = (lo.to(device), (hi - lo).to(device))
    return cache[device]


def expression_pose_errors(shifts, params_shifted, params_target, angles_shifted, angles_target):
    """(pose [B], exp_error [B]) of utils_train.py:709-725 for every row, in float64 like the reference's numpy scalars, returned
    as float32.  exp_error: mean over the num_expressions expression coefficients and the jaw of |norm(shifted) - norm(target)|,
    norm(v) = (v - min) / (max - min); pose: mean |difference| of yaw, pitch and roll -- roll counts whatever the dataset's
    direction table says (:724).  Runs on whatever device the tensors live on."""
    E = shifts.num_expressions
    lo, span = _metric_ranges(shifts, params_target['alpha_exp'].device)
    cols = lambda p: torch.cat([p['alpha_exp'][:, :E], p['pose'][:, 3:4]], 1).detach().double()
    gt, sh = (cols(params_target) - lo) / span, (cols(params_shifted) - lo) / span
    exp_error = (sh - gt).abs().mean(1)
    pose = (angles_shifted[:, :3].detach().double() - angles_target[:, :3].detach().double()).abs().sum(1) / 3
    return pose.float(), exp_error.float()


def evaluation_metrics(shifts, id_loss, params_shifted, params_target, angles_shifted, angles_target, imgs_shifted, imgs_source):
    """Utilities_train.extract_evaluation_metrics (utils_train.py:695-732) for every row of the batch ->
    (csim [B], pose [B], exp_error [B]) as device tensors; row 0 is what the reference returns as three host numbers.  csim is
    the row-wise dot product of id_loss's unit-norm embeddings of imgs_shifted and imgs_source (csim.mean() = 1 - id_loss(...)).
    Nothing here synchronises; fetch the three with one .cpu() where they are logged."""
    pose, exp_error = expression_pose_errors(shifts, params_shifted, params_target, angles_shifted, angles_target)
    with torch.no_grad():
        e_shifted, e_source = ID.embed(id_loss.facenet, imgs_shifted.detach(), imgs_source.detach(), True)
        csim = (e_shifted * e_source).sum(1)
    return csim, pose, exp_error


_PARTS = ('G', 'A', 'det', 'fan', 'E', 'shifts', 'id_loss', 'truncation', 'trunc')


def evaluate_pairs(trainer_or_parts, source_code, target_z, input_is_latent):
    """The batch body of Utilities_train.evaluate_model_reenactment (utils_train.py:756-768) under no_grad ->
    (csim [B], pose [B], exp_error [B]) device tensors.  `trainer_or_parts`: a DirectionTrainer, a PairedTrainer, or a mapping with
    the keys G, A, det, fan, E, shifts, id_loss, truncation, trunc.  source_code: z codes, or W / W+ codes with input_is_latent=True
    (the `real` methods); the target is always drawn from z (:759).  CSIM is taken between the reenacted and the SOURCE render."""
    if isinstance(trainer_or_parts, dict):
        missing = [k for k in _PARTS if k not in trainer_or_parts]
        if missing:
            raise ValueError('evaluate_pairs: the parts lack %s (needed: %s)' % (missing, ', '.join(_PARTS)))
        p = trainer_or_parts
    else:
        t = trainer_or_parts
        p = {'G': t.G, 'A': t.A, 'det': t.det, 'fan': t.fan, 'E': t.E, 'shifts': getattr(t, 'shifts', None) or t.losses.shifts,
             'id_loss': t.losses.id_loss, 'truncation': t.truncation, 'trunc': t.trunc}
    if p['id_loss'] is None:
        raise ValueError('evaluate_pairs: CSIM needs an id_loss head')
    G, shifts = p['G'], p['shifts']
    with torch.no_grad():
        imgs_source = generate_image(G, source_code, p['truncation'], p['trunc'], input_is_latent=input_is_latent)        # :756
        params_source, angles_source = shape_params(p['det'], p['fan'], p['E'], imgs_source)
        imgs_target = generate_image(G, target_z, p['truncation'], p['trunc'], input_is_latent=False)                     # :759
        params_target, angles_target = shape_params(p['det'], p['fan'], p['E'], imgs_target)
        shift_vector = shifts.make_shifts_interpolation(params_source, params_target, angles_source, angles_target)      # :762
        imgs_shifted = generate_image(G, source_code, p['truncation'], p['trunc'], shift_code=p['A'](shift_vector),
                                      input_is_latent=input_is_latent)                                                    # :764
        params_shifted, angles_shifted = shape_params(p['det'], p['fan'], p['E'], imgs_shifted)
        return evaluation_metrics(shifts, p['id_loss'], params_shifted, params_target, angles_shifted, angles_target, imgs_shifted,
                                  imgs_source)

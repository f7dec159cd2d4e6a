"""The direction-learning step of the synthetic training method, from latents to the updated direction matrix A, on this
package's HIP heads -- DESIGN.md section 4.20.  Counterparts, same names and argument order:

  * ``shape_params``                        libs/utilities/generic.py:22-34 calculate_shapemodel for GAN-range images with
                                            libs/DECA/estimate_DECA.py:30-53 extract_DECA_params (the failed-row rule)
  * ``DirectionLosses.calculate_losses``    libs/utilities/utils_train.py:376-433
  * ``DirectionTrainer.step``               the loop body of libs/trainer.py:153-189

    losses = DirectionLosses(flame, id_loss, lpips, shifts, {'lambda_shape': 1.0, 'lambda_mouth_shape': 1.0, 'lambda_eye_shape': 1.0,
                                                             'lambda_identity': 10.0, 'lambda_perceptual': 10.0})
    trainer = DirectionTrainer(G, A, det, fan, E, losses, truncation=0.7, trunc=trunc)
    loss, loss_dict = trainer.step(source_z, target_z)               # 0-d device tensors; to_host(loss_dict) for logging

Nothing in the step's own code synchronises with the host: the face boxes, the has_face mask, the drawn directions, the
ground-truth coefficients (shift.ShiftVectors.get_params_gt_reenacted) and every loss term stay device tensors, where the
reference reads int(target_indices[count]) once per row and calls .item() six times per step.  One head does wait: a no-grad
render through generic.generate_image is verified against the generator's fp16 range plan before it is handed back
(generic.VERIFY_RANGE; model.Generator.forward), which the two no-grad renders of a step go through.  The paired / real-image
losses (calculate_losses_paired, lambda_pixel_wise, lambda_w_reg), the datasets, logging, checkpoints and wandb are not here.
"""
import torch

from . import deca as DECA
from . import face_detector as FD
from .flame import ShapeLoss
from .generic import generate_image

LOSS_KEYS = ('loss_shape', 'loss_eye', 'loss_mouth', 'loss_identity', 'loss_perceptual', 'loss')
LAMBDAS = ('lambda_shape', 'lambda_mouth_shape', 'lambda_eye_shape', 'lambda_identity', 'lambda_perceptual')
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

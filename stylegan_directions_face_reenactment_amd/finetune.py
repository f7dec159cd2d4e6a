"""Generator fine-tuning on one source (PTI), the counterpart of libs/optimization.py:25-72 (`optimize_g`): same parameter
selection, optimiser and truncation.  The default loss is the L2 term alone (l2_loss_fn); PtiLoss is the reference's
100 * MSE + LPIPS(alex) on the HIP LPIPS (lpips.py), its target features cached once per source; PooledPtiLoss is the same loss on
the generator's output pooled to the crop's side, for the 512 and 1024 generators (pool_loss.py).  The step -- forward, backward through autograd.SynthesisFn, Adam -- can be captured once and
replayed as a hipGraph: at one source per step the eager step is bound by its host launches (~5 ms), the replay takes
3.4-3.8 ms (bench.py --config pti, scripts/pti_step_bench.py)."""
import torch

from . import _native as N
from . import functional as F_


def pti_parameters(generator, optimize_all=False):
    """optimization.py:31-40: convs[4..11] (pt_l2_lambda 100) or every parameter (pt_l2_lambda 1)."""
    if optimize_all:
        return list(generator.parameters()), 1
    return [p for i in range(11, 3, -1) for p in generator.convs[i].parameters()], 100


def l2_loss_fn(imgs_gen, real_imgs, pt_l2_lambda):
    """The L2 term of calc_loss (libs/criteria/l2_loss.py: mse) weighted as optimization.py does; stand-in default."""
    return pt_l2_lambda * torch.nn.functional.mse_loss(imgs_gen, real_imgs)


class PtiLoss:
    """The PTI loss of libs/criteria/PTI/base_coach.py:24-43 (calc_loss, use_ball_holder off): pt_l2_lambda * mse +
    pt_lpips_lambda * LPIPS(alex) (hyperparameters.py: pt_lpips_lambda = 1), callable as optimize_g's loss_fn.  The features of
    the fixed real image are computed once, here (before any capture); an eager call checks that it is handed the same image,
    unchanged (a captured replay cannot look, so do not write into real_imgs between replays)."""

    def __init__(self, lpips, real_imgs, pt_lpips_lambda=1.0):
        self.lpips = lpips
        self.pt_lpips_lambda = float(pt_lpips_lambda)
        self.real = real_imgs.detach()
        self.target = lpips.target(self.real)

    def _check(self, real_imgs):
        r = self.real
        if real_imgs.data_ptr() != r.data_ptr() or real_imgs.shape != r.shape or real_imgs.stride() != r.stride():
            raise RuntimeError('PtiLoss: called with a different real image than it was built for')
        if real_imgs._version != self.target.source_version:
            raise RuntimeError('PtiLoss: the real image was modified in place after its LPIPS features were cached')

    def __call__(self, imgs_gen, real_imgs, pt_l2_lambda):
        if not torch.cuda.is_current_stream_capturing():
            self._check(real_imgs)
        loss = torch.nn.functional.mse_loss(imgs_gen, real_imgs) * pt_l2_lambda
        return loss + self.lpips(imgs_gen, self.target) * self.pt_lpips_lambda


class PooledPtiLoss:
    """PtiLoss for a generator above 256^2: the image the loss sees is the one generic.generate_image hands out, the generator's
    output pooled to P x P (AdaptiveAvgPool2d((256,256)), generic.py:146-148): pt_l2_lambda * mse(pooled, real) + pt_lpips_lambda *
    LPIPS(pooled, real), pooled and mse from ONE walk over the generated image (pool_loss.PoolMse), whose backward puts both
    gradients back onto it in one launch.  The reference's optimize_g hands the loss the generator's own 1024^2 output beside the
    256^2 crop (optimization.py:50-58) and cannot run there.  PtiLoss's contract: real_imgs [B,3,P,P], its LPIPS features cached
    here, the same-image check in eager mode, callable as optimize_g's loss_fn."""

    def __init__(self, lpips, real_imgs, P=256, pt_lpips_lambda=1.0):
        if isinstance(P, bool) or not isinstance(P, int) or P < 1:
            raise ValueError('PooledPtiLoss: P must be a positive int, got %r' % (P,))
        if not torch.is_tensor(real_imgs) or real_imgs.dim() != 4 or tuple(real_imgs.shape[1:]) != (3, P, P):
            raise ValueError('PooledPtiLoss: the real images must be [B,3,%d,%d], got %s' % (
                P, P, tuple(real_imgs.shape) if torch.is_tensor(real_imgs) else type(real_imgs).__name__))
        self.lpips, self.P = lpips, P
        self.pt_lpips_lambda = float(pt_lpips_lambda)
        self.real = real_imgs.detach()
        self.target = lpips.target(self.real)

    def _check(self, real_imgs):
        r = self.real
        if real_imgs.data_ptr() != r.data_ptr() or real_imgs.shape != r.shape or real_imgs.stride() != r.stride():
            raise RuntimeError('PooledPtiLoss: called with a different real image than it was built for')
        if real_imgs._version != self.target.source_version:
            raise RuntimeError('PooledPtiLoss: the real image was modified in place after its LPIPS features were cached')

    def __call__(self, imgs_gen, real_imgs, pt_l2_lambda):
        from .pool_loss import PoolMse
        if not (imgs_gen.is_cuda and torch.cuda.is_current_stream_capturing()):      # (a host tensor is refused below, unlaunched)
            self._check(real_imgs)
        pooled, mse = PoolMse.apply(imgs_gen, self.real, self.P)
        return mse * pt_l2_lambda + self.lpips(pooled, self.target) * self.pt_lpips_lambda


class FusedAdam:
    """torch.optim.Adam(params, lr) as libs/optimization.py:41 builds it (default betas and eps, no weight decay) with the whole
    update in ONE launch (sgdfr_adam_f32) and the step count on the device: under a hipGraph torch's capturable multi-tensor Adam
    spends ~100 launches on the 24 tensors of a PTI step (per-parameter step-size tensors), a tenth of the step.  Interface: the
    three calls the step uses -- zero_grad(set_to_none), step(), and state in .state for inspection."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.params = [p for p in params]
        if not self.params or len(self.params) > N.MAX_ADAM_TENSORS:
            raise ValueError('FusedAdam takes 1..%d parameter tensors' % N.MAX_ADAM_TENSORS)
        for p in self.params:
            N.require_device(p)
            if not p.is_contiguous():
                raise ValueError('FusedAdam: parameters must be contiguous')
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        dev = self.params[0].device
        self.step_count = torch.zeros(1, device=dev, dtype=torch.float32)
        self.state = {p: {'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)} for p in self.params}

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self):
        live = [p for p in self.params if p.grad is not None]
        if not live:
            return
        self.step_count.add_(1.0)
        arr = (N.AdamTensor * len(live))()
        keep = []
        for i, p in enumerate(live):
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            N.require_device(g)
            st = self.state[p]
            keep.append(g)
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), p.numel()
        N.call('sgdfr_adam_f32', arr, len(live), N.ptr(self.step_count), self.lr, self.betas[0], self.betas[1], self.eps, N.stream())
        for p in live:          # the native launch wrote p behind autograd's back: bump the version counter the weight packs
            torch.autograd.graph.increment_version(p)       # (ModulatedConv2d.packed) and the saved-tensor checks watch -- no launch


class GraphedStep:
    """Captures `step_fn()` (a full training step on static tensors: forward, backward, optimizer.step of an optimiser built
    with capturable=True) after `warmup` eager calls on a side stream, then replays it.  Call it like step_fn; the returned
    tensor is the static output of the captured step."""

    def __init__(self, step_fn, warmup=3, clear_grads_of=()):
        """clear_grads_of: parameters whose .grad is set to None right before the capture, so that the captured backward WRITES their
        gradients (into buffers of the graph's pool) instead of adding to tensors left by the warm-up steps -- one in-place add per
        parameter tensor and step otherwise (the whole-network capture recipe of torch.cuda.graphs)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                step_fn()
        torch.cuda.current_stream().wait_stream(side)
        for p in clear_grads_of:
            p.grad = None
        self.graph = torch.cuda.CUDAGraph()
        with F_.capture_graph(self.graph):
            self.out = step_fn()          # recorded, not executed: the first replay is step warmup + 1
        self.steps_done = warmup

    def __call__(self):
        self.graph.replay()
        self.steps_done += 1
        return self.out


def optimize_g(generator, latent, real_imgs, trunc, opt_steps=200, lr=3e-3, optimize_all=False, loss_fn=None, truncation=0.7,
               graph=True, freeze_unused=False, fused_adam=True):
    """Fine-tunes `generator` in place so that G(latent) reproduces real_imgs (optimization.py:25-72).  `trunc` is the
    truncation latent (the reference draws generator.mean_latent(4096) itself); loss_fn(imgs_gen, real_imgs, pt_l2_lambda)
    -> scalar (default: the weighted L2 term).  freeze_unused=True stops producing gradients nobody reads (the reference
    leaves requires_grad on every parameter).  fused_adam: the one-launch Adam (FusedAdam; False = torch.optim.Adam as the reference
    builds it -- the same update to rounding).  Returns (generator, last loss tensor)."""
    params, pt_l2_lambda = pti_parameters(generator, optimize_all)
    loss_fn = loss_fn or l2_loss_fn
    saved = None
    if freeze_unused:
        ids = {id(p) for p in params}
        saved = [(p, p.requires_grad) for p in generator.parameters()]
        for p in generator.parameters():
            p.requires_grad_(id(p) in ids)
    generator.train()
    if fused_adam and len(params) <= N.MAX_ADAM_TENSORS and all(p.is_cuda and p.is_contiguous() for p in params):
        optimizer = FusedAdam(params, lr=lr)
    else:
        optimizer = torch.optim.Adam(params, lr=lr, capturable=bool(graph))
    latent, real_imgs = latent.detach(), real_imgs.detach()

    def step():
        imgs_gen, _ = generator([latent], input_is_latent=True, return_latents=False, truncation=truncation,
                                truncation_latent=trunc)
        loss = loss_fn(imgs_gen, real_imgs, pt_l2_lambda)
        optimizer.zero_grad(set_to_none=True)         # (optimization.py:66: the backward then writes fresh gradients, no zero + add pair)
        loss.backward()
        optimizer.step()
        return loss.detach()

    loss = None
    try:
        if graph and opt_steps > 4:
            runner = GraphedStep(step, warmup=3, clear_grads_of=list(generator.parameters()))
            for _ in range(opt_steps - runner.steps_done):
                loss = runner()
        else:
            for _ in range(opt_steps):
                loss = step()
    finally:
        if saved is not None:
            for p, rg in saved:
                p.requires_grad_(rg)
    return generator, loss

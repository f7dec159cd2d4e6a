"""Times the direction-learning step (train_step.DirectionTrainer.step) at the per-rank shape of BASELINE configs[4] -- B = 16,
256 x 256, channel multiplier 1, frozen generator, synthetic weights in every network -- on one GPU, and splits it per stage.

    python scripts/train_step_time.py [--out profiles/train_step_time.txt] [--batch 16] [--warmup 3] [--repeats 20]

Two measurements, each after `warmup` steps, `repeats` times, median with min .. max:
  * the whole step, DirectionTrainer.step as a caller runs it: device-event time, and host wall time around a step that ends in a
    device synchronise;
  * the same sequence written out stage by stage with a device event between the stages (the stages are the step's own calls, in
    its order): the two no-grad renders with their shape_params | shift vector + ground-truth coefficients | A and the grad
    render | shape_params with gradient | the three loss heads | backward | Adam.
The step's time is not the generator-only figure of the bench's trainer leg: it holds three renders, three passes of the face
detector, the landmark network and the coefficient encoder, and three loss heads beside the one generator backward.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stylegan_directions_face_reenactment_amd import synthetic as S                     # noqa: E402
from stylegan_directions_face_reenactment_amd import deca as D, face_detector as FD, landmarks as L   # noqa: E402
from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix   # noqa: E402
from stylegan_directions_face_reenactment_amd.flame import FLAME                        # noqa: E402
from stylegan_directions_face_reenactment_amd.generic import generate_image             # noqa: E402
from stylegan_directions_face_reenactment_amd.id_loss import IDLoss                     # noqa: E402
from stylegan_directions_face_reenactment_amd.lpips import LPIPS                        # noqa: E402
from stylegan_directions_face_reenactment_amd.model import Generator                    # noqa: E402
from stylegan_directions_face_reenactment_amd.shift import ShiftVectors                 # noqa: E402
from stylegan_directions_face_reenactment_amd.train_step import DirectionLosses, DirectionTrainer, shape_params, to_host   # noqa: E402

SEED = 14
STAGES = ('2 no-grad renders + shape_params', 'shift vector + GT coefficients', 'A + grad render', 'shape_params with gradient',
          'three loss heads', 'backward', 'Adam')
LAMBDAS = {'lambda_shape': 1.0, 'lambda_mouth_shape': 1.0, 'lambda_eye_shape': 1.0, 'lambda_identity': 10.0, 'lambda_perceptual': 10.0}


def load(module, state):
    module.load_state_dict(state)
    return module.cuda().eval()


def build():
    G = Generator(256, 512, 8, channel_multiplier=1)
    G.load_state_dict(S.synthetic_state_dict(G.state_dict(), seed=SEED))
    G = G.eval().cuda()
    for p in G.parameters():
        p.requires_grad_(False)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(SEED, num_layers=8))
    det, fan, E = load(FD.S3FD(), S.synthetic_s3fd_state(SEED)), load(L.FAN(4), S.synthetic_fan_state(SEED)), \
        load(D.ResnetEncoder(), S.synthetic_deca_encoder_state(SEED))
    flame, idl, lp = load(FLAME(), S.synthetic_flame_state(SEED)), load(IDLoss(), S.synthetic_arcface_state(SEED)), \
        load(LPIPS(), S.synthetic_lpips_state(SEED))
    ranges = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat8_shift.npz'))['ranges_voxceleb']
    shifts = ShiftVectors('voxceleb', 15, 6.0, ranges=ranges)
    losses = DirectionLosses(flame, idl, lp, shifts, LAMBDAS)
    trunc = S.counter_tensor(SEED, 'tst.trunc', (1, 512)).cuda()
    return DirectionTrainer(G, A.cuda(), det, fan, E, losses, truncation=0.7, trunc=trunc)


def staged_step(t, zs, zt, marks):
    """DirectionTrainer.step, its calls in its order, marks[i].record() between the stages."""
    G, losses, sp = t.G, t.losses, lambda x: shape_params(t.det, t.fan, t.E, x)
    marks[0].record()
    with torch.no_grad():
        imgs_source = generate_image(G, zs, t.truncation, t.trunc)
        params_source, angles_source = sp(imgs_source)
        imgs_target = generate_image(G, zt, t.truncation, t.trunc)
        params_target, angles_target = sp(imgs_target)
    marks[1].record()
    shift_vector, idx = losses.shifts.make_shift_vector_50(params_source, params_target, angles_source, angles_target)
    gt = losses.coefficients_gt(params_source, params_target, shift_vector, idx, angles_source)      # (timed here, built again below)
    marks[2].record()
    imgs_shifted, _ = generate_image(G, zs, t.truncation, t.trunc, shift_code=t.A(shift_vector), return_latents=True)
    marks[3].record()
    params_shifted, angles_shifted = sp(imgs_shifted)
    marks[4].record()
    loss, loss_dict = losses.calculate_losses(params_source, angles_source, params_shifted, angles_shifted, params_target, angles_target,
                                              shift_vector, idx, imgs_source, imgs_shifted)
    marks[5].record()
    t.A.zero_grad()
    loss.backward()
    marks[6].record()
    t.optimizer.step()
    marks[7].record()
    return loss_dict, gt


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d      # noqa: E731
    out, batch, warmup, repeats = arg('--out', ''), arg('--batch', 16), arg('--warmup', 3), arg('--repeats', 20)
    assert torch.cuda.is_available(), 'train_step_time.py needs a GPU'
    t = build()
    zs, zt = S.synthetic_z(SEED, batch, key='tst.zs').cuda(), S.synthetic_z(SEED, batch, key='tst.zt').cuda()
    lines = ['direction-learning step, B = %d, 256 x 256, cm = 1, frozen generator, synthetic weights (%s); %d warm-up steps, %d repeats'
             % (batch, torch.cuda.get_device_name(0), warmup, repeats)]
    for _ in range(warmup):
        loss, d = t.step(zs, zt)
    torch.cuda.synchronize()
    lines.append('terms after the warm-up: %s' % ', '.join('%s %.5g' % kv for kv in to_host(d).items()))
    dev, wall = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        t.step(zs, zt)
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    lines.append('%-36s median %8.3f ms   min %8.3f   max %8.3f' % (('DirectionTrainer.step, device events',) + stats(dev)))
    lines.append('%-36s median %8.3f ms   min %8.3f   max %8.3f' % (('DirectionTrainer.step, host wall',) + stats(wall)))
    per = [[] for _ in STAGES]
    total = []
    for i in range(warmup + repeats):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        torch.cuda.synchronize()
        staged_step(t, zs, zt, marks)
        torch.cuda.synchronize()
        if i >= warmup:
            for k in range(len(STAGES)):
                per[k].append(marks[k].elapsed_time(marks[k + 1]))
            total.append(marks[0].elapsed_time(marks[-1]))
    lines.append('the same sequence stage by stage (device events between the stages; a stage also holds the host time the device waited for):')
    for name, v in zip(STAGES, per):
        lines.append('  %-34s median %8.3f ms   min %8.3f   max %8.3f' % ((name,) + stats(v)))
    lines.append('  %-34s median %8.3f ms   min %8.3f   max %8.3f' % (('all stages',) + stats(total)))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

"""Times the paired direction-learning step (train_step.PairedTrainer.step) -- B = 16, 256 x 256, channel multiplier 1, frozen
generator, synthetic weights in every network -- on one GPU, splits it per stage, and times the kernels of csrc/pairloss.hip alone
against the stock-torch sequence they replace, in the same process.

    python scripts/paired_step_time.py [--out profiles/paired_step_time.txt] [--batch 16] [--warmup 3] [--repeats 20]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o pl -- python scripts/paired_step_time.py --only-kernels
    python scripts/paired_step_time.py --kernel-trace DIR/pl_kernel_trace.csv [--out profiles/paired_kernel_time.txt]      (no GPU)

Three measurements, each after `warmup` rounds, `repeats` times, median with min .. max:
  * the whole step as a caller runs it: device-event time, and host wall time around a step that ends in a device synchronise;
  * the same sequence stage by stage with a device event between the stages (the step's own calls, in its order): shape_params of
    the two frames | shift vector | A and the grad render | shape_params with gradient | the paired losses | backward | Adam;
  * the paired step's own arithmetic alone at [B,3,256,256] images and [B,14,512] latents, forward and backward (upstream gradients
    handed to torch.autograd.grad, the image gradient standing in for LPIPS's): pair_loss (one forward launch pair and one
    backward launch per term) against stock torch (transform x 2, two L1Loss, their autograd backward), alternating, in windows
    of 10 calls; and the forward pass of pixel_wise_255 alone with its achieved bytes per second -- 2 reads, plus 2 writes when the
    images are materialised -- on the same buffers (50 MB: resident in the 256 MiB Infinity Cache) and rotating over 8 input sets
    (403 MB of inputs, more than the cache holds), against the 6.29 TB/s HBM copy rate profiles/ records for this GPU.
A window of back-to-back calls is bounded by whichever is slower, the host's enqueue or the device; at these sizes that is the host.
The kernels' own durations come from a kernel trace of --only-kernels (the three legs above without the networks, separated by a
one-block marker call), which --kernel-trace turns into per-kernel medians and bytes per second.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import train_step_time as T                                                             # noqa: E402  (load, stats, SEED)
from stylegan_directions_face_reenactment_amd import synthetic as S                     # noqa: E402
from stylegan_directions_face_reenactment_amd import deca as D, face_detector as FD, landmarks as L   # noqa: E402
from stylegan_directions_face_reenactment_amd import pair_loss as PL                    # noqa: E402
from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix   # noqa: E402
from stylegan_directions_face_reenactment_amd.flame import FLAME                        # noqa: E402
from stylegan_directions_face_reenactment_amd.generic import generate_image             # noqa: E402
from stylegan_directions_face_reenactment_amd.id_loss import IDLoss                     # noqa: E402
from stylegan_directions_face_reenactment_amd.lpips import LPIPS                        # noqa: E402
from stylegan_directions_face_reenactment_amd.model import Generator                    # noqa: E402
from stylegan_directions_face_reenactment_amd.shift import ShiftVectors                 # noqa: E402
from stylegan_directions_face_reenactment_amd.train_step import PairedLosses, PairedTrainer, shape_params, to_host   # noqa: E402

SEED = T.SEED
STAGES = ('shape_params of the two frames', 'shift vector', 'A + grad render', 'shape_params with gradient', 'paired losses (5 heads)',
          'backward', 'Adam')
LAMBDAS = {'lambda_shape': 1.0, 'lambda_mouth_shape': 1.0, 'lambda_eye_shape': 1.0, 'lambda_identity': 10.0, 'lambda_perceptual': 10.0,
           'lambda_pixel_wise': 0.01, 'lambda_w_reg': 0.1}
COPY_RATE = 6.29e12                                                                     # bytes/s: the float4 copy of profiles/*_pmc.md
WINDOW = 10


def build():
    G = Generator(256, 512, 8, channel_multiplier=1)
    G.load_state_dict(S.synthetic_state_dict(G.state_dict(), seed=SEED))
    G = G.eval().cuda()
    for p in G.parameters():
        p.requires_grad_(False)
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(SEED, num_layers=8))
    det, fan, E = T.load(FD.S3FD(), S.synthetic_s3fd_state(SEED)), T.load(L.FAN(4), S.synthetic_fan_state(SEED)), \
        T.load(D.ResnetEncoder(), S.synthetic_deca_encoder_state(SEED))
    flame, idl, lp = T.load(FLAME(), S.synthetic_flame_state(SEED)), T.load(IDLoss(), S.synthetic_arcface_state(SEED)), \
        T.load(LPIPS(), S.synthetic_lpips_state(SEED))
    ranges = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat8_shift.npz'))['ranges_voxceleb']
    shifts = ShiftVectors('voxceleb', 15, 6.0, ranges=ranges)
    trunc = S.counter_tensor(SEED, 'pst.trunc', (1, 512)).cuda()
    return PairedTrainer(G, A.cuda(), det, fan, E, PairedLosses(flame, idl, lp, LAMBDAS), shifts, truncation=0.7, trunc=trunc)


def staged_step(t, ws, source_img, wt, target_img, marks):
    """PairedTrainer.step, its calls in its order, marks[i].record() between the stages."""
    sp = lambda x: shape_params(t.det, t.fan, t.E, x)                                   # noqa: E731
    marks[0].record()
    with torch.no_grad():
        params_source, angles_source = sp(source_img)
        params_target, angles_target = sp(target_img)
    marks[1].record()
    shift_vector = t.shifts.make_shift_vector(params_source, params_target, angles_source, angles_target)
    marks[2].record()
    imgs_shifted, latents = generate_image(t.G, ws, t.truncation, t.trunc, shift_code=t.A(shift_vector), input_is_latent=True,
                                           return_latents=True)
    marks[3].record()
    params_shifted, _ = sp(imgs_shifted)
    marks[4].record()
    loss, loss_dict = t.losses.calculate_losses_paired(params_shifted, params_target, imgs_shifted, target_img, latents, wt)
    marks[5].record()
    t.A.zero_grad()
    loss.backward()
    marks[6].record()
    t.optimizer.step()
    marks[7].record()
    return loss_dict


def stock_255(image):
    return image.clone().clamp(min=-1, max=1).add(1).div(2 + 1e-5).mul(255.0)


def hip_terms(x, y, lat, tw, c, g):
    pw, x255, _ = PL.pixel_wise_255(x, y, True)
    return torch.autograd.grad((pw, x255, PL.l1_mean(lat, tw)), (x, lat), (g, c, g))


def stock_terms(x, y, lat, tw, c, g):
    x255, y255 = stock_255(x), stock_255(y)
    l1 = torch.nn.L1Loss()
    return torch.autograd.grad((l1(y255.detach(), x255), x255, l1(lat, tw)), (x, lat), (g, c, g))


def window(fn, calls=WINDOW):
    """ms per call of `calls` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def line(name, v, width=36, extra=''):
    return '%-*s median %8.3f ms   min %8.3f   max %8.3f%s' % ((width, name) + T.stats(v) + (extra,))


def kernel_legs(batch, n_latent, warmup, repeats):
    """--only-kernels: pixel_wise_255 forward without, then with, the images (rotating inputs), then the terms forward + backward;
    a one-block l1_mean call marks each boundary in the kernel trace."""
    gen = torch.Generator(device='cuda').manual_seed(SEED)
    rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)                    # noqa: E731
    sets = [(0.8 * rnd(batch, 3, 256, 256), 0.8 * rnd(batch, 3, 256, 256)) for _ in range(8)]
    x, y, c = sets[0][0].clone().requires_grad_(True), sets[0][1], rnd(batch, 3, 256, 256)
    lat, tw, g = rnd(batch, n_latent, 512).requires_grad_(True), rnd(batch, n_latent, 512), torch.tensor(0.37, device='cuda')
    mark = torch.zeros(7, device='cuda')
    with torch.no_grad():
        for want in (False, True):
            for k in range(warmup + repeats):
                PL.pixel_wise_255(*sets[k % 8], want)
            PL.l1_mean(mark, mark)
    for k in range(warmup + repeats):
        hip_terms(x, y, lat, tw, c, g)
    torch.cuda.synchronize()


def kernel_table(path, batch, n_latent, repeats):
    """--kernel-trace: medians of the last `repeats` dispatches per kernel and leg, from rocprofv3's *_kernel_trace.csv."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    rows = [(r['Kernel_Name'].replace(' ', ''), int(r.get('Grid_Size') or r['Grid_Size_X']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3) for r in rows
            if 'pairloss' in r['Kernel_Name']]
    legs, skip = [[]], False
    for name, grid, us in rows:
        if skip:                                                                             # the marker's finish launch
            skip = False
        elif 'forward_kernel<0' in name and grid == 256:
            legs.append([])
            skip = True
        else:
            legs[-1].append((name, us))
    assert len(legs) == 3, 'expected three legs, found %d' % len(legs)
    img, lat = batch * 3 * 256 * 256 * 4, batch * n_latent * 512 * 4
    med = lambda leg, key: T.stats([us for name, us in leg if key in name][-repeats:])       # noqa: E731
    lines = ['kernels of csrc/pairloss.hip, durations from a kernel trace of their own (us, median min max of the last %d dispatches); '
             '[%d,3,256,256] images = %.1f MB, [%d,%d,512] latents = %.2f MB per array; bytes/s against the %.2f TB/s copy rate'
             % (repeats, batch, img / 1e6, batch, n_latent, lat / 1e6, COPY_RATE / 1e12)]

    def row(what, leg, key, nbytes):
        m = med(leg, key)
        rate = nbytes / (m[0] * 1e-6) if nbytes else 0.0
        lines.append('  %-66s %7.2f %7.2f %7.2f%s' % ((what,) + m + (('   %.2f TB/s = %.2f of the copy rate' % (rate / 1e12, rate / COPY_RATE)) if nbytes else '',)))
    row('forward range255, 2 reads (rotating inputs)', legs[0], 'forward_kernel<1', 2 * img)
    row('forward range255, 2 reads + 2 writes (rotating inputs)', legs[1], 'forward_kernel<1', 4 * img)
    row('finish (sums 768 partials)', legs[1], 'finish_kernel', 0)
    row('in the terms: forward range255, 2 reads + 2 writes (same buffers)', legs[2], 'forward_kernel<1', 4 * img)
    row('in the terms: backward range255, 3 reads + 1 write', legs[2], 'backward_kernel<1', 4 * img)
    row('in the terms: forward plain on the latents, 2 reads', legs[2], 'forward_kernel<0', 2 * lat)
    row('in the terms: backward plain on the latents, 2 reads + 1 write', legs[2], 'backward_kernel<0', 3 * lat)
    total = sum(med(legs[2], k)[0] for k in ('forward_kernel<1', 'backward_kernel<1', 'forward_kernel<0', 'backward_kernel<0')) + 2 * med(legs[2], 'finish_kernel')[0]
    lines.append('  the six launches of the terms, forward + backward: %.2f us of kernel time' % total)
    return lines


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d      # noqa: E731
    out, batch, warmup, repeats = arg('--out', ''), arg('--batch', 16), arg('--warmup', 3), arg('--repeats', 20)
    if '--kernel-trace' in sys.argv:
        text = '\n'.join(kernel_table(arg('--kernel-trace', ''), batch, 14, repeats))
        print(text)
        if out:
            with open(out, 'w') as f:
                f.write(text + '\n')
        return
    assert torch.cuda.is_available(), 'paired_step_time.py needs a GPU'
    if '--only-kernels' in sys.argv:
        return kernel_legs(batch, 14, warmup, repeats)
    t = build()
    n_latent = t.G.n_latent
    ws, wt = (S.synthetic_latents(SEED, batch, n_latent=n_latent, key=k).cuda() for k in ('pst.ws', 'pst.wt'))
    with torch.no_grad():       # the frames: renders of codes next to the ones handed over, as an inverted frame is next to its inversion
        source_img, target_img = (generate_image(t.G, w + 0.25 * S.synthetic_latents(SEED, batch, n_latent=n_latent, key=k).cuda(), 0.7,
                                                 t.trunc, input_is_latent=True).clone() for w, k in ((ws, 'pst.ds'), (wt, 'pst.dt')))
    lines = ['paired direction-learning step, B = %d, 256 x 256, cm = 1, frozen generator, synthetic weights (%s); %d warm-up steps, %d repeats'
             % (batch, torch.cuda.get_device_name(0), warmup, repeats)]
    for _ in range(warmup):
        loss, d = t.step(ws, source_img, wt, target_img)
    torch.cuda.synchronize()
    lines.append('terms after the warm-up: %s' % ', '.join('%s %.5g' % kv for kv in to_host(d).items()))
    dev, wall = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        t.step(ws, source_img, wt, target_img)
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    lines.append(line('PairedTrainer.step, device events', dev))
    lines.append(line('PairedTrainer.step, host wall', wall))
    per, total = [[] for _ in STAGES], []
    for i in range(warmup + repeats):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        torch.cuda.synchronize()
        staged_step(t, ws, source_img, wt, target_img, marks)
        torch.cuda.synchronize()
        if i >= warmup:
            for k in range(len(STAGES)):
                per[k].append(marks[k].elapsed_time(marks[k + 1]))
            total.append(marks[0].elapsed_time(marks[-1]))
    lines.append('the same sequence stage by stage (device events between the stages; a stage also holds the host time the device waited for):')
    for name, v in zip(STAGES, per):
        lines.append('  ' + line(name, v, 34))
    lines.append('  ' + line('all stages', total, 34))

    # ---- the paired step's own arithmetic alone, against the stock sequence, alternating in one loop
    gen = torch.Generator(device='cuda').manual_seed(SEED)
    rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)                    # noqa: E731
    x, y, c = (0.8 * rnd(batch, 3, 256, 256)).requires_grad_(True), 0.8 * rnd(batch, 3, 256, 256), rnd(batch, 3, 256, 256)
    lat, tw, g = rnd(batch, n_latent, 512).requires_grad_(True), rnd(batch, n_latent, 512), torch.tensor(0.37, device='cuda')
    hip, stock = [], []
    for i in range(warmup + repeats):
        a = window(lambda: hip_terms(x, y, lat, tw, c, g))
        b = window(lambda: stock_terms(x, y, lat, tw, c, g))
        if i >= warmup:
            hip.append(a)
            stock.append(b)
    lines.append('the transform x 2, the pixel-wise L1 and the latent L1, forward + backward, [%d,3,256,256] and [%d,%d,512], per call (windows of %d):'
                 % (batch, batch, n_latent, WINDOW))
    lines.append('  ' + line('pair_loss (HIP: 4 + 2 launches)', hip, 34))
    lines.append('  ' + line('stock torch ops with autograd', stock, 34))
    lines.append('  stock / HIP, medians: %.2f' % (T.stats(stock)[0] / T.stats(hip)[0]))
    nbytes = x.numel() * 4
    sets = [(0.8 * rnd(batch, 3, 256, 256), 0.8 * rnd(batch, 3, 256, 256)) for _ in range(8)]
    lines.append('pixel_wise_255 forward alone (no graph), %.1f MB per array, per call (windows of %d); bytes/s against the %.2f TB/s copy rate:'
                 % (nbytes / 1e6, 8 * WINDOW, COPY_RATE / 1e12))
    with torch.no_grad():
        for want, moved in ((False, 2), (True, 4)):
            for name, pick in (('the same buffers (cache-resident)', lambda k: (x, y)), ('rotating over 8 input sets', lambda k: sets[k % 8])):
                turn, v = [0], []

                def call():
                    PL.pixel_wise_255(*pick(turn[0]), want)
                    turn[0] += 1
                for i in range(warmup + repeats):
                    ms = window(call, 8 * WINDOW)
                    if i >= warmup:
                        v.append(ms)
                rate = moved * nbytes / (T.stats(v)[0] * 1e-3)
                lines.append('  ' + line('%s, %s' % ('2 reads + 2 writes' if want else '2 reads', name), v, 54,
                                         '   %.2f TB/s = %.2f of the copy rate' % (rate / 1e12, rate / COPY_RATE)))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

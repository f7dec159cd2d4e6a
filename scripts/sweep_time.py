"""Times the direction sweep (sweep.DirectionSweep.run, csrc/sweep.hip) on one GPU.  Recorded, not asserted: nothing earlier to compare with.

    python scripts/sweep_time.py [--out profiles/sweep_time.txt]

(a) the whole sweep: one 256^2 source (synthetic weights, cm = 1), 15 directions, shifts_count = 10, want = images + frames, against the
    written-out B=1 loop of run_facial_editing.py:144-207: per row a host-built one_hot vector and its upload, A(vector),
    generic.generate_image (this repository's, unchanged by the sweep: verified forwards), tensor_to_image-style uint8 conversion on the
    device.  The loop takes its ladder values from the sweep's own host records, so it is spared get_direction_info's per-direction
    host round trips.  Host clock around work that ends in a device synchronise; both warmed; the two alternate.
(b) the frames kernel: sgdfr_sweep_frames_f32 at R = 32, f = 4, P = 256 (403 MB read) against the stock sequence it replaces,
    adaptive_avg_pool2d -> grid_frames_uint8 / images_to_uint8; device events, 10 warm-up and 50 timed calls, alternating; bytes the
    algorithm needs (input once + outputs + the source panel) over the time, beside the 6.29 TB/s HBM copy rate of profiles/r06_i_pmc.md.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

COPY_RATE = 6.29e12


def event_ms(fn, warm, steps):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit('sweep_time.py needs a GPU: a CPU run gives no time')
    from stylegan_directions_face_reenactment_amd import synthetic as S
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.model import Generator
    from stylegan_directions_face_reenactment_amd.reenact import grid_frames_uint8, images_to_uint8
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    from stylegan_directions_face_reenactment_amd.sweep import DirectionSweep, pool_frames
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('direction sweep on %s' % torch.cuda.get_device_name(0))
    # ---------------------------------------------------------------- (a)
    G = Generator(256, 512, 8, channel_multiplier=1)
    G.load_state_dict(S.synthetic_state_dict(G.state_dict(), seed=7))
    G = G.eval().cuda()
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(5))
    A = A.cuda()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat8_shift.npz'))
    sv = ShiftVectors('voxceleb', 15, 6, ranges=g['ranges_voxceleb'])
    ang = torch.tensor([[4.0, -3.0, 2.0]]).cuda()
    # a source inside the dataset's ranges: every ladder has about 21 rows, as a real face's has
    mid = g['ranges_voxceleb'].mean(1)
    pose = torch.zeros(1, 6)
    pose[0, 3] = float(mid[3])
    params = {'pose': pose.cuda(), 'alpha_exp': torch.tensor(mid[4:54], dtype=torch.float32).view(1, 50).cuda()}
    w = S.synthetic_latents(7, 1, n_latent=G.n_latent).cuda()
    trunc = S.counter_tensor(7, 'trunc', (1, 512)).cuda()
    src = generate_image(G, w, 0.7, trunc, input_is_latent=True)
    sw = DirectionSweep(G, A, sv, 0.7, trunc, True, 8, batch=32)
    dirs = list(range(15))

    def batched():
        res = sw.run(w, dirs, params, ang, input_is_latent=True, shifts_count=10, source_img=src, want=('images', 'frames'))
        torch.cuda.synchronize()
        return res

    res = batched()
    rows = res.rows.cpu()
    total = rows.shape[0]

    def loop():
        frames = []
        with torch.no_grad():
            for r in range(total):
                k = int(rows[r].abs().argmax())
                vec = torch.zeros(15)
                vec[k] = float(rows[r, k])                              # one_hot on the host
                img = generate_image(G, w, 0.7, trunc, True, 8, shift_code=A(vec.cuda()), input_is_latent=True)
                frames.append(grid_frames_uint8([src, img]))
        torch.cuda.synchronize()
        return frames

    loop()
    batched()
    tb, tl = [], []
    for _ in range(3):
        t0 = time.perf_counter(); batched(); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); loop(); tl.append(time.perf_counter() - t0)
    say('(a) one 256^2 source, 15 directions, shifts_count 10: %d rows, lengths %s' % (total, [s.stop - s.start for s in res.slices]))
    say('    DirectionSweep.run (batch 32, images + 2-panel frames)  %8.1f ms  %7.1f frames/s   (runs: %s ms)'
        % (1e3 * min(tb), total / min(tb), ' '.join('%.1f' % (1e3 * t) for t in tb)))
    say('    B=1 loop (one_hot upload, A, generate_image, frame)     %8.1f ms  %7.1f frames/s   (runs: %s ms)'
        % (1e3 * min(tl), total / min(tl), ' '.join('%.1f' % (1e3 * t) for t in tl)))
    say('    ratio %.2fx' % (min(tl) / min(tb)))
    del res
    # ---------------------------------------------------------------- (b)
    R_, P, f = 32, 256, 4
    x = torch.empty(R_, 3, P * f, P * f, device='cuda').uniform_(-1.2, 1.2)
    srcp = torch.empty(1, 3, P, P, device='cuda').uniform_(-1.2, 1.2)
    flags = torch.zeros(R_, dtype=torch.int32, device='cuda')
    read = x.numel() * 4
    cases = (
        ('frames (2 panels)', lambda: pool_frames(x, P, None, srcp, ('frames',)),
         lambda: grid_frames_uint8([srcp, torch.nn.functional.adaptive_avg_pool2d(x, (P, P))]), read + R_ * P * 2 * P * 3 + R_ * 3 * P * P * 4),
        ('frames (1 panel)', lambda: pool_frames(x, P, None, None, ('frames',)),
         lambda: images_to_uint8(torch.nn.functional.adaptive_avg_pool2d(x, (P, P))), read + R_ * P * P * 3),
        ('images', lambda: pool_frames(x, P, None, None, ('images',)),
         lambda: torch.nn.functional.adaptive_avg_pool2d(x, (P, P)), read + R_ * 3 * P * P * 4),
        ('images + bordered + frames (2 panels)', lambda: pool_frames(x, P, flags, srcp, ('images', 'bordered', 'frames')),
         None, read + 2 * R_ * 3 * P * P * 4 + R_ * P * 2 * P * 3 + R_ * 3 * P * P * 4),
    )
    say('(b) sgdfr_sweep_frames_f32, x [%d,3,%d,%d] = %.0f MB; GB/s = bytes the kernel needs / time; HBM copy rate %.2f TB/s' % (R_, P * f, P * f, read / 1e6, COPY_RATE / 1e12))
    for name, mine, stock, nbytes in cases:
        tm = event_ms(mine, 10, 50)
        ts = event_ms(stock, 10, 50) if stock is not None else None
        tm2 = event_ms(mine, 2, 50)
        tm = min(tm, tm2)
        say('    %-40s kernel %7.3f ms = %6.0f GB/s = %.2f of the copy rate%s'
            % (name, tm, nbytes / tm / 1e6, nbytes / (tm * 1e-3) / COPY_RATE,
               '' if ts is None else '; stock sequence %7.3f ms (x%.2f)' % (ts, ts / tm)))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

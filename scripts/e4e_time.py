"""Times the e4e W+ encoder on one GPU: the HIP path (encoder.encode, csrc/e4e.hip) against the module's own MIOpen plan (`enc(x)`
under no_grad) with the same weights, alternated call by call in the same process: R = 256 at B = 1 and B = 32, device events,
warm-up calls first, several repetitions of a block of timed calls (the median block is reported beside the fastest and slowest).
Synthetic weights throughout.  The implied rate uses 118 GFLOP per image against the 157.3 TFLOP/s exact-f32 MFMA peak.

    python scripts/e4e_time.py [--out profiles/e4e_time.txt] [--steps 10] [--reps 5] [--rows 1,32]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260929
PEAK_TF = 157.3
GFLOP_PER_IMAGE = 118.0


def main():
    import torch
    from stylegan_directions_face_reenactment_amd import encoder as E, synthetic as S
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    out = arg('--out', None)
    steps, reps, warm = int(arg('--steps', 10)), int(arg('--reps', 5)), int(arg('--warmup', 3))
    row_list = [int(v) for v in arg('--rows', '1,32').split(',')]
    enc = E.Encoder4Editing(50, 'ir_se', 256).eval()
    enc.load_state_dict(S.synthetic_encoder_state(enc.state_dict(), seed=SEED), strict=True)
    enc = enc.cuda()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if out:
            with open(out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    def event_ms(fns):
        """Per function the per-call device-event time of each repetition, the functions alternated call by call."""
        for _ in range(warm):
            for fn in fns:
                fn()
        blocks = [[] for _ in fns]
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
        for _ in range(reps):
            tot = [0.0] * len(fns)
            for _ in range(steps):
                for (a, b), fn in zip(ev, fns):
                    a.record()
                    fn()
                    b.record()
                torch.cuda.synchronize()
                for i, (a, b) in enumerate(ev):
                    tot[i] += a.elapsed_time(b)
            for i, t in enumerate(tot):
                blocks[i].append(t / steps)
        return [sorted(b) for b in blocks]

    say('e4e encoder, 256x256 images, synthetic weights (%s), %d warm-up calls, %d repetitions of %d timed calls' % (
        torch.cuda.get_device_name(0), warm, reps, steps))
    with torch.no_grad():
        for B in row_list:
            x = S.counter_tensor(SEED, 'e4e.time.x%d' % B, (B, 3, 256, 256), 0.0, 0.5).clamp_(-1, 1).cuda()
            a, b = E.encode(enc, x), enc(x)
            say('B=%d W+: HIP vs MIOpen plan max |diff| %.2e (max |w| %.2f)' % (B, float((a - b).abs().max()), float(b.abs().max())))
            hip, stock = event_ms([lambda: E.encode(enc, x), lambda: enc(x)])
            h, s = hip[len(hip) // 2], stock[len(stock) // 2]
            tf = lambda ms: B * GFLOP_PER_IMAGE / ms
            say('B=%-2d HIP %9.3f ms (%.3f .. %.3f)  MIOpen plan %9.3f ms (%.3f .. %.3f)  HIP/MIOpen %.2f   HIP %.1f TFLOP/s = %.3f of the '
                '%.1f TF exact-f32 MFMA peak, MIOpen plan %.1f TFLOP/s   %.0f and %.0f images/s' % (
                    B, h, hip[0], hip[-1], s, stock[0], stock[-1], h / s, tf(h), tf(h) / PEAK_TF, PEAK_TF, tf(s), B / h * 1e3, B / s * 1e3))


if __name__ == '__main__':
    main()

"""Times flip_input and the 3D landmark type on one GPU: the 2D call, 2D + flip and the 3D call of landmarks.py, and the depth
network alone (landmarks.ResNetDepth, csrc/fandepth.hip) against the stock fp32 ResNetDepth with the same weights
(tests/fan3d_restatement.py's unfolded `depth_network` on PyTorch-ROCm: MIOpen convs, eval BatchNorm, torch.cat in front), the two
alternated call by call in the same process: rows 1, 16 and 32 of 256x256 images, device events, 10 warm-up and 50 timed calls.
Synthetic weights throughout.

    python scripts/fan3d_time.py [--out profiles/fan3d_time.txt] [--steps 50] [--rows 1,16,32]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEED = 21
PEAK_TF = 157.3


def depth_flops():
    """Useful FLOPs per row of ResNetDepth, from the layer shapes."""
    f = 2 * 128 * 128 * 64 * 71 * 49
    cin, h = 64, 64
    for s, (p, n) in enumerate(zip((64, 128, 256, 512), (3, 8, 36, 3))):
        for k in range(n):
            stride = 2 if (k == 0 and s > 0) else 1
            ho = h // stride
            f += 2 * h * h * cin * p + 2 * ho * ho * 9 * p * p + 2 * ho * ho * p * 4 * p
            if k == 0:
                f += 2 * ho * ho * cin * 4 * p
            cin, h = 4 * p, ho
    return f + 2 * 2048 * 68


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    import torch
    from stylegan_directions_face_reenactment_amd import landmarks as L, synthetic as S
    import fan3d_restatement as R3
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 50
    row_list = [int(v) for v in sys.argv[sys.argv.index('--rows') + 1].split(',')] if '--rows' in sys.argv else [1, 16, 32]
    fan = L.FAN(4)
    fan.load_state_dict(S.synthetic_fan_state(SEED))
    fan = fan.cuda().eval()
    sd = S.synthetic_fan_depth_state(SEED)
    net = L.ResNetDepth()
    net.load_state_dict(sd)
    net = net.cuda().eval()
    sdc = {k: v.cuda() for k, v in sd.items()}
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if out:
            with open(out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    def event_ms(fns, n, warm=10):
        """Device-event time per call of each function, the functions alternated call by call."""
        for _ in range(warm):
            for fn in fns:
                fn()
        tot = [0.0] * len(fns)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
        for _ in range(n):
            for (a, b), fn in zip(ev, fns):
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(ev):
                tot[i] += a.elapsed_time(b)
        return [t / n for t in tot]

    fl = depth_flops()
    say('flip_input and the 3D landmark type, 256x256 images, synthetic weights (%s), %d timed calls, eager' % (torch.cuda.get_device_name(0), steps))
    say('depth network: %.2f GFLOP per row by the layer shapes' % (fl / 1e9))
    with torch.no_grad():
        for B in row_list:
            x = S.counter_tensor(SEED, 'f3t.x%d' % B, (B, 3, 256, 256), 127.5, 60.0).clamp(0, 255).cuda()
            fd = torch.tensor([[52.0, 40.0, 204.0, 222.0]]).repeat(B, 1).cuda()
            crop = L.crop(x, fd)
            _, pts, _ = L.get_landmarks(fan, x, fd)
            maps = L.draw(pts)
            a, b = L.depth_network(net, crop, maps), R3.depth_network(sdc, crop, maps)['depth']
            say('B=%d depths: HIP vs stock max |diff| %.2e (max |depth| %.2f)' % (B, float((a - b).abs().max()), float(b.abs().max())))
            t2, tf_, t3 = event_ms([lambda: L.get_landmarks(fan, x, fd), lambda: L.get_landmarks(fan, x, fd, flip_input=True),
                                    lambda: L.get_landmarks_3d(fan, net, x, fd)], steps)
            say('B=%-2d get_landmarks %9.3f ms   with flip_input %9.3f ms (%.2f x)   get_landmarks_3d %9.3f ms (+%.3f ms)' % (
                B, t2, tf_, tf_ / t2, t3, t3 - t2))
            hd, sdt = event_ms([lambda: L.depth_network(net, crop, maps), lambda: R3.depth_network(sdc, crop, maps)], steps)
            tf = B * fl / (hd * 1e-3) / 1e12
            say('B=%-2d depth network alone: HIP %9.3f ms  stock %9.3f ms (HIP/stock %.2f); HIP %.0f GFLOP/s (%.3f of the %.1f TF exact-f32 '
                'MFMA peak), stock %.0f GFLOP/s' % (B, hd, sdt, hd / sdt, tf * 1e3, tf / PEAK_TF, PEAK_TF, B * fl / (sdt * 1e-3) / 1e9))


if __name__ == '__main__':
    main()

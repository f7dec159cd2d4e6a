"""Times the 2D-FAN-4 landmark head on one GPU: the HIP head (landmarks.FAN, csrc/fan.hip) against the stock fp32 module with the
same weights (tests/fan_restatement.py's unfolded `network` on PyTorch-ROCm: MIOpen convs, eval BatchNorm), alternated call by call
in the same process: rows 1, 16 and 48 (3 x the trainer's per-rank batch) of 256x256 images, crop + network + decode and the network
alone, device events, 20 warm-up and 100 timed calls; the network alone also replayed as a hipGraph.  Synthetic weights throughout.

    python scripts/fan_time.py [--out profiles/fan_time.txt] [--steps 100] [--rows 1,16,48]
    python scripts/fan_time.py --only-b16             three B=16 calls of the HIP head (for a pass of
                                                      rocprofv3 --kernel-trace --stats --output-format csv of its own)
    python scripts/fan_time.py --stats <kernel_stats.csv> [--out ...]     per kernel family: time, useful FLOPs from the layer
                                                      shapes, TFLOP/s against the 157.3 TF exact-f32 MFMA peak
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEED = 13
PEAK_TF = 157.3
CALLS = 3


def flops():
    """Useful FLOPs per row of fan_conv_kernel<KS, EXT>, from the layer shapes."""
    f = {'<7, false>': 2 * 128 * 128 * 64 * 147, '<3, false>': 0, '<1, false>': 0, '<1, true>': 0}

    def block(cin, cout, h):
        f['<3, false>'] += 2 * h * h * 9 * (cin * cout // 2 + (cout // 2) * (cout // 4) + (cout // 4) * (cout // 4))
        if cin != cout:
            f['<1, false>'] += 2 * h * h * cin * cout

    def hourglass(level, h):
        block(256, 256, h)                       # b1
        block(256, 256, h // 2)                  # b2
        if level > 1:
            hourglass(level - 1, h // 2)
        else:
            block(256, 256, h // 2)              # b2_plus
        block(256, 256, h // 2)                  # b3

    block(64, 128, 128), block(128, 128, 64), block(128, 256, 64)
    for s in range(4):
        hourglass(4, 64)
        block(256, 256, 64)
        f['<1, false>'] += 2 * 64 * 64 * (256 * 256 + 256 * 68)
        if s < 3:
            f['<1, true>'] += 2 * 64 * 64 * (256 + 68) * 256
    return f, sum(f.values())


NAMES = {'<7, false>': 'stem conv 7x7/2', '<3, false>': 'ConvBlock 3x3 convs', '<1, false>': 'projections, conv_last, l', '<1, true>': 'bl + al'}


def stats(path, out):
    rows = list(csv.DictReader(open(path, newline='')))
    name_k = [k for k in rows[0] if k.lower() in ('name', 'kernelname', 'kernel_name')][0]
    dur_k = [k for k in rows[0] if 'total' in k.lower() and 'ns' in k.lower()][0]
    calls_k = [k for k in rows[0] if k.lower() in ('calls', 'count')][0]
    ours = [(r[name_k], int(r[calls_k]), float(r[dur_k])) for r in rows if 'fan_' in r[name_k] and 'pack' not in r[name_k]]
    fl, fwd = flops()
    tot = sum(t for _, _, t in ours) / CALLS
    lines = ['HIP FAN head, B=16 crop + network + decode: %.2f ms of kernel time per call; %.2f GFLOP per row by the layer shapes'
             % (tot / 1e6, fwd / 1e9)]
    for key, name in NAMES.items():
        t = sum(tt for n, _, tt in ours if 'fan_conv_kernel' in n and key.replace(' ', '') in n.replace(' ', '')) / CALLS
        if t:
            tf = 16 * fl[key] / (t * 1e-9) / 1e12
            lines.append('  %-36s %7.2f ms  %7.1f GFLOP  %5.1f TFLOP/s  (%.2f of %.1f)' % (name, t / 1e6, 16 * fl[key] / 1e9, tf, tf / PEAK_TF, PEAK_TF))
    for n, k, t in sorted(ours, key=lambda r: -r[2]):
        if 'fan_conv_kernel' not in n:
            short = n.split('fan_')[1].split('(')[0]
            lines.append('  fan_%-32s %7.2f ms  %d dispatches per call' % (short[:32], t / CALLS / 1e6, k // CALLS))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'a') as f:
            f.write(text + '\n')


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    if '--stats' in sys.argv:
        return stats(sys.argv[sys.argv.index('--stats') + 1], out)
    import torch
    from stylegan_directions_face_reenactment_amd import landmarks as L, synthetic as S
    import fan_restatement as R
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 100
    row_list = [int(v) for v in sys.argv[sys.argv.index('--rows') + 1].split(',')] if '--rows' in sys.argv else [1, 16, 48]
    sd = S.synthetic_fan_state(SEED)
    fan = L.FAN(4)
    fan.load_state_dict(sd)
    fan = fan.cuda().eval()
    sdc = {k: v.cuda() for k, v in sd.items()}

    def inputs(B):
        x = S.counter_tensor(SEED, 'ft.x%d' % B, (B, 3, 256, 256), 127.5, 60.0).clamp(0, 255).cuda()
        faces = torch.tensor([[52.0, 40.0, 204.0, 222.0]]).repeat(B, 1)
        return x, faces

    if '--only-b16' in sys.argv:
        x, faces = inputs(16)
        fd = faces.cuda()
        for _ in range(CALLS):
            L.get_landmarks(fan, x, fd)
        torch.cuda.synchronize()
        return

    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if out:
            with open(out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    def event_ms(fns, n, warm=20):
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

    def capture(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    _, fwd = flops()
    say('2D-FAN-4 landmark head, 256x256 images, synthetic weights (%s), %d timed calls' % (torch.cuda.get_device_name(0), steps))
    say('network: %.2f GFLOP per row by the layer shapes' % (fwd / 1e9))
    with torch.no_grad():
        for B in row_list:
            x, faces = inputs(B)
            fd = faces.cuda()
            crop = L.crop(x, fd)
            a, b = L.network(fan, crop), R.network(sdc, crop)['heatmaps'][-1]
            say('B=%d heatmaps: HIP vs stock max |diff| %.2e (max |heatmap| %.2f)' % (B, float((a - b).abs().max()), float(b.abs().max())))

            def hip_full():
                L.get_landmarks(fan, x, fd)

            def stock_full():
                R.decode(R.network(sdc, R.crop(x, faces))['heatmaps'][-1], faces)

            def hip_net():
                L.network(fan, crop)

            def stock_net():
                R.network(sdc, crop)

            for what, hf, sf in (('crop + network + decode', hip_full, stock_full), ('network alone', hip_net, stock_net)):
                he, se = event_ms([hf, sf], steps)
                line = 'B=%-2d %-24s eager: HIP %9.3f ms  stock %9.3f ms (HIP/stock %.2f)' % (B, what, he, se, he / se)
                if what == 'network alone':
                    hr, sr = event_ms([capture(hf).replay, capture(sf).replay], steps)
                    line += '   replayed: HIP %9.3f ms  stock %9.3f ms (HIP/stock %.2f)' % (hr, sr, hr / sr)
                    say(line)
                    tf = B * fwd / (hr * 1e-3) / 1e12
                    say('     HIP network replayed: %.0f GFLOP/s (%.3f of the %.1f TF exact-f32 MFMA peak); stock %.0f GFLOP/s'
                        % (tf * 1e3, tf / PEAK_TF, PEAK_TF, B * fwd / (sr * 1e-3) / 1e9))
                else:
                    say(line)


if __name__ == '__main__':
    main()

"""Times DECA's coefficient encoder on one GPU: the HIP head (deca.ResnetEncoder, csrc/deca.hip) against the stock fp32 module with
the same weights (tests/deca_restatement.py on PyTorch-ROCm: MIOpen convs, eval BatchNorm), alternated in the same process:
forward and forward + dL/dx at B = 1 and 16 on 256x256 inputs, device events, 20 warm-up and 100 timed calls, eager and replayed
as a hipGraph.  Synthetic weights throughout.

    python scripts/deca_time.py [--out profiles/deca_time.txt] [--steps 100]
    python scripts/deca_time.py --only-b16            three B=16 forward + dL/dx calls of the HIP head (for a pass of
                                                      rocprofv3 --kernel-trace --stats --output-format csv of its own)
    python scripts/deca_time.py --stats <kernel_stats.csv> [--out ...]     per kernel family: time, useful FLOPs from the layer
                                                      shapes, TFLOP/s against the 157.3 TF exact-f32 MFMA peak
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEED = 13
PEAK_TF = 157.3
LAYERS = ((64, 3), (128, 4), (256, 6), (512, 3))
CALLS = 3


def flops(B):
    """Useful FLOPs of one forward and one dL/dx per deca_conv_kernel<TAP, KS, EXT> instance, from the layer shapes."""
    f = {'<0, 7, false>': 2 * B * 112 * 112 * 64 * 147, '<0, 1, false>': 0, '<0, 3, false>': 0, '<0, 1, true>': 0, '<1, 3, false>': 0}
    head = 2 * B * (2048 * 1024 + 1024 * 236)
    f['<0, 1, false>'] += 2 * head                                      # forward and input gradient
    fwd = f['<0, 7, false>'] + head
    cin, h = 64, 56
    for i, (p, count) in enumerate(LAYERS):
        for k in range(count):
            s = 2 if (k == 0 and i > 0) else 1
            ho = h // s
            c1, c2, c3 = 2 * B * h * h * cin * p, 2 * B * ho * ho * 9 * p * p, 2 * B * ho * ho * p * 4 * p
            cd = 2 * B * ho * ho * cin * 4 * p if k == 0 else 0
            fwd += c1 + c2 + c3 + cd
            f['<0, 1, false>'] += c1 + c3 + cd + c3                     # forward 1x1s, conv3's input gradient
            f['<0, 3, false>'] += c2
            f['<1, 3, false>'] += c2
            if k == 0:
                f['<0, 1, true>'] += c1 + cd
            else:
                f['<0, 1, false>'] += c1
            cin, h = 4 * p, ho
    return f, fwd


NAMES = {'<0, 7, false>': 'stem conv 7x7/2', '<0, 1, false>': '1x1 convs, head GEMMs, 1x1 dgrads', '<0, 3, false>': 'conv2 3x3',
         '<0, 1, true>': 'conv1 + projection dgrad', '<1, 3, false>': 'conv2 3x3 dgrad'}


def stats(path, out):
    rows = list(csv.DictReader(open(path, newline='')))
    name_k = [k for k in rows[0] if k.lower() in ('name', 'kernelname', 'kernel_name')][0]
    dur_k = [k for k in rows[0] if 'total' in k.lower() and 'ns' in k.lower()][0]
    calls_k = [k for k in rows[0] if k.lower() in ('calls', 'count')][0]
    ours = [(r[name_k], int(r[calls_k]), float(r[dur_k])) for r in rows if 'deca_' in r[name_k] and 'pack' not in r[name_k]]
    fl, fwd = flops(16)
    tot = sum(t for _, _, t in ours) / CALLS
    lines = ['HIP DECA encoder, B=16 forward + dL/dx: %.2f ms of kernel time per call; forward %.2f GFLOP per row by the layer shapes'
             % (tot / 1e6, fwd / 16 / 1e9)]
    for key, name in NAMES.items():
        t = sum(tt for n, _, tt in ours if 'deca_conv_kernel' in n and key.replace(' ', '') in n.replace(' ', '')) / CALLS
        if t:
            tf = fl[key] / (t * 1e-9) / 1e12
            lines.append('  %-36s %7.2f ms  %7.1f GFLOP  %5.1f TFLOP/s  (%.2f of %.1f)' % (name, t / 1e6, fl[key] / 1e9, tf, tf / PEAK_TF, PEAK_TF))
    for n, k, t in sorted(ours, key=lambda r: -r[2]):
        if 'deca_conv_kernel' not in n:
            short = n.split('deca_')[1].split('(')[0]
            lines.append('  deca_%-31s %7.2f ms  %d dispatches per call' % (short[:31], t / CALLS / 1e6, k // CALLS))
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
    from stylegan_directions_face_reenactment_amd import deca as D, synthetic as S
    import deca_restatement as R
    from lpips_time import capture
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 100
    sd = S.synthetic_deca_encoder_state(SEED)
    E = D.ResnetEncoder()
    E.load_state_dict(sd)
    E = E.cuda().eval()
    sdc = {k: v.cuda() for k, v in sd.items()}

    def inputs(B):
        x = torch.tanh(S.counter_tensor(SEED, 'dt.x%d' % B, (B, 3, 256, 256))).cuda()
        boxes = torch.tensor([[60.0, 70.0, 196.0, 206.0]]).repeat(B, 1)
        return x, D.crop_matrix(boxes, (256, 256)).cuda(), S.counter_tensor(SEED, 'dt.g%d' % B, (B, 236)).cuda()

    if '--only-b16' in sys.argv:
        x, M, g = inputs(16)
        xs = x.clone().requires_grad_(True)
        for _ in range(CALLS):
            xs.grad = None
            (D.run(E, xs, M)[0] * g).sum().backward()
        torch.cuda.synchronize()
        return

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

    lines = ['DECA coefficient encoder, 256x256 -> 224x224 crop -> ResNet-50 -> 236 parameters, synthetic weights (%s), %d timed calls'
             % (torch.cuda.get_device_name(0), steps)]
    _, fwd = flops(1)
    lines.append('forward: %.2f GFLOP per row by the layer shapes' % (fwd / 1e9))
    for B in (1, 16):
        x, M, g = inputs(B)
        with torch.no_grad():
            a, b = D.run(E, x, M)[0], R.run(sdc, x, M)['params']
        lines.append('B=%d parameters: HIP vs stock max |diff| %.2e (max |p| %.2f)' % (B, float((a - b).abs().max()), float(b.abs().max())))
        xs = x.clone().requires_grad_(True)

        def hip_f():
            with torch.no_grad():
                D.run(E, x, M)

        def stock_f():
            with torch.no_grad():
                R.run(sdc, x, M)

        def hip_fb():
            xs.grad = None
            (D.run(E, xs, M)[0] * g).sum().backward()

        def stock_fb():
            xs.grad = None
            (R.run(sdc, xs, M)['params'] * g).sum().backward()

        for what, hf, sf in (('forward', hip_f, stock_f), ('forward + dL/dx', hip_fb, stock_fb)):
            he, se = event_ms([hf, sf], steps)
            gh, gs = capture(hf, clear=[xs]), capture(sf, clear=[xs])
            hr, sr = event_ms([gh.replay, gs.replay], steps)
            lines.append('B=%-2d %-16s eager: HIP %8.3f ms  stock %8.3f ms (HIP/stock %.2f)   replayed: HIP %8.3f ms  stock %8.3f ms (HIP/stock %.2f)'
                         % (B, what, he, se, he / se, hr, sr, hr / sr))
            if what == 'forward':
                lines.append('     HIP forward replayed: %.1f TFLOP/s (%.2f of the %.1f TF exact-f32 MFMA peak)'
                             % (B * fwd / (hr * 1e-3) / 1e12, B * fwd / (hr * 1e-3) / 1e12 / PEAK_TF, PEAK_TF))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

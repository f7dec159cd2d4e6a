"""Times the S3FD face detector on one GPU: the HIP detector (face_detector.S3FD, csrc/s3fd.hip) against the stock fp32 network with
the same weights (tests/s3fd_restatement.py's `network` on PyTorch-ROCm: MIOpen convs, torch max-pool and L2Norm), alternated call
by call in the same process: rows 1 and 48 (3 x the trainer's per-rank batch) of 256x256 images, device events, 10 warm-up and 50
timed calls.  Two comparisons: the network alone (the twelve maps), and HIP network + candidates + NMS against the stock network
alone -- the reference decodes on the CPU in a Python loop, which no device timer covers, so the second line flatters the stock
side.  Synthetic weights throughout.

    python scripts/s3fd_time.py [--out profiles/s3fd_time.txt] [--steps 50] [--rows 1,48]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEED = 20261018
PEAK_TF = 157.3


def flops(H, W):
    """Useful FLOPs per row from the layer shapes."""
    import s3fd_restatement as R
    from stylegan_directions_face_reenactment_amd import face_detector as FD
    det = FD.S3FD()
    total, h, w = 0, H, W
    for name in R.TRUNK:
        m = getattr(det, name)
        k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        total += 2 * h * w * m.out_channels * m.in_channels * k * k
        if name in R.POOL_AFTER:
            h, w = h // 2, w // 2
    for (hh, ww), name in zip(FD.level_dims(H, W), R.HEADS):
        c = getattr(det, name + '_mbox_conf')
        total += 2 * hh * ww * (c.out_channels + 4) * c.in_channels * 9
    return total


def main():
    import torch
    from stylegan_directions_face_reenactment_amd import face_detector as FD, synthetic as S
    import s3fd_restatement as R
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 50
    row_list = [int(v) for v in sys.argv[sys.argv.index('--rows') + 1].split(',')] if '--rows' in sys.argv else [1, 48]
    sd = S.synthetic_s3fd_state(SEED)
    det = FD.S3FD()
    det.load_state_dict(sd)
    det = det.cuda()
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

    fwd = flops(256, 256)
    say('S3FD face detector, 256x256 images, synthetic weights (%s), %d timed calls' % (torch.cuda.get_device_name(0), steps))
    say('network: %.2f GFLOP per row by the layer shapes' % (fwd / 1e9))
    with torch.no_grad():
        for B in row_list:
            x = R.images(S, SEED, 'st.x%d' % B, B, 256, 256).cuda()
            a, b = FD.network(det, x), R.network(sdc, x)['maps']
            say('B=%d maps: HIP vs stock max |diff| %.2e (max |map| %.2f)' % (B, max(float((p - q).abs().max()) for p, q in zip(a, b)),
                                                                            max(float(q.abs().max()) for q in b)))
            _, kept, valid = FD.detect(det, x)
            say('B=%d detect: %d..%d boxes per image, every list within the capacity: %s' % (B, int(kept.min()), int(kept.max()), bool(valid.all())))
            hn, sn = event_ms([lambda: FD.network(det, x), lambda: R.network(sdc, x)], steps)
            tf = B * fwd / (hn * 1e-3) / 1e12
            say('B=%-2d network alone            HIP %9.3f ms  stock %9.3f ms (HIP/stock %.2f)   HIP %.1f TFLOP/s = %.3f of the %.1f TF '
                'exact-f32 MFMA peak, stock %.1f TFLOP/s' % (B, hn, sn, hn / sn, tf, tf / PEAK_TF, PEAK_TF, B * fwd / (sn * 1e-3) / 1e12))
            hd, sn2 = event_ms([lambda: FD.detect(det, x), lambda: R.network(sdc, x)], steps)
            say('B=%-2d HIP network + candidates + NMS %9.3f ms  against the stock network alone %9.3f ms (HIP/stock %.2f)' % (B, hd, sn2, hd / sn2))


if __name__ == '__main__':
    main()

"""Times the alignment crop (face_crop.crop_using_landmarks, csrc/facecrop.hip) and reenact.preprocess_frames on one GPU: 32 frames
of 562 x 1000 (a 1080p frame after the reference's width-1000 resize), every second box leaving the frame by 50 pixels, the 256 x 256
output, device events, 10 warm-up and 50 timed calls.  preprocess_frames (S3FD, FAN, crop; synthetic weights, so the landmarks and
with them the boxes are arbitrary) runs as two calls of 16 frames: the detector takes at most 2^24 pixels per call; where one such
pass takes more than 150 ms it is timed over a fifth of the calls.  Recorded, not
asserted: there is no earlier figure to compare with.

    python scripts/face_crop_time.py [--out profiles/face_crop_time.txt] [--steps 50]
    python scripts/face_crop_time.py --cpu [--out profiles/face_crop_time.txt]      (no GPU: appends the PIL + scipy time of one frame)

--cpu times the same steps for ONE padded frame with numpy, scipy.ndimage and PIL on the host, as context only.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261018
B, H, W, SIZE = 32, 562, 1000, 200


def landmarks(np):
    """Box half side 200; even rows centred, odd rows 50 pixels over the left edge."""
    lm = np.empty((B, 68, 2), np.float32)
    for b in range(B):
        cx = 500.0 if b % 2 == 0 else 150.0
        lm[b, :, 0] = np.linspace(cx - SIZE / 2 - 0.125, cx + SIZE / 2 + 0.125, 68)
        lm[b, :, 1] = np.linspace(281 + SIZE // 6 - 60, 281 + SIZE // 6 + 60, 68)
    return lm


def cpu_frame(np, frame, lm):
    """The same steps for one frame on the host: the box and the mask of tests/face_crop_restatement.py, scipy's Gaussian, numpy's
    median and PIL's resize."""
    import scipy.ndimage
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import face_crop_restatement as R
    box, _ = R.crop_box(lm)
    pl, pt, pr, pb = R.borders(box, frame.shape[0], frame.shape[1])
    img = np.pad(frame, ((pt, pb), (pl, pr), (0, 0)), mode='symmetric').astype(np.float32)
    mask = R.feather_mask(img.shape[0], img.shape[1], (pl, pt, pr, pb))
    blur = scipy.ndimage.gaussian_filter(img, [R.SIGMA, R.SIGMA, 0])
    img = img + (blur - img) * np.clip(mask * np.float32(3) + np.float32(1), 0, 1)
    img = img + (np.median(img, axis=(0, 1)) - img) * np.clip(mask, 0, 1)
    crop = img[box[1] + pt:box[3] + pt, box[0] + pl:box[2] + pl]
    return np.array(Image.fromarray(crop.astype(np.uint8)).resize((256, 256), Image.BICUBIC))


def main():
    import numpy as np
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 50
    rng = np.random.default_rng(SEED)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    lm = landmarks(np)
    if '--cpu' in sys.argv:
        cpu_frame(np, frames[1], lm[1])
        t0 = time.perf_counter()
        for _ in range(5):
            cpu_frame(np, frames[1], lm[1])
        line = 'host, for context: numpy + scipy + PIL on one padded 562x1000 frame %.1f ms (mean of 5, one thread of the build machine)' % (
            (time.perf_counter() - t0) / 5 * 1e3)
        print(line)
        if out:
            with open(out, 'a') as f:
                f.write(line + '\n')
        return
    import torch
    from stylegan_directions_face_reenactment_amd import face_crop as FC, face_detector as FD, landmarks as L, reenact, synthetic as S
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if out:
            with open(out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    def event_ms(fn, n, warm=10):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tot = 0.0
        for _ in range(n):
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            tot += a.elapsed_time(b)
        return tot / n

    f, l = torch.from_numpy(frames).cuda(), torch.from_numpy(lm).cuda()
    say('alignment crop, %d frames of %dx%d, box side %d -> 256, every second box padded (%s), %d timed calls' % (
        B, H, W, 2 * SIZE, torch.cuda.get_device_name(0), steps))
    crops, valid = FC.crop_using_landmarks(f, l)
    say('valid rows %d of %d; workspace %.0f MB' % (int(valid.sum()), B, FC._workspace(B, H, W, max(H, W) // 2, f.device)[1] / 1e6))
    ms = event_ms(lambda: FC.crop_using_landmarks(f, l, as_tensor=True), steps)
    say('crop alone, all rows       %9.3f ms per call = %.3f ms per frame' % (ms, ms / B))
    ms0 = event_ms(lambda: FC.crop_using_landmarks(f, l[::2].repeat_interleave(2, 0).contiguous(), as_tensor=True), steps)
    say('crop alone, no row padded  %9.3f ms per call = %.3f ms per frame' % (ms0, ms0 / B))
    det = FD.S3FD()
    det.load_state_dict(S.synthetic_s3fd_state(SEED))
    det = det.cuda()
    fan = L.FAN(4)
    fan.load_state_dict(S.synthetic_fan_state(20261208), strict=True)
    fan = fan.cuda().eval()
    halves = (f[:16].contiguous(), f[16:].contiguous())
    whole = lambda: [reenact.preprocess_frames(det, fan, h) for h in halves]
    first = event_ms(whole, 1, warm=2)
    n, warm = (steps, 10) if first < 150.0 else (max(steps // 5, 1), 2)          # a slow detector pass gets fewer calls
    ms = event_ms(whole, n, warm=warm)
    say('preprocess_frames, 2 x 16  %9.3f ms for the 32 frames = %.3f ms per frame (detector and landmark network included; %d timed '
        'calls after %d)' % (ms, ms / B, n, warm))


if __name__ == '__main__':
    main()

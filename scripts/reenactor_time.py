"""Times the reenactment pipeline (reenact.Reenactor) and the launch below its pooled sessions (sgdfr_video_frames_f32) on one GPU.
Recorded, not asserted: there is no earlier end-to-end figure.

    python scripts/reenactor_time.py [--out profiles/reenactor_time.txt] [--frames 256]

(a) the fused frames launch against the composition it replaces, sgdfr_sweep_frames_f32(pooled) -> sgdfr_grid_to_u8_f32, at B = 32,
    P = 256, f = 4 and f = 2, source panel with batch stride 0, target panel per row, swap_rb on.  Same process, the two alternating
    window by window; a window is CALLS calls between two device events; the inputs rotate over buffers that together exceed the
    256 MiB cache, so no call finds its input there.  Median and min..max of the windows; bytes the launch needs (x once, the
    panels, the frames) over the median beside the 6.29 TB/s HBM copy rate of profiles/r06_i_pmc.md.
(b) Reenactor.reenact end to end, frames in to video frames out: N target frames of 256 x 256 and of 540 x 960, batch 32, cm = 1,
    synthetic weights in every network; wall time around a call that ends in a device synchronise, and device events around the same
    call; per stage (each stage run over all chunks between two synchronises: the stages of one call overlap less than that); and
    the same flow one frame at a time -- B = 1 calls of the same heads, generic.generate_image and grid_frames_uint8, the shape of
    run_inference.py:170-195 -- in the same process, alternating.  set_source with 200 PTI steps separately.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

COPY_RATE = 6.29e12
CALLS, WINDOWS = 100, 9


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def ab_windows(one, two):
    for i in range(10):
        one(i), two(i)
    torch.cuda.synchronize()
    t1, t2 = [], []
    for _ in range(WINDOWS):
        t1.append(window_ms(one, CALLS))
        t2.append(window_ms(two, CALLS))
    return t1, t2


def timed(fn):
    """(wall seconds, device-event seconds) of fn(), which leaves its work queued; both clocks stop behind a device synchronise."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, a.elapsed_time(b) * 1e-3


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    n_frames = int(sys.argv[sys.argv.index('--frames') + 1]) if '--frames' in sys.argv else 256
    if not torch.cuda.is_available():
        raise SystemExit('reenactor_time.py needs a GPU: a CPU run gives no time')
    from stylegan_directions_face_reenactment_amd import deca as DE, encoder as EN, face_detector as FD, landmarks as L, reenact as RE
    from stylegan_directions_face_reenactment_amd import synthetic as S
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    from stylegan_directions_face_reenactment_amd.model import Generator
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    from stylegan_directions_face_reenactment_amd.train_step import shape_params
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('reenactment pipeline on %s' % torch.cuda.get_device_name(0))
    # ---------------------------------------------------------------- (a)
    B, P = 32, 256
    src = torch.empty(1, 3, P, P, device='cuda').uniform_(-1.2, 1.2)
    tgt = torch.empty(B, 3, P, P, device='cuda').uniform_(-1.2, 1.2)
    say('(a) sgdfr_video_frames_f32 against sgdfr_sweep_frames_f32(pooled) -> sgdfr_grid_to_u8_f32: B = %d, P = %d, 3 panels, swap_rb; '
        '%d windows of %d calls each, alternating; HBM copy rate %.2f TB/s' % (B, P, WINDOWS, CALLS, COPY_RATE / 1e12))
    verdict = {}
    for f, n_buf in ((4, 3), (2, 4)):
        xs = [torch.empty(B, 3, P * f, P * f, device='cuda').uniform_(-1.2, 1.2) for _ in range(n_buf)]
        outs = [torch.empty(B, P, 3 * P, 3, device='cuda', dtype=torch.uint8) for _ in range(2)]
        fused = lambda i: RE.video_frames_uint8(xs[i % n_buf], [src, tgt], P, swap_rb=True, out=outs[0])
        comp = lambda i: RE.grid_frames_uint8([src, tgt, RE.pool_images(xs[i % n_buf], P)], swap_rb=True, out=outs[1])
        fused(0), comp(0)
        assert torch.equal(outs[0], outs[1])
        tf, tc = ab_windows(fused, comp)
        read = xs[0].numel() * 4
        need = read + src.numel() * 4 + tgt.numel() * 4 + outs[0].numel()
        need_c = need + 2 * B * 3 * P * P * 4                           # the float intermediate, written and read back
        mf, mc = statistics.median(tf), statistics.median(tc)
        say('    f = %d: x %.0f MB x %d buffers' % (f, read / 1e6, n_buf))
        say('      fused        median %7.4f ms (min %7.4f, max %7.4f)  needs %6.1f MB = %5.0f GB/s = %.2f of the copy rate'
            % (mf, min(tf), max(tf), need / 1e6, need / mf / 1e6, need / (mf * 1e-3) / COPY_RATE))
        say('      composition  median %7.4f ms (min %7.4f, max %7.4f)  needs %6.1f MB = %5.0f GB/s = %.2f of the copy rate'
            % (mc, min(tc), max(tc), need_c / 1e6, need_c / mc / 1e6, need_c / (mc * 1e-3) / COPY_RATE))
        spread = max(max(tf) - min(tf), max(tc) - min(tc))
        verdict[f] = mf <= mc + spread
        say('      fused / composition = %.3f; spread of the windows %.4f ms: the fused launch is %s'
            % (mf / mc, spread, 'not slower than the composition' if verdict[f] else 'SLOWER than the composition by more than the spread'))
        del xs, outs
    torch.cuda.empty_cache()
    # ---------------------------------------------------------------- (b)
    G = Generator(256, 512, 8, channel_multiplier=1)
    G.load_state_dict(S.synthetic_state_dict(G.state_dict(), seed=7))
    G = G.eval().cuda()
    A = DirectionMatrix(512, input_dim=15, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(5))
    A = A.cuda()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat8_shift.npz'))
    shifts = ShiftVectors('voxceleb', 15, 6, ranges=g['ranges_voxceleb'])
    det = FD.S3FD()
    det.load_state_dict(S.synthetic_s3fd_state(int(np.load(os.path.join(ROOT, 'tests', 'golden', 'kat14_s3fd.npz'))['seed'])), strict=True)
    det = det.cuda()
    fan = L.FAN(4)
    fan.load_state_dict(S.synthetic_fan_state(20261208), strict=True)
    fan = fan.cuda().eval()
    E = DE.ResnetEncoder()
    E.load_state_dict(S.synthetic_deca_encoder_state(20261101))
    E = E.cuda().eval()
    enc = EN.Encoder4Editing(50, 'ir_se', 256).eval()
    enc.load_state_dict(S.synthetic_encoder_state(enc.state_dict(), seed=7), strict=True)
    enc = enc.cuda()
    lp = LPIPS()
    lp.load_state_dict(S.synthetic_lpips_state(7))
    lp = lp.cuda()
    trunc = S.counter_tensor(7, 'trunc', (1, 512)).cuda()
    with torch.no_grad():
        faces, _ = G([S.synthetic_z(7, 32, key='time.z').cuda()], truncation=0.7, truncation_latent=trunc)
        faces = RE.images_to_uint8(faces)
        _, xf, okf = RE.preprocess_frames(det, fan, faces)
        _, _, hasf = FD.detect_landmarks(det, fan, xf, input_range='gan')
    good = (okf & hasf).nonzero().flatten().tolist()                    # frames the synthetic detector and the crop accept
    if len(good) < 2:
        raise SystemExit('only %d of 32 generated frames are usable with these synthetic weights' % len(good))
    faces = faces[good[:9]].contiguous()
    source, faces = faces[-1].contiguous(), faces[:-1]
    T = faces.shape[0]
    r = RE.Reenactor(G, A, enc, det, fan, E, shifts, truncation=0.7, trunc=trunc, lpips=lp, batch=32)
    say('(b) Reenactor.reenact, %d target frames, batch 32, 256^2 generator (cm 1), synthetic weights, output = video' % n_frames)
    for H, W in ((256, 256), (540, 960)):
        small = faces.repeat((n_frames + T - 1) // T, 1, 1, 1)[:n_frames]
        if (H, W) == (256, 256):
            frames = small.contiguous()
        else:                                                           # the same faces in the middle of a grey frame
            frames = torch.full((n_frames, H, W, 3), 128, dtype=torch.uint8, device='cuda')
            frames[:, (H - 256) // 2:(H - 256) // 2 + 256, (W - 256) // 2:(W - 256) // 2 + 256] = small
        r.set_source(source, optimize=False)
        info = {'x': r.source_x, 'params': r.source_params, 'angles': r.source_angles, 'code': r.session.source}

        def batched():
            return r.reenact(frames, on_fail='hold', output='video')

        def loop():
            video = []
            with torch.no_grad():
                for i in range(n_frames):
                    _, xt, ok = RE.preprocess_frames(det, fan, frames[i:i + 1])
                    _, boxes, has = FD.detect_landmarks(det, fan, xt, input_range='gan')
                    pt, at = shape_params(det, fan, E, xt, boxes=boxes, has_face=has)
                    sv = shifts.make_shift(info['angles'], at, info['params'], pt)
                    img = generate_image(G, info['code'], 0.7, trunc, True, 8, shift_code=A(sv), input_is_latent=True)
                    video.append(RE.grid_frames_uint8([info['x'], xt, img], swap_rb=True))
            return video

        for _ in range(3):
            batched()
        loop()
        _, ok, _ = batched()
        tb, tl = [], []
        for _ in range(3):
            tb.append(timed(batched))
            tl.append(timed(loop))
        wb, eb = min(t[0] for t in tb), min(t[1] for t in tb)
        wl, el = min(t[0] for t in tl), min(t[1] for t in tl)
        say('    frames %d x %d (%d of %d rows ok)' % (H, W, int(ok.sum()), n_frames))
        say('      Reenactor.reenact        wall %8.1f ms  device events %8.1f ms  %7.1f frames/s  %.3f ms per frame   (wall runs: %s ms)'
            % (1e3 * wb, 1e3 * eb, n_frames / wb, 1e3 * wb / n_frames, ' '.join('%.1f' % (1e3 * t[0]) for t in tb)))
        say('      one frame at a time      wall %8.1f ms  device events %8.1f ms  %7.1f frames/s  %.3f ms per frame   (wall runs: %s ms)'
            % (1e3 * wl, 1e3 * el, n_frames / wl, 1e3 * wl / n_frames, ' '.join('%.1f' % (1e3 * t[0]) for t in tl)))
        say('      ratio %.2fx' % (wl / wb))
        # per stage, each over all chunks between two synchronises
        chunks = [frames[lo:lo + 32] for lo in range(0, n_frames, 32)]
        keep = {}

        def st_pre():
            keep['pre'] = [RE.preprocess_frames(det, fan, c) for c in chunks]

        def st_shape():
            res = []
            with torch.no_grad():
                for _, xt, ok_ in keep['pre']:
                    _, boxes, has = FD.detect_landmarks(det, fan, xt, input_range='gan')
                    res.append(shape_params(det, fan, E, xt, boxes=boxes, has_face=has) + (ok_ & has,))
            keep['shape'] = res

        def st_shift():
            svs = torch.cat([shifts.make_shift(info['angles'], at, info['params'], pt) for pt, at, _ in keep['shape']])
            oks = torch.cat([o for _, _, o in keep['shape']])
            keep['sv'] = RE.hold_failed_rows(svs, oks, torch.zeros(15, device='cuda'), torch.zeros((), dtype=torch.bool, device='cuda'))[0]

        def st_render():
            keep['video'] = r.session.video_frames(info['x'], torch.cat([xt for _, xt, _ in keep['pre']]), keep['sv'], swap_rb=True)

        stages = (('preprocess (S3FD, FAN, crop)', st_pre), ('shape parameters (S3FD, FAN, DECA)', st_shape),
                  ('shift and policy', st_shift), ('render and frames', st_render))
        for _, fn in stages:
            fn()
        total = 0.0
        rows = []
        for name, fn in stages:
            t = min(timed(fn)[0] for _ in range(3))
            total += t
            rows.append((name, t))
        for name, t in rows:
            say('      stage %-36s %8.1f ms  %.3f ms per frame  %4.1f %%' % (name, 1e3 * t, 1e3 * t / n_frames, 100 * t / total))
        say('      stages, summed                             %8.1f ms' % (1e3 * total))
        keep.clear()
    # ---------------------------------------------------------------- set_source
    r.set_source(source, optimize=True, opt_steps=200)
    runs = [timed(lambda: r.set_source(source, optimize=True, opt_steps=200)) for _ in range(2)]
    plain = [timed(lambda: r.set_source(source, optimize=False)) for _ in range(2)]
    say('    set_source, 200 PTI steps   wall %8.1f ms (runs: %s ms)' % (1e3 * min(t[0] for t in runs), ' '.join('%.1f' % (1e3 * t[0]) for t in runs)))
    say('    set_source, optimize=False  wall %8.1f ms (runs: %s ms)' % (1e3 * min(t[0] for t in plain), ' '.join('%.1f' % (1e3 * t[0]) for t in plain)))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""Times cross-reenactment (Reenactor.analyse + reenact_many) and the launch below it (sgdfr_video_frames_px) on one GPU.

    python scripts/cross_reenact_time.py [--out profiles/cross_reenact_time.txt] [--frames 256] [--sources 4]

Without --leg this is a driver that never touches the GPU itself: it runs each leg in a fresh child process under a time limit of its
own (LIMITS), stops at the first leg that fails or runs out of time, and joins what the legs printed into --out.  The exit status is
nonzero when a leg fails or when one of the two bars below is missed.

(a) --leg a: sgdfr_video_frames_px with float32 panels against sgdfr_video_frames_f32 at B = 32, P = 256, f = 1, 2 and 4, source panel
    one row, target panel per row, swap_rb on.  Same process, the two alternating window by window; a window is CALLS calls between
    two device events; the inputs rotate over buffers that together exceed the 256 MiB cache (section (a) of
    profiles/reenactor_time.txt was measured this way).  BAR: the new entry is not slower than the existing one by more than the
    spread of the windows.  Then the new entry with the uint8 target panel: it reads 9 * P^2 fewer bytes a frame; bytes needed over the
    median as a fraction of the 6.29 TB/s HBM copy rate.
(b) --leg b: S sources against N target frames of 256 x 256, batch 32, cm = 1, synthetic weights: S make_source(optimize=False) +
    analyse + reenact_many against S passes of set_source(optimize=False) + reenact, in the same process, alternating; wall time
    around calls that end in a device synchronise, and the peak device memory of both forms.  BAR: the ratio is below 0.5 (from the
    stage table of profiles/reenactor_time.txt, (1001 + 4 * 25) / (4 * 1025) = 0.27 is expected at S = 4; above 0.5 the heads ran more
    than once).
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
CALLS, WINDOWS = 100, 9
LIMITS = {'a': 240, 'b': 420}                                             # seconds per leg


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def driver():
    import tempfile
    out = arg('--out', '')
    passed, text = True, []
    parts = tempfile.mkdtemp(prefix='cross_reenact_time.')
    for leg in ('a', 'b'):
        part = os.path.join(parts, leg + '.txt')
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--part', part, '--frames', str(arg('--frames', 256)),
               '--sources', str(arg('--sources', 4))]
        try:
            code = subprocess.run(cmd, timeout=LIMITS[leg]).returncode    # (the leg prints as it goes; its lines come back in `part`)
        except subprocess.TimeoutExpired:
            code = 124
        if os.path.exists(part):
            text.append(open(part).read())
        if code not in (0, 3):                                            # 3: the leg ran to its end and missed its bar
            print('leg (%s) ended with status %d: nothing further is started' % (leg, code), flush=True)
            return code
        passed = passed and code == 0
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write(''.join(text))
    return 0 if passed else 3


def window_ms(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def ab_windows(one, two):
    import torch
    for i in range(10):
        one(i), two(i)
    torch.cuda.synchronize()
    t1, t2 = [], []
    for _ in range(WINDOWS):
        t1.append(window_ms(one, CALLS))
        t2.append(window_ms(two, CALLS))
    return t1, t2


def say(s):
    print(s, flush=True)
    part = arg('--part', '')
    if part:
        with open(part, 'a') as fh:
            fh.write(s + '\n')


def leg_a():
    import torch
    from stylegan_directions_face_reenactment_amd import reenact as RE
    B, P = 32, 256
    say('cross-reenactment on %s' % torch.cuda.get_device_name(0))
    say('(a) sgdfr_video_frames_px against sgdfr_video_frames_f32: B = %d, P = %d, 3 panels, swap_rb; %d windows of %d calls each, '
        'alternating; HBM copy rate %.2f TB/s' % (B, P, WINDOWS, CALLS, COPY_RATE / 1e12))
    src = torch.empty(1, 3, P, P, device='cuda').uniform_(-1.2, 1.2)
    tgt_u8 = torch.randint(0, 256, (B, P, P, 3), device='cuda', dtype=torch.uint8)
    tgt = ((tgt_u8.float() / torch.full((1,), 255.0, device='cuda')) * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()
    ok = True
    for f, n_buf in ((1, 12), (2, 4), (4, 3)):
        xs = [torch.empty(B, 3, P * f, P * f, device='cuda').uniform_(-1.2, 1.2) for _ in range(n_buf)]
        outs = [torch.empty(B, P, 3 * P, 3, device='cuda', dtype=torch.uint8) for _ in range(3)]
        old = lambda i: RE.video_frames_uint8(xs[i % n_buf], [src, tgt], P, swap_rb=True, out=outs[0])
        new = lambda i: RE.video_frames_px(xs[i % n_buf], [src, tgt], P, swap_rb=True, out=outs[1])
        u8 = lambda i: RE.video_frames_px(xs[i % n_buf], [src, tgt_u8], P, swap_rb=True, out=outs[2])
        old(0), new(0), u8(0)
        assert torch.equal(outs[0], outs[1])
        differ = int((outs[0] != outs[2]).sum())                         # 0 when torch's device division gave the crop kernel's quotient
        t_new, t_old = ab_windows(new, old)
        t_u8, t_old2 = ab_windows(u8, old)
        read = xs[0].numel() * 4
        need = read + src.numel() * 4 + tgt.numel() * 4 + outs[0].numel()
        need_u8 = need - tgt.numel() * 4 + tgt_u8.numel()
        m_new, m_old, m_u8, m_old2 = (statistics.median(t) for t in (t_new, t_old, t_u8, t_old2))
        say('    f = %d: x %.0f MB x %d buffers' % (f, read / 1e6, n_buf))
        for name, t, m, n in (('video_frames_f32          ', t_old, m_old, need), ('video_frames_px, float32 ', t_new, m_new, need),
                              ('video_frames_f32 (again)  ', t_old2, m_old2, need), ('video_frames_px, uint8    ', t_u8, m_u8, need_u8)):
            say('      %s median %7.4f ms (min %7.4f, max %7.4f)  needs %6.1f MB = %5.0f GB/s = %.2f of the copy rate'
                % (name, m, min(t), max(t), n / 1e6, n / m / 1e6, n / (m * 1e-3) / COPY_RATE))
        spread = max(max(t_new) - min(t_new), max(t_old) - min(t_old))
        fine = m_new <= m_old + spread
        ok = ok and fine
        say('      px(float32) / f32 = %.3f; spread of the windows %.4f ms: the new entry is %s'
            % (m_new / m_old, spread, 'not slower than the existing one' if fine else 'SLOWER than the existing one by more than the spread'))
        say('      px(uint8) / f32 = %.3f: %.1f MB fewer to read (9 P^2 bytes a frame); %d bytes differ from the float target'
            % (m_u8 / m_old2, (need - need_u8) / 1e6, differ))
        del xs, outs
        torch.cuda.empty_cache()
    return 0 if ok else 3


def leg_b():
    import numpy as np
    import torch
    from stylegan_directions_face_reenactment_amd import deca as DE, encoder as EN, face_detector as FD, landmarks as L, reenact as RE
    from stylegan_directions_face_reenactment_amd import synthetic as S
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.model import Generator
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    n_frames, n_src = arg('--frames', 256), arg('--sources', 4)
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
    trunc = S.counter_tensor(7, 'trunc', (1, 512)).cuda()
    with torch.no_grad():
        faces, _ = G([S.synthetic_z(7, 48, key='time.z').cuda()], truncation=0.7, truncation_latent=trunc)
        faces = RE.images_to_uint8(faces)
        _, xf, okf = RE.preprocess_frames(det, fan, faces)
        _, _, hasf = FD.detect_landmarks(det, fan, xf, input_range='gan')
    good = (okf & hasf).nonzero().flatten().tolist()                    # frames the synthetic detector and the crop accept
    if len(good) < n_src + 1:
        raise SystemExit('only %d of 48 generated frames are usable with these synthetic weights' % len(good))
    faces = faces[good[:n_src + 8]].contiguous()
    source_frames, faces = [faces[i].contiguous() for i in range(n_src)], faces[n_src:]
    T = faces.shape[0]
    frames = faces.repeat((n_frames + T - 1) // T, 1, 1, 1)[:n_frames].contiguous()
    r = RE.Reenactor(G, A, enc, det, fan, E, shifts, truncation=0.7, trunc=trunc, batch=32)
    say('(b) %d sources x %d target frames of 256 x 256, batch 32, 256^2 generator (cm 1), synthetic weights, output = video'
        % (n_src, n_frames))

    def once():
        sources = [r.make_source(f, optimize=False) for f in source_frames]
        return r.reenact_many(sources, r.analyse(frames))

    def per_source():
        outs = []
        for f in source_frames:
            r.set_source(f, optimize=False)
            outs.append(r.reenact(frames))
        return outs

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        return t, torch.cuda.max_memory_allocated() - base, res

    for _ in range(2):
        many = once()
        each = per_source()
    same = all(torch.equal(many[0][s], each[s][0]) for s in range(n_src))
    say('    reenact_many equals the %d reenact passes byte for byte: %s; %d of %d rows ok' % (n_src, same, int(many[1].sum()), n_frames))
    del many, each
    t_once, t_each = [], []
    for _ in range(3):
        t_once.append(timed(once)[:2])
        t_each.append(timed(per_source)[:2])
    a, b = min(t[0] for t in t_once), min(t[0] for t in t_each)
    say('      make_source x %d + analyse + reenact_many   wall %8.1f ms  (runs: %s ms)  peak device memory above the models %7.1f MB'
        % (n_src, 1e3 * a, ' '.join('%.1f' % (1e3 * t[0]) for t in t_once), max(t[1] for t in t_once) / 1e6))
    say('      %d x (set_source + reenact)                  wall %8.1f ms  (runs: %s ms)  peak device memory above the models %7.1f MB'
        % (n_src, 1e3 * b, ' '.join('%.1f' % (1e3 * t[0]) for t in t_each), max(t[1] for t in t_each) / 1e6))
    ratio = a / b
    expected = (1001.0 + n_src * 25.0) / (n_src * 1025.0)
    say('      ratio %.3f (expected from the stage table %.2f; bar 0.5): %s; both forms hold all %d x %d frames at their end (%.0f MB)'
        % (ratio, expected, 'the heads ran once' if ratio < 0.5 else 'ABOVE THE BAR', n_src, n_frames, n_src * n_frames * 256 * 768 * 3 / 1e6))
    return 0 if (ratio < 0.5 and same) else 3


def main():
    leg = arg('--leg', '')
    if not leg:
        return driver()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('cross_reenact_time.py needs a GPU: a CPU run gives no time')
    return {'a': leg_a, 'b': leg_b}[leg]()


if __name__ == '__main__':
    sys.exit(main())

"""Times the frames kernels of csrc/sweep.hip (one pooled walk) against another build of the library on one GPU.

    python scripts/build_ref.py <parent commit>
    python scripts/frames_walk_time.py [--ref <csrc>/libsgdfr_hip_ref.so] [--out profiles/frames_walk_time.txt]

Without --leg this is a driver that never touches the GPU itself: it runs the rows below in three fresh child processes, one after
another, each under a time limit of its own -- the reference library (SGDFR_LIB), this tree's library, the reference library again --
stops at the first child that fails or runs out of time, and joins the figures into --out.  The Python above the library is this
tree's in all three.

Rows (the protocols of cross_reenact_time.py leg (a), reenactor_time.py leg (a) and sweep_time.py leg (b)): B = 32, P = 256, source
panel one row, target panel per row, swap_rb on; a window is CALLS calls between two device events, the rows of one f take their
windows in turn, the inputs rotate over buffers that together exceed the 256 MiB cache.
    video_frames_uint8 / video_frames_px with float32 panels / video_frames_px with a uint8 target panel, f = 1, 2, 4
    pool_frames two panels at R = 32, f = 4; pool_images at f = 4
    (reported only) video_frames_uint8 on the dword path: x one float off 16 bytes, f = 1 and 4
BAR, per gated row: the median of this tree's windows exceeds the median of the reference's windows (both runs) by no more than the
reference's own spread, max - min over the windows of its two runs.  The exit status is 3 when a row misses it.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, WINDOWS = 100, 9
LIMIT = 240                                                               # seconds per child


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def window_ms(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def turns(rows):
    """{name: [window ms]} for rows = [(name, fn)]: ten calls each to warm up, then WINDOWS rounds of one window per row."""
    import torch
    for _, fn in rows:
        for i in range(10):
            fn(i)
    torch.cuda.synchronize()
    t = {name: [] for name, _ in rows}
    for _ in range(WINDOWS):
        for name, fn in rows:
            t[name].append(window_ms(fn, CALLS))
    return t


def leg():
    import torch
    from stylegan_directions_face_reenactment_amd import reenact as RE
    from stylegan_directions_face_reenactment_amd.sweep import pool_frames
    B, P = 32, 256
    src = torch.empty(1, 3, P, P, device='cuda').uniform_(-1.2, 1.2)
    tgt_u8 = torch.randint(0, 256, (B, P, P, 3), device='cuda', dtype=torch.uint8)
    tgt = ((tgt_u8.float() / torch.full((1,), 255.0, device='cuda')) * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()
    outs = [torch.empty(B, P, 3 * P, 3, device='cuda', dtype=torch.uint8) for _ in range(4)]
    res = {'device': torch.cuda.get_device_name(0)}
    for f, n_buf in ((1, 12), (2, 4), (4, 3)):
        n = B * 3 * P * f * P * f
        flat = [torch.empty(n + 4, device='cuda').uniform_(-1.2, 1.2) for _ in range(n_buf)]
        xs = [t[:n].view(B, 3, P * f, P * f) for t in flat]
        off = [t[1:n + 1].view(B, 3, P * f, P * f) for t in flat]         # one float off 16 bytes: the dword path
        rows = [('video_frames_uint8 f=%d' % f, lambda i: RE.video_frames_uint8(xs[i % n_buf], [src, tgt], P, swap_rb=True, out=outs[0])),
                ('video_frames_px float32 f=%d' % f, lambda i: RE.video_frames_px(xs[i % n_buf], [src, tgt], P, swap_rb=True, out=outs[1])),
                ('video_frames_px uint8 f=%d' % f, lambda i: RE.video_frames_px(xs[i % n_buf], [src, tgt_u8], P, swap_rb=True, out=outs[2]))]
        if f != 2:
            rows.append(('(dword path) video_frames_uint8 f=%d' % f,
                         lambda i: RE.video_frames_uint8(off[i % n_buf], [src, tgt], P, swap_rb=True, out=outs[3])))
        if f == 4:
            rows += [('pool_frames 2 panels R=32 f=4', lambda i: pool_frames(xs[i % n_buf], P, None, src, ('frames',))),
                     ('pool_images f=4', lambda i: RE.pool_images(xs[i % n_buf], P))]
        res.update(turns(rows))
        del flat, xs, off, rows
        torch.cuda.empty_cache()
    with open(arg('--json', ''), 'w') as fh:
        json.dump(res, fh)
    return 0


def driver():
    import tempfile
    from stylegan_directions_face_reenactment_amd import build_native
    ref = arg('--ref', os.path.join(build_native.CSRC, 'libsgdfr_hip_ref.so'))
    if not os.path.exists(ref):
        raise SystemExit('no reference library at %s (python scripts/build_ref.py <commit>)' % ref)
    runs = []
    with tempfile.TemporaryDirectory(prefix='frames_walk_time.') as parts:
        for k, lib in enumerate((ref, None, ref)):
            env = dict(os.environ)
            env.pop('SGDFR_LIB', None)
            if lib:
                env.update(SGDFR_LIB=lib, SGDFR_ALLOW_LIB_OVERRIDE='1')
            part = os.path.join(parts, '%d.json' % k)
            try:
                code = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', 'run', '--json', part], env=env, timeout=LIMIT).returncode
            except subprocess.TimeoutExpired:
                code = 124
            if code != 0:
                print('run %d (%s) ended with status %d: nothing further is started' % (k, lib or 'this tree', code), flush=True)
                return code
            runs.append(json.load(open(part)))
    text = ['frames kernels on %s: reference library -> this tree -> reference library, one process each; B = 32, P = 256, 3 panels, '
            'swap_rb; %d windows of %d calls per row and run; ms per call' % (runs[0].pop('device'), WINDOWS, CALLS)]
    ok = True
    for name in runs[0]:
        par, new = runs[0][name] + runs[2][name], runs[1][name]
        m_par, m_new, spread = statistics.median(par), statistics.median(new), max(par) - min(par)
        gated = not name.startswith('(')
        fine = m_new <= m_par + spread
        ok = ok and (fine or not gated)
        text.append('  %-38s reference %7.4f (runs %7.4f, %7.4f; min %7.4f, max %7.4f)  this tree %7.4f (min %7.4f, max %7.4f)  '
                    'ratio %.3f  spread %.4f  %s'
                    % (name, m_par, statistics.median(runs[0][name]), statistics.median(runs[2][name]), min(par), max(par), m_new,
                       min(new), max(new), m_new / m_par, spread,
                       'reported only' if not gated else 'not slower' if fine else 'SLOWER by more than the spread'))
    text = '\n'.join(text) + '\n'
    print(text, flush=True)
    out = arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write(text)
    return 0 if ok else 3


def main():
    if not arg('--leg', ''):
        return driver()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('frames_walk_time.py needs a GPU: a CPU run gives no time')
    return leg()


if __name__ == '__main__':
    sys.exit(main())

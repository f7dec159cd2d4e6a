"""Times what the 512 / 1024 generator path adds on one GPU and writes profiles/hires_time.txt.

    python scripts/hires_bench.py --leg encode  --json <part>      e4e with 18 and 14 heads on a 256^2 input, B = 1 and 32: encoder.encode
                                                                   against the module's own MIOpen forward
    python scripts/hires_bench.py --leg poolmse --json <part>      PoolMse forward + backward at (1, 256, 4) and (1, 256, 2) against the
                                                                   stock pool + MSE autograd sequence
    python scripts/hires_bench.py --leg pti1024 --json <part>      the cm = 2 1024^2 generator: one PTI step, set_source with 200 steps,
                                                                   reenact of 256 frames at batch 32
    python scripts/hires_bench.py --join <part> ... --out profiles/hires_time.txt
    python scripts/hires_bench.py [--out ...]                      all three legs in fresh child processes, each under its own time
                                                                   limit, stopping at the first that fails, then the join

Method: every row is warmed up first; the rows that are compared take their windows in turn (one window of row A, one of row B, ...),
a window is CALLS calls between two device events; the median, the minimum and the maximum of the windows are stated, and the
spread (max - min) beside every ratio.  Synthetic weights; nothing outside the repository is read.  No threshold is set: the
figures are recorded.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = 7
LIMITS = {'encode': 300, 'poolmse': 240, 'pti1024': 900}                 # seconds per child


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


def turns(rows, calls, warm=5):
    """{name: [window ms]} for rows = [(name, fn)]: `warm` calls each, then WINDOWS rounds of one window per row."""
    import torch
    for _, fn in rows:
        for i in range(warm):
            fn(i)
    torch.cuda.synchronize()
    t = {name: [] for name, _ in rows}
    for _ in range(WINDOWS):
        for name, fn in rows:
            t[name].append(window_ms(fn, calls))
    return t


def leg_encode():
    import torch
    from stylegan_directions_face_reenactment_amd import encoder as EN, synthetic as S
    res = {}
    encs = {}
    for res_img in (1024, 256):
        enc = EN.Encoder4Editing(50, 'ir_se', res_img).eval()
        enc.load_state_dict(S.synthetic_encoder_state(enc.state_dict(), seed=7), strict=True)
        encs[enc.style_count] = enc.cuda()
    for B, calls in ((1, 10), (32, 3)):
        xs = [torch.empty(B, 3, 256, 256, device='cuda').uniform_(-1, 1) for _ in range(4)]
        rows = []
        for n, enc in encs.items():
            rows.append(('encode %d heads B=%d' % (n, B), lambda i, enc=enc: EN.encode(enc, xs[i % 4])))
            rows.append(('MIOpen forward %d heads B=%d' % (n, B), lambda i, enc=enc: _no_grad_forward(enc, xs[i % 4])))
        res.update(turns(rows, calls))
    return res


def _no_grad_forward(enc, x):
    import torch
    with torch.no_grad():
        return enc(x)


def leg_poolmse():
    import torch
    import torch.nn.functional as F
    from stylegan_directions_face_reenactment_amd.pool_loss import PoolMse
    res = {}
    B, P = 1, 256
    real = torch.empty(B, 3, P, P, device='cuda').uniform_(-1, 1)
    gp = torch.empty(B, 3, P, P, device='cuda').normal_()
    gm = torch.full((), 100.0, device='cuda')
    for f, n_buf in ((4, 24), (2, 96)):                                   # the inputs rotate over more than the 256 MiB cache
        xs = [torch.empty(B, 3, P * f, P * f, device='cuda').uniform_(-1, 1).requires_grad_(True) for _ in range(n_buf)]

        def hip(i):
            x = xs[i % n_buf]
            pooled, mse = PoolMse.apply(x, real, P)
            return torch.autograd.grad((pooled, mse), x, (gp, gm))

        def stock(i):
            x = xs[i % n_buf]
            pooled = F.adaptive_avg_pool2d(x, (P, P))
            mse = F.mse_loss(pooled, real)
            return torch.autograd.grad((pooled, mse), x, (gp, gm))

        res.update(turns([('PoolMse fwd+bwd f=%d' % f, hip), ('stock pool+mse autograd f=%d' % f, stock)], 50, warm=10))
        del xs
        torch.cuda.empty_cache()
    return res


def leg_pti1024():
    import numpy as np
    import torch
    from stylegan_directions_face_reenactment_amd import deca as DE, encoder as EN, face_detector as FD, finetune, landmarks as L
    from stylegan_directions_face_reenactment_amd import reenact as RE, synthetic as S
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    from stylegan_directions_face_reenactment_amd.model import Generator
    from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
    res = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def generator(size, cm):
        G = Generator(size, 512, 8, channel_multiplier=cm)
        G.load_state_dict(S.synthetic_state_dict(G.state_dict(), seed=7))
        return G.eval().cuda()

    G256, G = generator(256, 1), generator(1024, 2)
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
    enc = EN.Encoder4Editing(50, 'ir_se', 1024).eval()
    enc.load_state_dict(S.synthetic_encoder_state(enc.state_dict(), seed=7), strict=True)
    enc = enc.cuda()
    lp = LPIPS()
    lp.load_state_dict(S.synthetic_lpips_state(7))
    lp = lp.cuda()
    trunc = S.counter_tensor(7, 'trunc', (1, 512)).cuda()
    with torch.no_grad():                                                 # 256^2 faces of the small generator: the frames
        faces, _ = G256([S.synthetic_z(7, 32, key='time.z').cuda()], truncation=0.7, truncation_latent=trunc)
        faces = RE.images_to_uint8(faces)
        _, xf, okf = RE.preprocess_frames(det, fan, faces)
        _, _, hasf = FD.detect_landmarks(det, fan, xf, input_range='gan')
    good = (okf & hasf).nonzero().flatten().tolist()
    if len(good) < 2:
        raise SystemExit('only %d of 32 generated frames are usable with these synthetic weights' % len(good))
    faces = faces[good[:9]].contiguous()
    source, faces = faces[-1].contiguous(), faces[:-1]
    del G256
    r = RE.Reenactor(G, A, enc, det, fan, E, shifts, truncation=0.7, trunc=trunc, lpips=lp, batch=32)
    # one eager PTI step on a copy: forward at 1024^2, PooledPtiLoss, backward, Adam
    src0 = r.make_source(source, optimize=False)
    import copy
    G1 = copy.deepcopy(G)
    G1.invalidate_packs()
    loss_fn = finetune.PooledPtiLoss(lp, src0.x, 256)
    steps = []
    for _ in range(4):
        ms, _ = timed(lambda: finetune.optimize_g(G1, src0.code, src0.x, trunc, opt_steps=1, lr=3e-3, loss_fn=loss_fn, truncation=0.7, graph=False))
        steps.append(ms)
    res['one eager PTI step at 1024^2 (first call first)'] = steps
    del G1
    torch.cuda.empty_cache()
    ms, info = timed(lambda: r.set_source(source, optimize=True, opt_steps=200))
    res['set_source, 200 PTI steps'] = [ms]
    res['last PTI loss'] = [float(info['loss'])]
    n = 256
    frames = faces.repeat((n + faces.shape[0] - 1) // faces.shape[0], 1, 1, 1)[:n].contiguous()
    r.reenact(frames, on_fail='hold', output='video')                     # warm-up: packs, workspaces, graph captures
    res['reenact 256 frames, batch 32'] = [timed(lambda: r.reenact(frames, on_fail='hold', output='video'))[0] for _ in range(3)]
    return res


LEGS = {'encode': leg_encode, 'poolmse': leg_poolmse, 'pti1024': leg_pti1024}


def fmt(name, t):
    return '  %-44s median %9.4f ms  (min %9.4f, max %9.4f, %d windows)' % (name, statistics.median(t), min(t), max(t), len(t))


def ratio(text, res, a, b, what, stock=True):
    """stock: row b is the stock sequence row a stands in for: say so plainly where a is slower by more than the spread."""
    if a in res and b in res:
        ma, mb = statistics.median(res[a]), statistics.median(res[b])
        spread = max(max(res[a]) - min(res[a]), max(res[b]) - min(res[b]))
        text.append('      %s: %.3f (spread of the windows %.4f ms)%s' % (what, ma / mb, spread, '' if not stock or ma <= mb + spread else
                                                                        '  -- SLOWER than the stock sequence by more than the spread'))


def join(parts, out):
    res, device = {}, None
    for p in parts:
        d = json.load(open(p))
        device = d.pop('device', device)
        res.update(d)
    text = ['the 512 / 1024 generator path on %s (scripts/hires_bench.py); %d windows per row, the compared rows in turn; ms per call'
            % (device, WINDOWS)]
    if any(k.startswith('encode') for k in res):
        text.append('e4e on a 256^2 input, synthetic weights: encoder.encode (csrc/e4e.hip) against the module\'s MIOpen forward')
        for B in (1, 32):
            for n in (18, 14):
                a, b = 'encode %d heads B=%d' % (n, B), 'MIOpen forward %d heads B=%d' % (n, B)
                if a in res:
                    text += [fmt(a, res[a]), fmt(b, res[b])]
                    ratio(text, res, a, b, 'encode / MIOpen forward')
            ratio(text, res, 'encode 18 heads B=%d' % B, 'encode 14 heads B=%d' % B, '18 heads / 14 heads on the HIP path', stock=False)
    if any(k.startswith('PoolMse') for k in res):
        text.append('PoolMse forward + backward (one walk, one finish, one backward launch) against adaptive_avg_pool2d + mse_loss + '
                    'autograd, B = 1, P = 256, gradients into both outputs')
        for f in (4, 2):
            a, b = 'PoolMse fwd+bwd f=%d' % f, 'stock pool+mse autograd f=%d' % f
            if a in res:
                mb = 3 * (256 * f) ** 2 * 4 / 1e6
                text += [fmt(a, res[a]), fmt(b, res[b])]
                ratio(text, res, a, b, 'PoolMse / stock')
                ma = statistics.median(res[a])
                text.append('      bytes the pair has to move: %.1f MB read (x) + %.1f MB written (dx) per step, + %.1f MB of pooled-size '
                            'tensors = %.0f GB/s over the pair' % (mb, mb, 6 * 3 * 256 * 256 * 4 / 1e6,
                                                                   (2 * mb + 6 * 3 * 256 * 256 * 4 / 1e6) / ma))
    if any(k.startswith('set_source') for k in res):
        text.append('the cm = 2 1024^2 generator, 18-head encoder on the 256^2 crop, PooledPtiLoss, synthetic weights (wall clock, one run)')
        for k in ('one eager PTI step at 1024^2 (first call first)', 'set_source, 200 PTI steps', 'reenact 256 frames, batch 32'):
            if k in res:
                text.append('  %-44s %s ms' % (k, ', '.join('%.1f' % v for v in res[k])))
        if 'last PTI loss' in res:
            text.append('  last PTI loss %.6g' % res['last PTI loss'][0])
    text = '\n'.join(text) + '\n'
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write(text)
    return 0


def driver():
    import tempfile
    parts = []
    with tempfile.TemporaryDirectory(prefix='hires_bench.') as tmp:
        for name in LEGS:
            part = os.path.join(tmp, name + '.json')
            try:
                code = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, '--json', part], timeout=LIMITS[name]).returncode
            except subprocess.TimeoutExpired:
                code = 124
            if code != 0:
                print('leg %s ended with status %d: nothing further is started' % (name, code), flush=True)
                return code
            parts.append(part)
        return join(parts, arg('--out', os.path.join(ROOT, 'profiles', 'hires_time.txt')))


def main():
    if '--join' in sys.argv:
        i = sys.argv.index('--join') + 1
        parts = []
        while i < len(sys.argv) and not sys.argv[i].startswith('--'):
            parts.append(sys.argv[i])
            i += 1
        return join(parts, arg('--out', ''))
    name = arg('--leg', '')
    if not name:
        return driver()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('hires_bench.py needs a GPU: a CPU run gives no time')
    res = LEGS[name]()
    res['device'] = torch.cuda.get_device_name(0)
    with open(arg('--json', ''), 'w') as fh:
        json.dump(res, fh)
    return 0


if __name__ == '__main__':
    sys.exit(main())

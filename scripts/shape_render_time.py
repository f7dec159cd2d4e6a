"""Times the shape renderer (shape_render.py, csrc/shaperender.hip) on one GPU: reenact.shape_panels for 256 frames, batch 32, size 256,
and the split between its launches.  Recorded, not asserted: there is no stock path to beat and no earlier figure.

    python scripts/shape_render_time.py [--out profiles/shape_render_time.txt] [--steps 20]

Two meshes, because FLAME's own files are not part of this repository:
  soup    the synthetic FLAME tables of the tests (synthetic.synthetic_flame_state): 5023 vertices and 9976 faces drawn as random index
          triples, at DECA's camera scale 8.  Every pixel lies under about a thousand faces and every tile meets nearly every face: the
          worst case for the rasteriser, far from what a face mesh costs.
  sheet   a manifold sheet of FLAME's size (71 x 71 vertices, 9800 faces) bent into a dome that fills the middle of the image the way
          a fitted head does: a few faces per pixel.  This is the figure to read as "a frame".
Each step runs in a process of its own under its own time limit; the first step that fails or runs out of time ends the run.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261019
N, BATCH, SIZE = 256, 32, 256
HEADS_MS_PER_FRAME = 4.003          # profiles/reenactor_time.txt: Reenactor.reenact, 256 x 256 frames
STEPS = (('soup', 240), ('sheet', 240), ('split', 240))


def event_ms(torch, fn, n, warm=3):
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


def flame_module(torch):
    from stylegan_directions_face_reenactment_amd import flame as FL, synthetic as S
    m = FL.FLAME()
    m.load_state_dict(S.synthetic_flame_state(SEED))
    return m.cuda()


def soup_params(torch, rows):
    from stylegan_directions_face_reenactment_amd import synthetic as S
    c = S.synthetic_flame_coeffs(SEED, 'shape_render_time', rows, [0.3 * ((i % 7) - 3) for i in range(rows)])
    return {'alpha_shp': c['shape'].cuda(), 'alpha_exp': c['exp'].cuda(), 'pose': c['pose'].cuda(), 'cam': c['cam'].cuda()}


def sheet(torch, rows):
    """(vertices [rows,V,3], MeshTopology, cam [rows,3]): a dome of 71 x 71 vertices, about 0.18 across, at camera scale 8"""
    import numpy as np
    from stylegan_directions_face_reenactment_amd.shape_render import MeshTopology
    n = 71
    u, v = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    verts = np.stack([0.09 * u, 0.11 * v, 0.08 * np.cos(1.3 * u) * np.cos(1.1 * v)], -1).reshape(1, -1, 3)
    yaw = np.linspace(-0.5, 0.5, rows).reshape(rows, 1, 1)
    x, z = verts[..., 0:1], verts[..., 2:3]
    verts = np.concatenate([np.cos(yaw) * x + np.sin(yaw) * z, np.broadcast_to(verts[..., 1:2], (rows, n * n, 1)), np.cos(yaw) * z - np.sin(yaw) * x], -1)
    faces = []
    for r in range(n - 1):
        for m in range(n - 1):
            k = r * n + m
            faces += [[k, k + 1, k + n + 1], [k, k + n + 1, k + n]]
    cam = torch.tensor([[8.0, 0.0, 0.0]]).repeat(rows, 1)
    return torch.tensor(verts, dtype=torch.float32).cuda(), MeshTopology(torch.tensor(faces), n * n), cam.cuda()


def step(name, steps):
    import torch
    from stylegan_directions_face_reenactment_amd import flame as FL, reenact, shape_render as SR
    dev = torch.cuda.get_device_name(0)
    share = lambda ms: '%.1f %% of the %.1f ms a frame the heads take' % (100.0 * ms / HEADS_MS_PER_FRAME, HEADS_MS_PER_FRAME)
    if name == 'soup':
        m, params = flame_module(torch), soup_params(torch, N)
        out = reenact.shape_panels(m, params, size=SIZE, batch=BATCH)
        covered = float((out != -1.0).any(1).float().mean())
        ms = event_ms(torch, lambda: reenact.shape_panels(m, params, size=SIZE, batch=BATCH), max(steps // 4, 2), warm=1)
        print('soup   (%s) shape_panels N = %d, batch %d, size %d: %9.2f ms per call = %.3f ms per frame (%.2f of the pixels lit); %s'
              % (dev, N, BATCH, SIZE, ms, ms / N, covered, share(ms / N)))
    elif name == 'sheet':
        v, topo, cam = sheet(torch, N)

        def panels():
            return [SR.render_shape(v[lo:lo + BATCH], topo, cam=cam[lo:lo + BATCH], size=SIZE, gan_range=True)['shape'] for lo in range(0, N, BATCH)]

        out = torch.cat(panels())
        covered = float((out != -1.0).any(1).float().mean())
        ms = event_ms(torch, panels, steps)
        m, params = flame_module(torch), soup_params(torch, BATCH)
        fl = event_ms(torch, lambda: m(params['alpha_shp'], params['alpha_exp'], params['pose']), steps) * (N / BATCH)
        print('sheet  (%s) render_shape N = %d, batch %d, size %d: %9.3f ms per call = %.4f ms per frame (%.2f of the pixels lit)'
              % (dev, N, BATCH, SIZE, ms, ms / N, covered))
        print('       with the FLAME forward of shape_panels (%.3f ms for the %d frames): %.4f ms per frame; %s'
              % (fl, N, (ms + fl) / N, share((ms + fl) / N)))
    elif name == 'split':
        v, topo, cam = sheet(torch, BATCH)
        m = flame_module(torch)
        soup_topo, sp = FL.topology(m), soup_params(torch, BATCH)
        with torch.no_grad():
            sv = m(sp['alpha_shp'], sp['alpha_exp'], sp['pose'])[0].contiguous()
        proj = lambda vv, cc: torch.stack([cc[:, None, 0] * (vv[..., 0] + cc[:, None, 1]), -(cc[:, None, 0] * (vv[..., 1] + cc[:, None, 2])),
                                           -(cc[:, None, 0] * vv[..., 2]) + 10.0], -1).contiguous()
        for label, vv, tt, cc in (('sheet', v, topo, cam), ('soup', sv, soup_topo, sp['cam'])):
            p = proj(vv, cc)
            n_ms = event_ms(torch, lambda: SR.vertex_normals(vv, tt), steps)
            r_ms = event_ms(torch, lambda: SR.rasterize(p, tt, SIZE), steps)
            w_ms = event_ms(torch, lambda: SR.render_shape(vv, tt, cam=cc, size=SIZE), steps)
            print('split  %-5s batch %d, size %d: one normals launch %.4f ms; project + face setup + raster without shading %.4f ms; '
                  'render_shape whole (five launches) %.4f ms' % (label, BATCH, SIZE, n_ms, r_ms, w_ms))
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for _ in range(5):
                        SR.render_shape(vv, tt, cam=cc, size=SIZE)
                    torch.cuda.synchronize()
                for e in prof.key_averages():
                    if 'sgdfr' in e.key and e.count:
                        total = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
                        print('       %-5s %-60s %9.4f ms per launch (%d launches)' % (label, e.key[:60], total / e.count / 1e3, e.count))
            except Exception as ex:                              # the profiler is context, not the measurement
                print('       per-kernel times not available (%s)' % type(ex).__name__)
    else:
        raise SystemExit('unknown step %r' % name)


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 20
    if '--step' in sys.argv:
        step(sys.argv[sys.argv.index('--step') + 1], steps)
        return
    lines = ['shape renderer: %d frames, batch %d, size %d, %d timed calls per figure' % (N, BATCH, SIZE, steps)]
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name, '--steps', str(steps)], timeout=limit,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            lines.append('step %s: no result within %d s; nothing further was run' % (name, limit))
            break
        lines += [l for l in r.stdout.splitlines() if l.strip()]
        if r.returncode != 0:
            lines.append('step %s: exit status %d; nothing further was run' % (name, r.returncode))
            lines += r.stderr.splitlines()[-5:]
            break
    print('\n'.join(lines))
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

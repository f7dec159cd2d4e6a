"""Times DECA's detail path on one GPU at batch 32, each part against the same step written as stock torch ops in fp32 on the same
device: E_detail (deca.ResnetEncoder(128)) against the stock module of tests/deca_restatement.py; D_detail (detail.DetailDecoder)
against F.interpolate + F.conv2d on the folded weights; the UV pass (detail.detail_normals, one launch) against gathers and
index_add_; the detail shade (shape_render.render_shape with a layout) against the smooth panel alone and, for what it adds,
gathers + F.grid_sample + the light sum on the rasteriser's outputs.  Recorded, not asserted.

    python scripts/detail_time.py [--out profiles/detail_time.txt] [--steps 30]

The mesh is a manifold sheet of FLAME's size (71 x 71 vertices, 9800 faces) bent into a dome, as in scripts/shape_render_time.py, with a
planar UV atlas; FLAME's own files are not part of this repository.  Warm-up calls first, then device-event time per call, the HIP
and the stock function alternated call by call in one process.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEED = 20261201
B, SIZE, UV = 32, 224, 256
HEADS_MS_PER_FRAME = 4.003          # profiles/reenactor_time.txt: Reenactor.reenact, 256 x 256 frames


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from stylegan_directions_face_reenactment_amd import deca as D, detail as DT, shape_render as SR, synthetic as S
    import deca_restatement as RE
    import detail_restatement as RD
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 30

    def event_ms(fns, n, warm=5):
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

    lines = ['DECA detail path, batch %d, image %d, UV map %d, synthetic weights (%s), %d timed calls per figure, eager'
             % (B, SIZE, UV, torch.cuda.get_device_name(0), steps)]
    total = 0.0

    def report(what, hip, stock, note=''):
        lines.append('%-14s HIP %8.3f ms a batch = %.4f ms a frame   stock fp32 %8.3f ms a batch = %.4f ms a frame (HIP/stock %.2f)%s'
                     % (what, hip, hip / B, stock, stock / B, hip / stock, note))

    with torch.no_grad():
        # ---- E_detail
        sd = S.synthetic_deca_detail_encoder_state(SEED)
        Ed = D.ResnetEncoder(128)
        Ed.load_state_dict(sd)
        Ed = Ed.cuda().eval()
        sdc = {k: v.cuda() for k, v in sd.items()}
        x = torch.tanh(S.counter_tensor(SEED, 'dt.x', (B, 3, 256, 256))).cuda()
        M = D.crop_matrix(torch.tensor([[60.0, 70.0, 196.0, 206.0]]).repeat(B, 1), (256, 256)).cuda()
        a, b = D.run(Ed, x, M)[0], RE.encoder(sdc, RE.front(x, M))['params']
        lines.append('E_detail codes: HIP vs stock max |diff| %.2e (max |code| %.2f)' % (float((a - b).abs().max()), float(b.abs().max())))
        h, s = event_ms([lambda: D.run(Ed, x, M), lambda: RE.encoder(sdc, RE.front(x, M))], steps)
        report('E_detail', h, s)
        total += h
        del Ed, sdc

        # ---- D_detail
        Dd = DT.DetailDecoder()
        Dd.load_state_dict(S.synthetic_detail_decoder_state(SEED))
        Dd = Dd.cuda().eval()
        folded = Dd.folded()
        z = S.counter_tensor(SEED, 'dt.z', (B, 181)).cuda()
        a, b = Dd(z), RD.decoder_chain(folded, z, Dd.out_scale, dtype=torch.float32)[0]
        lines.append('D_detail uv_z: HIP vs stock max |diff| %.2e (max |uv_z| %.4f)' % (float((a - b).abs().max()), float(b.abs().max())))
        h, s = event_ms([lambda: Dd(z), lambda: RD.decoder_chain(folded, z, Dd.out_scale, dtype=torch.float32)], steps)
        macs = 181 * 8192 + sum(9 * ci * co * (16 << i) ** 2 for i, (ci, co) in enumerate(RD.CHANNELS)) + 9 * 16 * 256 * 256
        report('D_detail', h, s, '; %.2f GMAC a row, HIP %.1f TFLOP/s' % (macs / 1e9, 2 * macs * B / h / 1e9))
        total += h
        uv_z = a

        # ---- the mesh and its atlas
        n = 71
        u, v = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
        base = np.stack([0.09 * u, 0.11 * v, 0.08 * np.cos(1.3 * u) * np.cos(1.1 * v)], -1).reshape(1, -1, 3)
        yaw = np.linspace(-0.5, 0.5, B).reshape(B, 1, 1)
        xx, zz = base[..., 0:1], base[..., 2:3]
        verts = np.concatenate([np.cos(yaw) * xx + np.sin(yaw) * zz, np.broadcast_to(base[..., 1:2], (B, n * n, 1)), np.cos(yaw) * zz - np.sin(yaw) * xx], -1)
        faces = []
        for r in range(n - 1):
            for m in range(n - 1):
                k = r * n + m
                faces += [[k, k + 1, k + n + 1], [k, k + n + 1, k + n]]
        faces = torch.tensor(faces)
        uv = torch.tensor(np.stack([0.02 + 0.96 * (u + 1) / 2, 0.02 + 0.96 * (v + 1) / 2], -1).reshape(-1, 2))
        mask = (S.counter_tensor(SEED, 'dt.mask', (UV, UV)) > -0.7).float()
        fixed = S.counter_tensor(SEED, 'dt.fixed', (UV, UV), 0.0, 0.003)
        L = DT.UvLayout(faces, uv, faces, UV, mask, fixed, n_vertices=n * n)
        topo = SR.MeshTopology(faces, n * n)
        verts = torch.tensor(verts, dtype=torch.float32).cuda()
        cam = torch.tensor([[8.0, 0.0, 0.0]]).repeat(B, 1).cuda()
        normals = SR.vertex_normals(verts, topo)
        fd, pix, bary, maskd, fixedd, face_uv = L.tables('cuda')

        # ---- UV pass
        tri = faces.cuda()[pix.long().clamp(min=0)]                                   # [S,S,3]
        w = torch.where((pix >= 0)[..., None], bary, torch.zeros((), device='cuda'))
        dense_faces = L.dense_faces.cuda()

        def stock_w2uv(values):
            att = values[:, tri]
            return (w[None, ..., 0, None] * att[..., 0, :] + w[None, ..., 1, None] * att[..., 1, :] + w[None, ..., 2, None] * att[..., 2, :]).permute(0, 3, 1, 2)

        def stock_uv():
            uv_v, uv_n = stock_w2uv(verts), stock_w2uv(normals)
            P = uv_v + (uv_z * maskd) * uv_n + fixedd[None, None] * uv_n
            dense = P.permute(0, 2, 3, 1).reshape(B, -1, 3)
            nrm = torch.zeros_like(dense)
            for k in (1, 2, 0):
                o, p, q = (dense[:, dense_faces[:, (k + i) % 3]] for i in range(3))
                nrm.index_add_(1, dense_faces[:, k], torch.cross(p - o, q - o, dim=-1))
            return F.normalize(nrm, eps=1e-6, dim=2).reshape(B, UV, UV, 3).permute(0, 3, 1, 2)

        a, b = DT.detail_normals(L, uv_z, verts, normals), stock_uv()
        lines.append('UV pass normals: HIP vs stock max |diff| %.2e (index_add_ on the device sums in no fixed order)' % float((a - b).abs().max()))
        h, s = event_ms([lambda: DT.detail_normals(L, uv_z, verts, normals), stock_uv], steps)
        report('UV pass', h, s)
        total += h
        uvn = a

        # ---- detail shade
        both = lambda: SR.render_shape(verts, topo, cam=cam, size=SIZE, layout=L, detail_normals=uvn, want=('shape', 'shape_detail'))
        smooth = lambda: SR.render_shape(verts, topo, cam=cam, size=SIZE)
        r = SR.render_shape(verts, topo, cam=cam, size=SIZE, want=('shape', 'alpha', 'pix_to_face', 'bary'))
        lights = torch.tensor(SR.DEFAULT_LIGHTS, device='cuda')
        d = F.normalize(lights[:, :3], dim=1)

        def stock_shade():
            p, covered = r['pix_to_face'].long(), r['pix_to_face'] >= 0
            wb = torch.where(covered[..., None], r['bary'], torch.zeros((), device='cuda'))
            fu = face_uv[p.clamp(min=0)]
            g = wb[..., 0, None] * fu[..., 0, :] + wb[..., 1, None] * fu[..., 1, :] + wb[..., 2, None] * fu[..., 2, :]
            Nn = F.grid_sample(uvn, g, mode='bilinear', padding_mode='zeros', align_corners=False) * covered[:, None]
            dots = torch.einsum('bcij,lc->bijl', Nn, d).clamp(0, 1)
            shading = torch.einsum('bijl,lc->bijc', dots, lights[:, 3:]) / lights.shape[0]
            return ((wb.sum(-1) * (180.0 / 255.0))[..., None] * shading).permute(0, 3, 1, 2) * r['alpha']

        a, b = both()['shape_detail'], stock_shade()
        lines.append('detail shade panel: HIP vs stock max |diff| %.2e (%.2f of the pixels covered)'
                     % (float((a - b).abs().max()), float((r['pix_to_face'] >= 0).float().mean())))
        hb, hs, s = event_ms([both, smooth, stock_shade], steps)
        lines.append('%-14s HIP both panels %8.3f ms a batch = %.4f ms a frame; the smooth panel alone %8.3f ms: the detail panel adds %.3f ms a '
                     'batch = %.4f ms a frame; stock fp32 shade on the rasteriser\'s outputs (no raster) %8.3f ms a batch (added HIP/stock %.2f)'
                     % ('detail shade', hb, hb / B, hs, hb - hs, (hb - hs) / B, s, (hb - hs) / s))
        total += hb - hs
    lines.append('the detail path adds %.3f ms a batch = %.4f ms a frame: %.1f %% of the %.1f ms a frame the head chain takes (E_detail, D_detail, '
                 'the UV pass, the detail panel beside the smooth one; the coarse normals and FLAME are already part of the shape panel)'
                 % (total, total / B, 100.0 * total / B / HEADS_MS_PER_FRAME, HEADS_MS_PER_FRAME))
    print('\n'.join(lines))
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""Times DECA's texture side on one GPU at batch 32, each part against the same step written as stock torch ops in fp32 on the same
device: FlameTex (texture.FlameTex, the real 512 x 512 x 3 x 50 basis) against the reference expression (broadcast-multiply-sum,
F.interpolate, channel index); the UV texture pass (texture.uv_textures, one launch) against gathers + F.grid_sample + the SH
expression; the textured render (shape_render.render_texture) against gathers + F.grid_sample + the SH expression on this
repository's own rasterize output -- no stock rasteriser exists to compare with, so that figure says what the fused epilogue saves,
and the whole launch is given beside it.  Recorded, not asserted.

    python scripts/texture_time.py [--out profiles/texture_time.txt] [--steps 30]

The mesh is the manifold sheet of FLAME's size of scripts/detail_time.py (71 x 71 vertices, 9800 faces) with a planar UV atlas.
Warm-up calls first, then device-event time per call, the HIP and the stock function alternated call by call in one process.
FlameTex's bytes are those of its pack (51 planes of 3 x 256 x 256 floats) read once plus the albedo written; the copy rate it is
held against is the 6.29 TB/s of BASELINE.md.  The pack (40 MB) fits the 256 MiB Infinity Cache, so the figure is given twice: as called
(one pack, repeated calls) and with eight copies of the pack and eight outputs taken in turn (524 MB), which the cache cannot hold.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEED = 20261215
B, SIZE, UV, SOURCE, N_TEX = 32, 224, 256, 512, 50
HBM_COPY_TBS = 6.29


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from stylegan_directions_face_reenactment_amd import detail as DT, shape_render as SR, synthetic as S, texture as TX
    import texture_restatement as RT
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

    lines = ['DECA texture side, batch %d, image %d, UV map %d, basis %d x %d x 3 x %d, synthetic values (%s), %d timed calls per figure, eager'
             % (B, SIZE, UV, SOURCE, SOURCE, N_TEX, torch.cuda.get_device_name(0), steps)]

    def report(what, hip, stock, note=''):
        lines.append('%-16s HIP %8.3f ms a batch = %.4f ms a frame   stock fp32 %8.3f ms a batch = %.4f ms a frame (HIP/stock %.3f)%s'
                     % (what, hip, hip / B, stock, stock / B, hip / stock, note))

    with torch.no_grad():
        # ---- FlameTex
        mean, basis = RT.synthetic_space(S, SEED, SOURCE, N_TEX)
        T = TX.FlameTex(N_TEX, SOURCE, UV)
        T.load_state_dict({'texture_mean': mean, 'texture_basis': basis})
        T = T.cuda()
        del mean, basis
        code = S.counter_tensor(SEED, 'tt.code', (B, N_TEX)).cuda()

        def stock_tex(c):
            t = T.texture_mean + (T.texture_basis * c[:, None, :]).sum(-1)
            t = F.interpolate(t.reshape(c.shape[0], SOURCE, SOURCE, 3).permute(0, 3, 1, 2), [UV, UV])
            return t[:, [2, 1, 0], :, :]

        a = T(code)
        b = torch.cat([stock_tex(code[i:i + 4]) for i in range(0, B, 4)])           # four rows at a time: the product of 32 takes 5 GB
        lines.append('FlameTex albedo: HIP vs stock max |diff| %.2e (max |albedo| %.2f)' % (float((a - b).abs().max()), float(b.abs().max())))
        del b
        h, s = event_ms([lambda: T(code), lambda: stock_tex(code)], steps)
        nbytes = 4 * ((1 + N_TEX) * 3 * UV * UV + B * 3 * UV * UV)
        report('FlameTex', h, s, '; %.1f MB a call (the pack once, the albedo out): %.2f TB/s = %.0f %% of the %.2f TB/s copy rate'
               % (nbytes / 1e6, nbytes / h / 1e9, 100.0 * nbytes / h / 1e9 / HBM_COPY_TBS, HBM_COPY_TBS))
        one, = event_ms([lambda: T(code[:1])], steps)
        nb1 = 4 * ((1 + N_TEX) * 3 * UV * UV + 3 * UV * UV)
        lines.append('%-16s HIP %8.3f ms at batch 1: %.2f TB/s (the pack of %.1f MB fits the 256 MB infinity cache, so repeated calls need not '
                     'come from HBM)' % ('FlameTex', one, nb1 / one / 1e9, nb1 / 1e6))
        from stylegan_directions_face_reenactment_amd import _native as N
        packs = [T.packed().clone() for _ in range(8)]
        outs = [torch.empty_like(a) for _ in range(8)]
        turn = [0]

        def rotating():
            i = turn[0] = (turn[0] + 1) % 8
            N.call('sgdfr_flametex_forward_f32', N.ptr(code), B, N.ptr(packs[i]), UV, N_TEX, N.ptr(outs[i]), N.stream())

        cold = event_ms([lambda: [rotating() for _ in range(8)]], steps, warm=2)[0] / 8
        lines.append('%-16s HIP %8.3f ms a batch, the launch alone, eight back to back over eight packs and outputs in turn (524 MB, beyond the '
                     'cache; no host time between the launches): %.2f TB/s = %.0f %% of the copy rate'
                     % ('FlameTex', cold, nbytes / cold / 1e9, 100.0 * nbytes / cold / 1e9 / HBM_COPY_TBS))
        turn[0] = 0
        c1 = code[:1].contiguous()
        one_cold = event_ms([lambda: [N.call('sgdfr_flametex_forward_f32', N.ptr(c1), 1, N.ptr(packs[i]), UV, N_TEX, N.ptr(outs[i]), N.stream())
                                      for i in range(8)]], steps, warm=2)[0] / 8
        lines.append('%-16s HIP %8.3f ms at batch 1, measured the same way: %.2f TB/s = %.0f %% of the copy rate'
                     % ('FlameTex', one_cold, nb1 / one_cold / 1e9, 100.0 * nb1 / one_cold / 1e9 / HBM_COPY_TBS))
        rotating()
        assert torch.equal(outs[1], a)
        del packs, outs
        albedo = a
        tex_ms = h

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
        mask = (S.counter_tensor(SEED, 'tt.mask', (UV, UV)) > -0.7).float()
        L = DT.UvLayout(faces, uv, faces, UV, mask, torch.zeros(UV, UV), n_vertices=n * n)
        topo = SR.MeshTopology(faces, n * n)
        verts = torch.tensor(verts, dtype=torch.float32).cuda()
        cam = torch.tensor([[8.0, 0.0, 0.0]]).repeat(B, 1).cuda()
        fd, pix, bary, maskd, _, face_uv = L.tables('cuda')
        light = S.counter_tensor(SEED, 'tt.light', (B, 9, 3), 0.0, 0.3).cuda()
        light[:, 0] += 2.5
        uvn = F.normalize(S.counter_tensor(SEED, 'tt.uvn', (B, 3, UV, UV)), dim=1).cuda()
        images = S.counter_tensor(SEED, 'tt.images', (B, 3, SIZE, SIZE), 0.5, 0.2).cuda()
        trans = TX.orth_proj(verts, cam).contiguous()
        consts = torch.tensor(SR.SH_CONSTANTS, device='cuda')

        def stock_sh(N, l):
            sh = torch.stack([N[:, 0] * 0. + 1., N[:, 0], N[:, 1], N[:, 2], N[:, 0] * N[:, 1], N[:, 0] * N[:, 2], N[:, 1] * N[:, 2],
                              N[:, 0] ** 2 - N[:, 1] ** 2, 3 * (N[:, 2] ** 2) - 1], 1) * consts[None, :, None, None]
            return torch.sum(l[:, :, :, None, None] * sh[:, :, None, :, :], 1)

        # ---- UV pass
        tri = fd.long()[pix.long().clamp(min=0)]
        w = torch.where((pix >= 0)[..., None], bary, torch.zeros((), device='cuda'))

        def stock_uv():
            shading = stock_sh(uvn, light)
            texture = albedo * shading
            att = trans[:, tri]
            pv = w[None, ..., 0, None] * att[..., 0, :] + w[None, ..., 1, None] * att[..., 1, :] + w[None, ..., 2, None] * att[..., 2, :]
            gt = F.grid_sample(images, pv[..., :2], mode='bilinear', padding_mode='zeros', align_corners=False)
            return shading, texture, gt * maskd + texture * (1 - maskd) * 0.7

        hip_uv = lambda: TX.uv_textures(L, albedo, uvn, light, trans, images)
        a, b = hip_uv(), stock_uv()
        lines.append('UV pass: HIP vs stock max |diff| uv_shading %.2e, uv_texture %.2e, uv_texture_gt %.2e'
                     % tuple(float((a[k] - t).abs().max()) for k, t in zip(('uv_shading', 'uv_texture', 'uv_texture_gt'), b)))
        h, s = event_ms([hip_uv, stock_uv], steps)
        report('UV texture pass', h, s)
        uv_ms = h

        # ---- textured render
        want = ('images', 'albedo_images', 'alpha_images', 'pos_mask', 'shading_images', 'grid', 'normal_images', 'normals', 'transformed_normals')
        hip_r = lambda: SR.render_texture(verts, topo, L, albedo, lights=light, cam=cam, size=SIZE, want=want)
        hip_i = lambda: SR.render_texture(verts, topo, L, albedo, lights=light, cam=cam, size=SIZE, want=('images',))
        P = trans.clone()
        raster = lambda: SR.rasterize(P, topo, SIZE)
        normals = SR.vertex_normals(verts, topo)

        def stock_epilogue():
            p, covered = p2f.long(), p2f >= 0
            wb = torch.where(covered[..., None], bry, torch.zeros((), device='cuda'))
            rows = torch.arange(B, device='cuda')[:, None, None, None]
            t3 = fd.long()[p.clamp(min=0)]
            fu = face_uv[p.clamp(min=0)]
            g = wb[..., 0, None] * fu[..., 0, :] + wb[..., 1, None] * fu[..., 1, :] + wb[..., 2, None] * fu[..., 2, :]
            Nw = (wb[..., None] * normals[rows, t3]).sum(-2).permute(0, 3, 1, 2)
            al = F.grid_sample(albedo, g, mode='bilinear', padding_mode='zeros', align_corners=False)
            sh = stock_sh(Nw, light)
            alpha = covered[:, None].float()
            return al * sh * alpha, al * alpha, sh, g, Nw * alpha

        P[:, :, 2] += 10.0
        p2f, _, bry = raster()
        a, b = hip_r(), stock_epilogue()
        lines.append('textured render: HIP vs stock max |diff| images %.2e, shading_images %.2e (%.2f of the pixels covered)'
                     % (float((a['images'] - b[0]).abs().max()), float((a['shading_images'] - b[2]).abs().max()), float((p2f >= 0).float().mean())))
        hr, hi, hraster, s = event_ms([hip_r, hip_i, raster, stock_epilogue], steps)
        lines.append('%-16s HIP all nine outputs %8.3f ms a batch = %.4f ms a frame; images alone %8.3f ms; rasterize alone (3 launches, no normals) '
                     '%8.3f ms; stock fp32 epilogue on the rasteriser\'s outputs (no raster, no normals) %8.3f ms a batch'
                     % ('textured render', hr, hr / B, hi, hraster, s))
        lines.append('%-16s what the textured epilogue and the two normal launches add to the rasterisation: %.3f ms a batch against %.3f ms stock '
                     '(HIP/stock %.3f)' % ('', hr - hraster, s, (hr - hraster) / s))
        total = tex_ms + uv_ms + hr
    lines.append('the texture side takes %.3f ms a batch = %.4f ms a frame (FlameTex, the UV pass, the textured render with every output)'
                 % (total, total / B))
    print('\n'.join(lines))
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

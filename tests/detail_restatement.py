"""DECA's detail path behind the rasteriser restated in torch on the CPU (float64, or float32 to measure what the number format alone
costs): the rules of include/sgdfr.h for sgdfr_detail_* and sgdfr_shaperender_detail_f32.

    generate_triangles    util.generate_triangles(h, w) written as the reference's two loops
    decoder_chain         D_detail as a plain torch chain on folded weights (F.interpolate + F.conv2d), every stage output
    world2uv              SRenderY.world2uv on a given UV table
    displacement2normal   DECA.displacement2normal via shape_render_restatement.reference_order_normals on the dense faces
    grid                  ops['grid']: the interpolated UV coordinate of a pixel
    grid_sample           F.grid_sample(bilinear, zeros, align_corners=False) written out; tests pin it to F.grid_sample itself
    detail_shade          render_shape with detail_normal_images on top of shape_render_restatement.render
    seam_atlas            a UV atlas for shape_render_cases.smooth_grid with a seam, an empty region and an island in the margin

pytorch3d is not installed: the face decisions (the UV table, pix_to_face) are inputs here, and the rasteriser's own rules are the
ones tests/shape_render_restatement.py states.
"""
import numpy as np
import torch
import torch.nn.functional as F

import shape_render_restatement as R

CHANNELS = ((128, 128), (128, 64), (64, 64), (64, 32), (32, 16))
SLOPE = 0.2


# kat22 (scripts/make_golden_detail.py SUB, BORDER, BATCHES): what the fixture samples of each of the seven decoder stages
SUB = ((4, 1), (8, 2), (8, 4), (8, 8), (8, 16), (4, 16), (1, 8))
BORDER = (16, 16, 8, 8, 8, 4, 1)
BATCHES = (('b1', 1), ('b3', 3))


def keys_of(module):
    return ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in module.state_dict().items()]


def stage_errors(g, tag, stages):
    """Per stage (sample, border, plane sums) deviations of `stages` (seven tensors [B,C,H,W]) from kat22, with the stage's dev."""
    out = []
    for s, x in enumerate(stages):
        x = x.detach().double().cpu()
        cs, ss = SUB[s]
        xb = x[:, ::BORDER[s]]
        brd = torch.stack([xb[:, :, 0, :], xb[:, :, -1, :], xb[:, :, :, 0], xb[:, :, :, -1]], 2)
        e_sub = float((x[:, ::cs, ::ss, ::ss] - torch.from_numpy(g['sub_%d_%s' % (s, tag)]).double()).abs().max())
        e_brd = float((brd - torch.from_numpy(g['border_%d_%s' % (s, tag)]).double()).abs().max())
        e_sum = float((x.sum((2, 3)) - torch.from_numpy(g['sums_%d_%s' % (s, tag)])).abs().max())
        out.append((e_sub, e_brd, e_sum, float(g['dev_%d_%s' % (s, tag)]), x.shape[2] * x.shape[3]))
    return out


def generate_triangles(h, w, margin_x=2, margin_y=5):
    tri = []
    for x in range(margin_x, w - 1 - margin_x):
        for y in range(margin_y, h - 1 - margin_y):
            tri.append([y * w + x, y * w + x + 1, (y + 1) * w + x])
            tri.append([y * w + x + 1, (y + 1) * w + x + 1, (y + 1) * w + x])
    return np.array(tri, dtype=np.int64)[:, [0, 2, 1]]


def decoder_chain(folded, latent, out_scale=0.01, dtype=torch.float64):
    """folded: the 14 tensors of DetailDecoder.folded(); latent [B,181] -> (uv_z [B,1,256,256], [the Linear's output [B,128,8,8], the
    five layers' outputs])."""
    p = [t.to(dtype) for t in folded]
    x = F.linear(latent.to(dtype), p[0], p[1]).view(-1, 128, 8, 8)
    taps = [x]
    for i in range(len(CHANNELS)):
        x = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
        x = F.leaky_relu(F.conv2d(x, p[2 + 2 * i], p[3 + 2 * i], padding=1), SLOPE)
        taps.append(x)
    return torch.tanh(F.conv2d(x, p[12], p[13], padding=1)) * out_scale, taps


def upconv(x, w, b, slope, up, dtype=torch.float64):
    x = x.to(dtype)
    if up:
        x = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
    return F.leaky_relu(F.conv2d(x, w.to(dtype), b.to(dtype), padding=1), slope)


def uv_vertices(uvcoords, dtype=torch.float64):
    """renderer.py:101-103: (2u - 1, -(2v - 1), 1)"""
    uv = torch.as_tensor(uvcoords).to(dtype)
    return torch.stack([2 * uv[:, 0] - 1, -(2 * uv[:, 1] - 1), torch.ones_like(uv[:, 0])], 1)


def world2uv(values, faces, pix, bary, dtype=torch.float64):
    """values [B,V,3], the UV table pix [S,S] (-1: none) and bary [S,S,3] -> [B,3,S,S]"""
    v = torch.as_tensor(values).to(dtype)
    faces = torch.as_tensor(faces).long()
    pix = torch.as_tensor(pix).long()
    covered = pix >= 0
    tri = faces[pix.clamp(min=0)]                                                        # [S,S,3]
    w = torch.where(covered[..., None], torch.as_tensor(bary).to(dtype), torch.zeros((), dtype=dtype))
    att = v[:, tri]                                                                      # [B,S,S,3 corners,3]
    out = w[None, ..., 0, None] * att[..., 0, :] + w[None, ..., 1, None] * att[..., 1, :] + w[None, ..., 2, None] * att[..., 2, :]
    return out.permute(0, 3, 1, 2)


def displacement2normal(uv_z, verts, normals, faces, pix, bary, mask, fixed, dtype=torch.float64):
    """-> (uv_detail_normals [B,3,S,S], dense vertices [B,S*S,3], the length of the un-normalised normal [B,S,S])"""
    uv_v = world2uv(verts, faces, pix, bary, dtype)
    uv_n = world2uv(normals, faces, pix, bary, dtype)
    B, _, S, _ = uv_v.shape
    z = torch.as_tensor(uv_z).to(dtype) * torch.as_tensor(mask).to(dtype)
    P = uv_v + z * uv_n + torch.as_tensor(fixed).to(dtype)[None, None] * uv_n
    dense = P.permute(0, 2, 3, 1).reshape(B, -1, 3)
    tri = torch.from_numpy(generate_triangles(S, S))
    n = R.reference_order_normals(dense, tri, dtype)
    # the un-normalised length, for the conditioning rule of the tests
    raw = torch.zeros_like(dense)
    for k in range(3):
        raw.index_add_(1, tri[:, k], R._corner_cross(dense, tri, k))
    return n.reshape(B, S, S, 3).permute(0, 3, 1, 2), dense, raw.norm(dim=-1).reshape(B, S, S)


def grid(pix, bary, face_uv, dtype=torch.float64):
    """pix [B,S,S], bary [B,S,S,3], face_uv [F,3,2] -> [B,S,S,2]; (0, 0) where no face covers"""
    pix = torch.as_tensor(pix).long()
    covered = pix >= 0
    w = torch.where(covered[..., None], torch.as_tensor(bary).to(dtype), torch.zeros((), dtype=dtype))
    uv = torch.as_tensor(face_uv).to(dtype)[pix.clamp(min=0)]                            # [B,S,S,3,2]
    return w[..., 0, None] * uv[..., 0, :] + w[..., 1, None] * uv[..., 1, :] + w[..., 2, None] * uv[..., 2, :]


def grid_sample(inp, g):
    """inp [B,C,H,W], g [B,h,w,2] -> [B,C,h,w]: bilinear, zero padding, align_corners False"""
    B, C, H, W = inp.shape
    ix = ((g[..., 0] + 1) * W - 1) / 2
    iy = ((g[..., 1] + 1) * H - 1) / 2
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros((B, C) + tuple(g.shape[1:3]), dtype=inp.dtype)
    rows = torch.arange(B)[:, None, None]
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            wx = (x0 + 1 - ix) if dx == 0 else (ix - x0)
            wy = (y0 + 1 - iy) if dy == 0 else (iy - y0)
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            v = inp[rows, :, y.clamp(0, H - 1).long(), x.clamp(0, W - 1).long()]          # [B,h,w,C]
            out += (v * (wx * wy * ok)[..., None]).permute(0, 3, 1, 2)
    return out


def detail_shade(r, face_uv, uv_normals, lights=None, images=None, dtype=torch.float64):
    """r: shape_render_restatement.render's dict (same dtype) -> {'grid', 'detail_normal_images', 'shape_detail'}"""
    pix, bary = r['pix_to_face'], r['bary']
    B, S = pix.shape[0], pix.shape[1]
    covered = pix >= 0
    g = grid(pix, bary, face_uv, dtype)
    N = grid_sample(torch.as_tensor(uv_normals).to(dtype), g) * covered[:, None].to(dtype)
    w = torch.where(covered[..., None], bary.to(dtype), torch.zeros((), dtype=dtype))
    albedo = w.sum(-1) * R.ALBEDO
    L = torch.as_tensor(R.DEFAULT_LIGHTS if lights is None else lights).to(dtype)
    L = (L[None] if L.ndim == 2 else L).expand(B, -1, -1)
    d = L[..., :3] / L[..., :3].norm(dim=-1, keepdim=True).clamp(min=1e-12)
    dots = torch.einsum('bcij,blc->bijl', N, d).clamp(0, 1)
    shading = torch.einsum('bijl,blc->bijc', dots, L[..., 3:]) / L.shape[1]
    alpha = r['alpha'].to(dtype)
    bg = torch.zeros(B, 3, S, S, dtype=dtype) if images is None else torch.as_tensor(images).to(dtype)
    shape = (albedo[..., None] * shading).permute(0, 3, 1, 2) * alpha + bg * (1 - alpha)
    return {'grid': g, 'detail_normal_images': N, 'shape_detail': shape}


def seam_atlas(faces, n=13, to_border=False):
    """A UV atlas for the n x n sheet of shape_render_cases.smooth_grid (its faces; vertex index row * n + column): two charts cut along the
    vertex column n // 2, whose vertices are listed twice (Vt = n n + n > V); the left chart fills u in [0, 0.475], v in [0, 1], into
    the margin util.generate_triangles leaves unmeshed; nothing maps to the strip 0.475 < u < 0.495 between the charts nor to v above
    0.975 on the right chart (empty regions: small, because a meshed texel whose whole neighbourhood is empty has a zero normal and
    counts as ill-conditioned in the tests).  A slight wobble keeps texel centres off the edges.  to_border: the right chart runs to
    u = 1 exactly, so pixels there sample the UV map across its border.  -> (uvcoords [Vt,2] float64, uvfaces [F,3] int64), corner
    by corner the faces given."""
    m = n // 2
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    wob = 0.004 * np.sin(1.7 * r + 0.9 * c)
    left_u = 0.475 * c / m + wob * ((c > 0) & (c < m))
    left_v = r / (n - 1) + 0.004 * np.sin(1.3 * c) * ((r > 0) & (r < n - 1))
    hi = 1.0 if to_border else 0.985
    right_u = 0.495 + (hi - 0.495) * (c - m) / (n - 1 - m) + wob * ((c > m) & (c < n - 1))
    right_v = 0.975 * r / (n - 1) + 0.004 * np.cos(1.1 * c) * (r > 0)
    uv = np.concatenate([np.stack([np.where(c <= m, left_u, right_u), np.where(c <= m, left_v, right_v)], -1).reshape(-1, 2),
                         np.stack([right_u[:, m], right_v[:, m]], -1)])                  # the seam column again, on the right chart
    faces = np.asarray(faces, dtype=np.int64)
    uvfaces = faces.copy()
    cols = faces % n
    right = cols.max(1) > m                                                              # a face of the right chart
    on_seam = right[:, None] & (cols == m)
    uvfaces[on_seam] = n * n + (faces[on_seam] // n)
    return torch.from_numpy(uv), torch.from_numpy(uvfaces)

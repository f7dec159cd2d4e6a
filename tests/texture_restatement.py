"""DECA's texture side restated in torch on the CPU (float64, or float32 to measure what the number format alone costs): the rules of
include/sgdfr.h for sgdfr_flametex_*, sgdfr_shaperender_texture_f32, sgdfr_shaperender_attr_f32, sgdfr_texture_uv_f32 and
sgdfr_flame_visofp_f32.

    flametex          FLAMETex.forward (models/FLAME.py:253-262) with the source and output sizes as arguments
    flametex_kept     the same values from the kept texels only (gather, then one matrix product): no 512 x 512 texture is formed
    sh_constants      the nine factors of renderer.py:114-119
    add_shlight       SRenderY.add_SHlight
    texture_render    SRenderY.forward behind shape_render_restatement.rasterize
    uv_textures       deca.py:180-181, 193-199 on a given UV table
    visofp            deca.py:143-148 on landmark corners and weights
    render_attr       SRenderY.render_normal behind the same rasteriser; render_depth: renderer.py:295-314 on top of it

grid_sample is the one pinned in detail_restatement.py.  pytorch3d is not installed: as there, the rasteriser's rules are the ones
tests/shape_render_restatement.py states.
"""
import numpy as np
import torch
import torch.nn.functional as F

import detail_restatement as RD
import shape_render_restatement as R

POS_Z = -0.05               # renderer.py:159
VIS_Z = 0.1                 # deca.py:147
SMALL = ((12, 6), (10, 4), (7, 5))      # source -> uv sizes of the small FlameTex cases
KAT_SEED = 20261215
KAT_BATCHES = (('b1', 1), ('b3', 3))
KAT_SUB = 8                 # kat23's strided sample: every 8th row and column


def synthetic_space(S, seed, source, n_tex):
    """Seeded texture_mean [1,1,source*source*3] around 0.5 and texture_basis [1,source*source*3,n_tex]."""
    n = source * source * 3
    key = 'flametex.%d.%d' % (source, n_tex)
    return S.counter_tensor(seed, key + '.mean', (1, 1, n), 0.5, 0.15), S.counter_tensor(seed, key + '.basis', (1, n, n_tex), 0.0, 0.03)


def flametex(mean, basis, code, source, uv, dtype=torch.float64):
    """FLAMETex.forward: the whole texture, F.interpolate (nearest), channels [2,1,0]."""
    mean, basis, code = mean.to(dtype), basis.to(dtype), code.to(dtype)
    t = mean + (basis * code[:, None, :]).sum(-1)
    t = t.reshape(code.shape[0], source, source, 3).permute(0, 3, 1, 2)
    t = F.interpolate(t, [uv, uv])
    return t[:, [2, 1, 0], :, :]


def interpolate_index(source, uv):
    """The source index F.interpolate(mode='nearest') keeps, read off F.interpolate itself."""
    ramp = torch.arange(source, dtype=torch.float32).view(1, 1, source, 1).expand(1, 1, source, source).contiguous()
    return F.interpolate(ramp, [uv, uv])[0, 0, :, 0].long()


def kept_rows(source, uv):
    """[uv,uv,3]: the row of texture_basis behind albedo[c, y, x]."""
    i = interpolate_index(source, uv)
    return ((i[:, None] * source + i[None, :]) * 3)[..., None] + torch.tensor([2, 1, 0])


def flametex_kept(mean, basis, code, source, uv, dtype=torch.float64):
    rows = kept_rows(source, uv)
    m = mean.reshape(-1)[rows].to(dtype)                                   # [uv,uv,3]
    b = basis.reshape(-1, basis.shape[-1])[rows].to(dtype)                 # [uv,uv,3,n_tex]
    return (m[..., None] + b @ code.to(dtype).T).permute(3, 2, 0, 1)


def digest(albedo):
    """What kat23 records of an albedo [B,3,uv,uv] (float64): the strided sample, the four border lines, the plane sums."""
    a = albedo.double()
    brd = torch.stack([a[:, :, 0, :], a[:, :, -1, :], a[:, :, :, 0], a[:, :, :, -1]], 2)
    return a[:, :, ::KAT_SUB, ::KAT_SUB], brd, a.sum((2, 3))


def sh_constants(dtype=torch.float64):
    pi = np.pi
    c = [1 / np.sqrt(4 * pi), ((2 * pi) / 3) * (np.sqrt(3 / (4 * pi))), ((2 * pi) / 3) * (np.sqrt(3 / (4 * pi))),
         ((2 * pi) / 3) * (np.sqrt(3 / (4 * pi))), (pi / 4) * (3) * (np.sqrt(5 / (12 * pi))), (pi / 4) * (3) * (np.sqrt(5 / (12 * pi))),
         (pi / 4) * (3) * (np.sqrt(5 / (12 * pi))), (pi / 4) * (3 / 2) * (np.sqrt(5 / (12 * pi))), (pi / 4) * (1 / 2) * (np.sqrt(5 / (4 * pi)))]
    return torch.tensor(c, dtype=torch.float64).float().to(dtype)          # the reference keeps them as float32


def add_shlight(normals, light, dtype=torch.float64):
    """normals [B,3,h,w], light [B,9,3] -> [B,3,h,w]"""
    N = normals.to(dtype)
    sh = torch.stack([N[:, 0] * 0. + 1., N[:, 0], N[:, 1], N[:, 2], N[:, 0] * N[:, 1], N[:, 0] * N[:, 2], N[:, 1] * N[:, 2],
                      N[:, 0] ** 2 - N[:, 1] ** 2, 3 * (N[:, 2] ** 2) - 1], 1)
    sh = sh * sh_constants(dtype)[None, :, None, None]
    return torch.sum(light.to(dtype)[:, :, :, None, None] * sh[:, :, None, :, :], 1)


def _interpolate(pix, bary, faces, values, dtype):
    """values [B,V,D] at the covering face's corners -> [B,S,S,D], 0 where none covers"""
    covered = pix >= 0
    tri = faces[pix.clamp(min=0)]
    w = torch.where(covered[..., None], bary.to(dtype), torch.zeros((), dtype=dtype))
    rows = torch.arange(pix.shape[0])[:, None, None, None]
    att = values.to(dtype)[rows, tri]                                      # [B,S,S,3 corners,D]
    return w[..., 0, None] * att[..., 0, :] + w[..., 1, None] * att[..., 1, :] + w[..., 2, None] * att[..., 2, :]


def texture_render(vertices, faces, S, face_uv, albedo, lights, cam=None, projected=None, dtype=torch.float64):
    """SRenderY.forward -> dict with the reference's outputs, pix_to_face / zbuf / bary, 'tz' (the interpolated transformed-normal z),
    'ambiguous' [B,S,S] (the rasteriser's edge and depth rules) and 'pos_ambiguous' (|tz + 0.05| < TOL on covered pixels)."""
    assert (cam is None) != (projected is None)
    v = torch.as_tensor(vertices).to(dtype)
    faces = torch.as_tensor(faces).long()
    P = R.project(v, cam, R.Z_OFFSET, dtype) if cam is not None else R.project(projected, None, R.Z_OFFSET, dtype)
    wn, tn = R.vertex_normals(v, faces, dtype), R.vertex_normals(P, faces, dtype)
    pix, zbuf, bary, amb = R.rasterize(P, faces, S, dtype)
    covered = pix >= 0
    alpha = covered[:, None].to(dtype)
    normal_images = _interpolate(pix, bary, faces, wn, dtype).permute(0, 3, 1, 2)
    tz = _interpolate(pix, bary, faces, tn, dtype)[..., 2]
    grid = RD.grid(pix, bary, face_uv, dtype)
    out = {'alpha_images': alpha, 'pos_mask': (tz < POS_Z)[:, None].to(dtype), 'grid': grid, 'normals': wn, 'transformed_normals': tn,
           'normal_images': normal_images * alpha, 'pix_to_face': pix, 'zbuf': zbuf, 'bary': bary, 'tz': tz, 'ambiguous': amb,
           'pos_ambiguous': covered & ((tz - POS_Z).abs() < R.TOL)}
    if albedo is not None:
        albedo_images = RD.grid_sample(torch.as_tensor(albedo).to(dtype), grid)
        out['albedo_images'] = albedo_images * alpha
    if lights is not None:
        out['shading_images'] = add_shlight(normal_images, lights, dtype)
        if albedo is not None:
            out['images'] = albedo_images * out['shading_images'] * alpha
    else:
        out['shading_images'] = torch.zeros_like(normal_images)
        if albedo is not None:
            out['images'] = albedo_images * alpha
    return out


def uv_textures(albedo, uv_normals, light, trans_verts, images, faces, pix, bary, mask, dtype=torch.float64):
    """-> dict: uv_shading, uv_texture (with an albedo), uv_pverts, uv_gt, uv_texture_gt"""
    shading = add_shlight(uv_normals, light, dtype)
    pverts = RD.world2uv(trans_verts, faces, pix, bary, dtype)
    gt = RD.grid_sample(torch.as_tensor(images).to(dtype), pverts.permute(0, 2, 3, 1)[..., :2])
    m = torch.as_tensor(mask).to(dtype)
    out = {'uv_shading': shading, 'uv_pverts': pverts, 'uv_gt': gt}
    if albedo is not None:
        out['uv_texture'] = albedo.to(dtype) * shading
        out['uv_texture_gt'] = gt * m + (out['uv_texture'] * (1 - m) * 0.7)
    else:
        out['uv_texture_gt'] = gt * m + (torch.ones_like(gt) * (1 - m) * 0.7)
    return out


def visofp(normals, faces, lmk_faces_idx, lmk_bary, dtype=torch.float64):
    """-> (vis [B,n,1], the gathered z [B,n])"""
    tri = torch.as_tensor(faces).long()[torch.as_tensor(lmk_faces_idx).long()]           # [n,3]
    g = (normals.to(dtype)[:, tri] * torch.as_tensor(lmk_bary).to(dtype)[None, :, :, None]).sum(2)
    return (g[:, :, 2:] < VIS_Z).to(dtype), g[:, :, 2]


def render_attr(projected, values, faces, S, z_offset=0.0, dtype=torch.float64):
    """-> (out [B,D,S,S], ambiguous [B,S,S])"""
    faces = torch.as_tensor(faces).long()
    P = R.project(projected, None, z_offset, dtype)
    pix, _, bary, amb = R.rasterize(P, faces, S, dtype)
    return _interpolate(pix, bary, faces, torch.as_tensor(values), dtype).permute(0, 3, 1, 2), amb, pix


def render_depth(projected, faces, S, dtype=torch.float64):
    p = torch.as_tensor(projected).to(dtype).clone()
    p[:, :, 2] = p[:, :, 2] - p[:, :, 2].min()
    z = -p[:, :, 2:].clone()
    z = z - z.min()
    z = z / z.max()
    return render_attr(p, z, faces, S, R.Z_OFFSET, dtype)

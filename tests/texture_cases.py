"""Inputs of the texture tests, built on the CPU so that tests/test_cpu_texture.py can prove them usable (set-aside shares under the cap
in the restatement alone) before tests/test_gpu_texture.py runs them on a GPU.  Everything is seeded and float32-representable."""
import torch

from util import S, SEED
import detail_restatement as RD
import shape_render_cases as C
import shape_render_restatement as R

CAP = 0.02                  # the largest share of a map that may be set aside
# textured render: image size (a whole tile, a partial tile, several tiles), UV size, rows, the atlas running to the UV border
RENDER = [(16, 16, 1, False), (24, 40, 3, False), (40, 16, 3, True), (40, 40, 1, True), (16, 40, 3, True), (24, 16, 1, False)]
RENDER_IDS = ['S%d_Su%d_rows%d%s' % (c[0], c[1], c[2], '_border' if c[3] else '') for c in RENDER]
# UV pass: UV size, image size, with an albedo, the mask
UV = [(16, 8, True, 'mixed'), (24, 24, False, 'zero'), (40, 8, True, 'one'), (40, 24, False, 'mixed'), (16, 24, True, 'zero'), (24, 8, False, 'one')]
UV_IDS = ['Su%d_H%d_%s_%s' % (c[0], c[1], 'albedo' if c[2] else 'plain', c[3]) for c in UV]
ATTR_SIZES = (16, 24, 40)
N_LMK = 68


def sheet(rows, to_border=False):
    """smooth_grid (n = 13) with the seam atlas; the camera is drawn in to 0.85 so that the image corners stay uncovered."""
    verts, faces, cam = C.smooth_grid(5, rows=rows)
    cam = cam.clone()
    cam[:, 0] *= 0.85
    uv, uvfaces = RD.seam_atlas(faces, to_border=to_border)
    return verts, faces, cam, uv, uvfaces


def mask_of(kind, Su):
    if kind == 'zero':
        return torch.zeros(Su, Su)
    if kind == 'one':
        return torch.ones(Su, Su)
    return (S.counter_tensor(SEED, 'texture.mask.%d' % Su, (Su, Su)) > -0.7).float()


def maps(rows, Su, size=None):
    """Seeded albedo [rows,3,Su,Su] in (0, 1), SH lights [rows,9,3], unit UV normals and, with size, images [rows,3,size,size]."""
    albedo = S.counter_tensor(SEED, 'texture.albedo.%d' % Su, (rows, 3, Su, Su), 0.5, 0.2)
    light = S.counter_tensor(SEED, 'texture.light', (rows, 9, 3), 0.0, 0.5)
    light[:, 0] += 2.0
    uvn = S.counter_tensor(SEED, 'texture.uvn.%d' % Su, (rows, 3, Su, Su))
    uvn = uvn / uvn.norm(dim=1, keepdim=True)
    images = None if size is None else S.counter_tensor(SEED, 'texture.images.%d' % size, (rows, 3, size, size), 0.5, 0.2)
    return albedo, light, uvn, images


def uv_table(uv, uvfaces, Su):
    """The UV table of the restatement's own rasterisation (the CPU stand-in for UvLayout.tables): pix [Su,Su], bary float32."""
    pix, _, bary, amb = R.rasterize(RD.uv_vertices(uv).float().double()[None], uvfaces, Su)
    return pix[0], bary[0].float(), amb[0]


def landmarks(n_faces):
    """68 landmarks spread over the faces with seeded positive weights."""
    idx = (torch.arange(N_LMK) * 7) % n_faces
    w = S.counter_tensor(SEED, 'texture.lmk', (N_LMK, 3)).abs() + 0.05
    return idx, w / w.sum(1, keepdim=True)


def stacked(rows=1):
    """stacked_quads as projected vertices [rows,8,3] (float32), the rows at different depths, with seeded per-vertex values."""
    out = []
    for far, near in ((2.0, 1.0), (3.0, 0.5))[:rows]:
        v, faces = C.stacked_quads(far, near)
        out.append(v)
    values = S.counter_tensor(SEED, 'texture.stacked.values', (rows, 8, 3))
    return torch.stack(out).float(), faces, values


def sheet_projected(rows):
    """The sheet's projected vertices (z without the renderer's offset) and the normals of the projected mesh, float32; row 1 is
    half as deep again as the camera leaves it, so that the rows' z ranges differ."""
    verts, faces, cam, _, _ = sheet(rows)
    p = R.project(verts, cam, 0.0, torch.float32)
    if rows > 1:
        p[1, :, 2] *= 1.5
    return p, faces, R.vertex_normals(p, faces).float()

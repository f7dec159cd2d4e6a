"""The shape renderer restated in torch on the CPU (float64, or float32 to measure what the number format alone costs): the rules
of include/sgdfr.h for sgdfr_shaperender_*, written out pixel by pixel with every face of a pixel block at once.

    project          batch_orth_proj with DECA's y / z flip and the renderer's z offset
    csr              the vertex -> (face, corner) table, built the slow and obvious way
    vertex_normals   the per-corner cross products summed per vertex, n / max(|n|, 1e-6)
    reference_order_normals   the same sum in the order the reference adds it (corner 1 of every face, corner 2, corner 0)
    rasterize        coverage, depth, the winner and -- in float64 -- the pixels a float32 rasteriser may decide differently
    render           the shaded panel on top of rasterize

The rasteriser's rules restate pytorch3d's documented behaviour at blur_radius 0, one face per pixel, no perspective correction; they
are not pinned against pytorch3d.  On equal depth the lower face index wins: this project's rule, not pytorch3d's.

Pixels are visited in blocks of `block` x `block`; a face is left out of a block when its bounding box, grown by `margin`, misses
every centre of the block.  Such a face cannot cover a centre there, nor come within the ambiguity threshold of one: with
w'_i = edge_i / area the centre is p = sum w'_i v_i and sum w'_i = 1, and w_i = w'_i area / (area + 1e-8) with that factor above 1/2
for |area| > 1e-8, so all w_i > -1e-4 puts p within 4e-4 of the box's extent beyond the box; margin is one pixel plus 1e-3 of the
largest coordinate span.
"""
import numpy as np
import torch

AREA_EPS = 1e-8
TOL = 1e-4                  # ambiguity threshold: about 100 x the float32 error of a barycentric (a few ulp of 1)
ALBEDO = 180.0 / 255.0
FRONT_Z = 0.15
Z_OFFSET = 10.0
DEFAULT_LIGHTS = [[x, y, z, 1.7, 1.7, 1.7] for x, y, z in ((-1, 1, 1), (1, 1, 1), (-1, -1, 1), (1, -1, 1), (0, 0, 1))]


def project(vertices, cam=None, z_offset=Z_OFFSET, dtype=torch.float64):
    """cam [B,3] = (s, tx, ty): X = s (x + tx), Y = -s (y + ty), Z = -s z + z_offset;  no cam: Z + z_offset only."""
    v = torch.as_tensor(vertices).to(dtype)
    if cam is None:
        return torch.stack([v[..., 0], v[..., 1], v[..., 2] + z_offset], -1)
    c = torch.as_tensor(cam).to(dtype)
    s, tx, ty = c[:, None, 0], c[:, None, 1], c[:, None, 2]
    return torch.stack([s * (v[..., 0] + tx), -(s * (v[..., 1] + ty)), -(s * v[..., 2]) + z_offset], -1)


def csr(faces, n_vertices):
    """offsets [V+1], entries = face * 3 + corner per vertex, by face and then corner."""
    per_vertex = [[] for _ in range(n_vertices)]
    for f, tri in enumerate(np.asarray(faces).tolist()):
        for k, v in enumerate(tri):
            per_vertex[v].append(f * 3 + k)
    offsets = np.zeros(n_vertices + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(p) for p in per_vertex])
    return offsets, np.array([e for p in per_vertex for e in p], dtype=np.int64)


def _corner_cross(v, faces, k):
    o, a, b = (v[:, faces[:, (k + i) % 3]] for i in range(3))
    return torch.cross(a - o, b - o, dim=-1)


def _unit(n):
    return n / n.norm(dim=-1, keepdim=True).clamp(min=1e-6)


def vertex_normals(vertices, faces, dtype=torch.float64):
    """[B,V,3] -> [B,V,3]: corner k of a face adds (v[k+1] - v[k]) x (v[k+2] - v[k]) to its vertex, faces in order, corners in order."""
    v = torch.as_tensor(vertices).to(dtype)
    faces = torch.as_tensor(faces).long()
    n = torch.zeros_like(v)
    cross = torch.stack([_corner_cross(v, faces, k) for k in range(3)], 2)              # [B,F,3 corners,3]
    n.index_add_(1, faces.reshape(-1), cross.reshape(v.shape[0], -1, 3))
    return _unit(n)


def reference_order_normals(vertices, faces, dtype=torch.float64):
    """The sum as libs/DECA/decalib/utils/util.py:193-225 orders it: all corners 1, then all corners 2, then all corners 0, over the
    batch flattened into one vertex list."""
    v = torch.as_tensor(vertices).to(dtype)
    faces = torch.as_tensor(faces).long()
    B, V = v.shape[:2]
    flat = v.reshape(B * V, 3)
    shifted = (faces[None] + (torch.arange(B) * V)[:, None, None]).reshape(-1, 3)
    tri = flat[shifted]                                                                 # [B F, 3, 3]
    n = torch.zeros_like(flat)
    for k in (1, 2, 0):
        n.index_add_(0, shifted[:, k], torch.cross(tri[:, (k + 1) % 3] - tri[:, k], tri[:, (k + 2) % 3] - tri[:, k], dim=-1))
    return _unit(n).reshape(B, V, 3)


def centres(S, dtype=torch.float64):
    """centre coordinate of pixel index 0..S-1 along either axis: (2 j + 1) / S - 1"""
    return (2 * torch.arange(S) + 1).to(dtype) / S - 1


def _edge(px, py, ux, uy, vx, vy):
    return (px - ux) * (vy - uy) - (py - uy) * (vx - ux)


def rasterize_one(P, faces, S, dtype=torch.float64, block=16):
    """One image: P [V,3] projected vertices -> pix_to_face [S,S] (int64, -1: none), zbuf, bary [S,S,3] (-1 where none), ambiguous
    [S,S] bool (edge and depth rules)."""
    P = torch.as_tensor(P).to(dtype)
    faces = torch.as_tensor(faces).long()
    a, b, c = P[faces[:, 0]], P[faces[:, 1]], P[faces[:, 2]]
    area = _edge(c[:, 0], c[:, 1], a[:, 0], a[:, 1], b[:, 0], b[:, 1])
    keep = (area.abs() > AREA_EPS) & ~((a[:, 2] < 0) & (b[:, 2] < 0) & (c[:, 2] < 0))
    xy = torch.stack([a[:, :2], b[:, :2], c[:, :2]], 1)
    lo, hi = xy.min(1).values, xy.max(1).values
    span = float((hi - lo).max()) if len(faces) else 0.0
    margin = 2.0 / S + 1e-3 * span
    ctr = centres(S, dtype)
    pix = torch.full((S, S), -1, dtype=torch.long)
    zbuf = torch.full((S, S), -1.0, dtype=dtype)
    bary = torch.full((S, S, 3), -1.0, dtype=dtype)
    amb = torch.zeros((S, S), dtype=torch.bool)
    for i0 in range(0, S, block):
        for j0 in range(0, S, block):
            ys, xs = ctr[i0:i0 + block], ctr[j0:j0 + block]
            sel = keep & (lo[:, 0] - margin <= xs[-1]) & (hi[:, 0] + margin >= xs[0]) & (lo[:, 1] - margin <= ys[-1]) & (hi[:, 1] + margin >= ys[0])
            ids = torch.nonzero(sel)[:, 0]
            if len(ids) == 0:
                continue
            py, px = (t.reshape(-1, 1) for t in torch.meshgrid(ys, xs, indexing='ij'))
            A, B_, C = a[ids], b[ids], c[ids]
            den = area[ids] + AREA_EPS
            w0 = _edge(px, py, B_[:, 0], B_[:, 1], C[:, 0], C[:, 1]) / den
            w1 = _edge(px, py, C[:, 0], C[:, 1], A[:, 0], A[:, 1]) / den
            w2 = _edge(px, py, A[:, 0], A[:, 1], B_[:, 0], B_[:, 1]) / den
            z = w0 * A[:, 2] + w1 * B_[:, 2] + w2 * C[:, 2]
            cand = (w0 > 0) & (w1 > 0) & (w2 > 0) & (z >= 0)
            zc = torch.where(cand, z, torch.full_like(z, float('inf')))
            zmin = zc.min(1).values
            first = torch.where(zc == zmin[:, None], torch.arange(len(ids))[None], len(ids)).min(1).values      # lowest index at the minimum
            hit = torch.isfinite(zmin)
            first = first.clamp(max=len(ids) - 1)
            rows = torch.arange(len(px))
            shape = (len(ys), len(xs))
            blk = (slice(i0, i0 + block), slice(j0, j0 + block))
            pix[blk] = torch.where(hit, ids[first], torch.full_like(first, -1)).reshape(shape)
            zbuf[blk] = torch.where(hit, zmin, torch.full_like(zmin, -1.0)).reshape(shape)
            wsel = torch.stack([w0[rows, first], w1[rows, first], w2[rows, first]], -1)
            bary[blk] = torch.where(hit[:, None], wsel, torch.full_like(wsel, -1.0)).reshape(shape + (3,))
            wmin = torch.minimum(torch.minimum(w0, w1), w2)
            near_edge = (wmin.abs() < TOL).any(1)
            two = torch.topk(zc, min(2, zc.shape[1]), dim=1, largest=False).values
            near_depth = (two[:, -1] - two[:, 0] < TOL) & torch.isfinite(two[:, -1]) if two.shape[1] == 2 else torch.zeros_like(hit)
            amb[blk] = (near_edge | near_depth).reshape(shape)
    return pix, zbuf, bary, amb


def rasterize(P, faces, S, dtype=torch.float64, block=16):
    """[B,V,3] -> pix_to_face [B,S,S], zbuf [B,S,S], bary [B,S,S,3], ambiguous [B,S,S]"""
    outs = [rasterize_one(p, faces, S, dtype, block) for p in torch.as_tensor(P)]
    return tuple(torch.stack([o[k] for o in outs]) for k in range(4))


def render(vertices, faces, S, cam=None, projected=None, lights=None, images=None, dtype=torch.float64, block=16):
    """render_shape -> dict: shape [B,3,S,S], alpha [B,1,S,S], pix_to_face, zbuf, bary, tz [B,S,S], ambiguous [B,S,S] (the edge, depth
    and |Tz - 0.15| rules)."""
    assert (cam is None) != (projected is None)
    v = torch.as_tensor(vertices).to(dtype)
    faces = torch.as_tensor(faces).long()
    P = project(v, cam, Z_OFFSET, dtype) if cam is not None else project(projected, None, Z_OFFSET, dtype)
    wn = vertex_normals(v, faces, dtype)
    tn = vertex_normals(P, faces, dtype)
    pix, zbuf, bary, amb = rasterize(P, faces, S, dtype, block)
    B = v.shape[0]
    covered = pix >= 0
    tri = faces[pix.clamp(min=0)]                                                        # [B,S,S,3]
    w = torch.where(covered[..., None], bary, torch.zeros_like(bary))
    rows = torch.arange(B)[:, None, None, None]
    Nw = (w[..., None] * wn[rows, tri]).sum(-2)                                          # [B,S,S,3], not re-normalised
    tz = (w * tn[rows, tri][..., 2]).sum(-1)
    albedo = w.sum(-1) * ALBEDO
    L = torch.as_tensor(DEFAULT_LIGHTS if lights is None else lights).to(dtype)
    L = L[None] if L.ndim == 2 else L
    L = L.expand(B, -1, -1)
    d = L[..., :3] / L[..., :3].norm(dim=-1, keepdim=True).clamp(min=1e-12)
    dots = torch.einsum('bijc,blc->bijl', Nw, d).clamp(0, 1)
    shading = torch.einsum('bijl,blc->bijc', dots, L[..., 3:]) / L.shape[1]
    alpha = (covered & (tz < FRONT_Z)).to(dtype)
    bg = torch.zeros(B, 3, S, S, dtype=dtype) if images is None else torch.as_tensor(images).to(dtype)
    shape = (albedo[..., None] * shading).permute(0, 3, 1, 2) * alpha[:, None] + bg * (1 - alpha[:, None])
    amb = amb | (covered & ((tz - FRONT_Z).abs() < TOL))
    return {'shape': shape, 'alpha': alpha[:, None], 'pix_to_face': pix, 'zbuf': zbuf, 'bary': bary, 'tz': tz, 'ambiguous': amb}


def gan_range(shape):
    return shape.clamp(0, 1) * 2 - 1

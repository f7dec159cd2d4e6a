"""Inputs of the render-side seam tests (tests/test_gpu_render_seams.py), built on the CPU so that tests/test_cpu_render_seams.py can
prove, with the restatements alone, that they reach what they claim before a GPU sees them.  Everything is seeded and
float32-representable.

    UPCONV         (rows, Cin, Cout, h, w) of sgdfr_detail_upconv_f32, each run as `up` and as plain; plan_rules.detail_plan says
                   what a case reaches
    FLAMETEX_*     row counts, component counts and (source, uv) sizes of FLAMETex
    sampler_*      coordinates that steer grid_sample3 through sgdfr_texture_uv_f32 with a hand-made table
    UV_SIZES       the UV passes' small and tile-edge sizes, three rows
    (the lattice sizes 1, 8 and 17 are shape_render_cases.SMALL_SIZES)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from util import S, SEED
import detail_restatement as RD
import shape_render_restatement as R
import texture_cases as TC
import texture_restatement as RT

# ---------------------------------------------------------------------------------------------------------------- the layer kernel
UPCONV = [(2, 29, 16, 5, 3), (2, 29, 17, 5, 3), (3, 29, 65, 3, 5), (1, 15, 64, 1, 7), (2, 40, 80, 1, 1), (2, 72, 64, 6, 10),
          (1, 260, 64, 4, 4), (1, 1024, 16, 2, 2), (3, 7, 5, 11, 1), (1, 8, 16, 64, 64)]
UPCONV_IDS = ['%dx%dx%d_%dto%d' % (c[0], c[3], c[4], c[1], c[2]) for c in UPCONV]
SLOPES = (0.2, 1.0)                                          # the five layers' LeakyReLU, and none (the decoder's last conv)


def upconv_inputs(case):
    """x [rows,Cin,h,w], weight [Cout,Cin,3,3] scaled to unit output variance, bias [Cout]: the same for `up` and plain."""
    rows, cin, cout, h, w = case
    key = 'seams.upconv.%d.%d.%d.%d.%d' % case
    x = S.counter_tensor(SEED, key + '.x', (rows, cin, h, w))
    wt = S.counter_tensor(SEED, key + '.w', (cout, cin, 3, 3), 0.0, (2.0 / (9 * cin)) ** 0.5)
    b = S.counter_tensor(SEED, key + '.b', (cout,), 0.0, 0.1)
    return x, wt, b


def upconv_reference(case, up, dtype=torch.float64):
    """The stock chain before its activation (F.interpolate + F.conv2d); leaky_relu of it is the layer's output at any slope."""
    x, wt, b = upconv_inputs(case)
    return RD.upconv(x, wt, b, 1.0, up, dtype=dtype)


def border_masks(Ho, Wo):
    """(border rows, border columns, interior) of an Ho x Wo map as [Ho,Wo] masks; the first two share the corners."""
    r, c = torch.zeros(Ho, Wo, dtype=torch.bool), torch.zeros(Ho, Wo, dtype=torch.bool)
    r[0], r[-1], c[:, 0], c[:, -1] = True, True, True, True
    return (('border rows', r), ('border cols', c), ('interior', ~(r | c)))


# ---------------------------------------------------------------------------------------------------------------- FLAMETex
FLAMETEX_ROWS = (8, 9, 16, 17, 32, 33, 41)                  # one, two and four waves; a full group; a second group of 1 and of 9 rows
FLAMETEX_BASE = (12, 6, 9)                                  # source, uv, n_tex: 108 elements, one block of the 16-byte path
FLAMETEX_COMPONENTS = (1, 7, 8, 9, 16, 17, 200)             # around the prefetch depth of 8, and the bound of the LDS table
FLAMETEX_PATHS = ((7, 5), (13, 10), (14, 11), (17, 12))     # 75 (dword, 2 blocks), 300 (16-byte, 75 lanes), 363 (dword, 6), 432 (16-byte)
FLAMETEX_MAX_ROWS = max(FLAMETEX_ROWS)


def flametex_code(n_tex):
    """[41, n_tex]: the first `rows` rows are the code of a batch of `rows`; every row differs from every other."""
    return S.counter_tensor(SEED, 'seams.flametex.code.%d' % n_tex, (FLAMETEX_MAX_ROWS, n_tex))


def flametex_path(P):
    """(elements per lane, blocks of 64 lanes, live lanes of the last block) of the launch for P = 3 uv^2 elements from aligned
    buffers: 16-byte loads where P is a multiple of 4."""
    vec = 4 if P % 4 == 0 else 1
    lanes = P // vec
    return vec, -(-lanes // 64), lanes - 64 * ((lanes - 1) // 64)


def flametex_instance(rows):
    """(waves of the instance, groups of 8 x waves rows it walks)"""
    waves = 1 if rows <= 8 else 2 if rows <= 16 else 4
    return waves, -(-rows // (8 * waves))


# ---------------------------------------------------------------------------------------------------------------- the sampler
SAMPLER_IMAGES = ((4, 4), (5, 3), (1, 1))                   # H x W
SAMPLER_GENERAL = 64


def _dyadic(n):
    return n & (n - 1) == 0


def axis_coordinates(n):
    """[(tag, float32 coordinate)] along an axis of n texels, by the texel index ix = ((g + 1) n - 1) / 2 it stands for:
    'centre'    ix = j: the texel itself
    'edge'      g = -1, +1 (ix = -0.5, n - 0.5): one neighbour inside with weight 1/2
    'partial'   ix = -0.75, n - 0.25: one neighbour inside with weight 1/4
    'outside'   ix = -1.5, n + 0.5 (between one and two texels outside) and, where n is a power of two so that float32 holds them
                exactly, ix = -1 and ix = n (the inside neighbour's weight is exactly 0; the guard's own edge): nothing
    'far'       +-3, +-1e30: nothing;  'nonfinite'  +-inf, NaN: nothing"""
    g = lambda ix: (2.0 * ix + 1.0) / n - 1.0
    out = [('centre', g(j)) for j in range(n)]
    out += [('edge', -1.0), ('edge', 1.0), ('partial', g(-0.75)), ('partial', g(n - 0.25)), ('outside', g(-1.5)), ('outside', g(n + 0.5))]
    if _dyadic(n):
        out += [('outside', g(-1.0)), ('outside', g(float(n)))]
    out += [('far', 3.0), ('far', -3.0), ('far', 1e30), ('far', -1e30)]
    out += [('nonfinite', float('inf')), ('nonfinite', float('-inf')), ('nonfinite', float('nan'))]
    return [(t, float(np.float32(v))) for t, v in out]


def restated_index(g, n):
    """ix of the float32 coordinate g as grid_sample3 forms it: every operation rounded to float32, none fused."""
    g = torch.as_tensor(g, dtype=torch.float32)
    return ((g + 1.0) * float(n) - 1.0) * 0.5


ZERO_TAGS = ('outside', 'far', 'nonfinite')


def sampler_points(H, W):
    """Every x of axis_coordinates(W) with every y of axis_coordinates(H), then SAMPLER_GENERAL seeded points inside ->
    (xy [n,2] float32, tags [(tag x, tag y)]); a general point carries ('general', 'general')."""
    ax, ay = axis_coordinates(W), axis_coordinates(H)
    xy = [(x, y) for _, y in ay for _, x in ax]
    tags = [(tx, ty) for ty, _ in ay for tx, _ in ax]
    gen = S.counter_tensor(SEED, 'seams.sampler.general.%d.%d' % (H, W), (SAMPLER_GENERAL, 2), 0.0, 0.5).clamp(-0.98, 0.98)
    pts = torch.cat([torch.tensor(xy, dtype=torch.float32), gen])
    return pts, tags + [('general', 'general')] * SAMPLER_GENERAL


def sampler_image(H, W):
    return S.counter_tensor(SEED, 'seams.sampler.image.%d.%d' % (H, W), (1, 3, H, W), 0.5, 0.2)


def sampler_exact_centres(pts, tags, H, W):
    """[n] bool and the texel (row, column) of the points that sit on a texel centre in BOTH axes as float32 arithmetic sees them
    (the restated index is the integer itself): there the sample must be the texel, bit for bit.  Every centre of a power-of-two
    side qualifies, and the middle texel of an odd side (g = 0); (2j + 1)/3 - 1 or (2j + 1)/5 - 1 is no float32 number, and a
    point that merely lies near a centre is held to the bar of the general points."""
    ix, iy = restated_index(pts[:, 0], W), restated_index(pts[:, 1], H)
    both = torch.tensor([t == ('centre', 'centre') for t in tags])
    exact = both & (ix == ix.floor()) & (iy == iy.floor())
    return exact, iy.clamp(0, H - 1).long(), ix.clamp(0, W - 1).long()


def sampler_reference(H, W):
    """The float64 side of one image: F.grid_sample(bilinear, zeros, align_corners=False) at every point whose two tags ask for a
    value, 0 where a tag of ZERO_TAGS says nothing is sampled (F.grid_sample is never handed those), and the same from
    detail_restatement.grid_sample run in float32 (the project's d32) -> dict."""
    pts, tags = sampler_points(H, W)
    img = sampler_image(H, W)
    zero = torch.tensor([tx in ZERO_TAGS or ty in ZERO_TAGS for tx, ty in tags])
    safe = pts.clone()
    safe[zero] = 0.0
    ref = F.grid_sample(img.double(), safe.double().view(1, 1, -1, 2), mode='bilinear', padding_mode='zeros', align_corners=False)[0, :, 0]
    r32 = RD.grid_sample(img, safe.view(1, 1, -1, 2))[0, :, 0].double()
    ref[:, zero], r32[:, zero] = 0.0, 0.0
    exact, ty, tx = sampler_exact_centres(pts, tags, H, W)
    general = torch.tensor([t == ('general', 'general') for t in tags])
    return {'pts': pts, 'tags': tags, 'image': img, 'zero': zero, 'ref': ref, 'r32': r32, 'exact': exact, 'texel': (ty, tx),
            'general': general, 'seam': ~zero & ~general & ~exact}


def sampler_table(n, zero_vertex=False):
    """The hand-made UV table that hands vertex t to texel t: Su = ceil(sqrt(n)), V = F = Su^2, faces[f] = (f, f, f),
    pix_to_face[t] = t, bary[t] = (1, 0, 0).  The gather forms 1 v + 0 v + 0 v, which is v for a finite v and NaN for an infinite one;
    zero_vertex=True appends a vertex of zeros and makes faces[f] = (f, Z, Z), so that 1 v + 0 0 + 0 0 hands +-inf on as it is
    (V = Su^2 + 1; every index stays inside its table) -> (Su, V, faces int32 [F,3], pix int32 [Su,Su], bary [Su,Su,3])."""
    Su = max(1, int(math.ceil(math.sqrt(n))))
    F_ = Su * Su
    f = torch.arange(F_, dtype=torch.int32)
    other = torch.full_like(f, F_) if zero_vertex else f
    bary = torch.zeros(Su, Su, 3)
    bary[..., 0] = 1.0
    return Su, F_ + int(zero_vertex), torch.stack([f, other, other], 1).contiguous(), f.reshape(Su, Su).contiguous(), bary


def sampler_vertices(pts, Su, V):
    """trans_verts [1,V,3]: (x, y) of point t at vertex t, z = t (any finite number), zeros behind the last point."""
    tv = torch.zeros(1, V, 3)
    tv[0, :pts.shape[0], :2] = pts
    tv[0, :Su * Su, 2] = torch.arange(Su * Su, dtype=torch.float32)
    return tv


# ---------------------------------------------------------------------------------------------------------------- the UV passes
UV_SIZES = (13, 17, 33)                                      # the smallest size; one texel in a second tile; one in a third
UV_ROWS = 3
UV_IMAGE = 8
# per size: a meshed texel (y, x) whose normal needs cells its own tile reads through its halo from a neighbouring tile's texels,
# or None where no meshed texel has such a neighbour; and a covered texel of the last, one-texel-wide tile column and row
UV_HALO_TEXEL = {13: None, 17: None, 33: (16, 16)}
UV_LAST_TILE_TEXEL = {13: None, 17: (8, 16), 33: (16, 32)}


def meshed(Su):
    """The vertices util.generate_triangles(S, S) names: quads x in [2, S-3), y in [5, S-6)."""
    m = torch.zeros(Su, Su, dtype=torch.bool)
    m[5:Su - 5, 2:Su - 2] = True
    return m


def uv_inputs(Su):
    """The seam atlas sheet with three rows (three cameras): verts, faces, cam, uv, uvfaces, mask, fixed_dis, uv_z, the coarse
    normals and, for the texture pass, albedo, light, images and the projected vertices."""
    verts, faces, cam, uv, uvfaces = TC.sheet(UV_ROWS)
    mask = TC.mask_of('mixed', Su)
    fixed = S.counter_tensor(SEED, 'seams.fixed.%d' % Su, (Su, Su), 0.0, 0.003)
    uv_z = S.counter_tensor(SEED, 'seams.uvz.%d' % Su, (UV_ROWS, 1, Su, Su), 0.0, 0.01)
    normals = R.vertex_normals(verts, faces).float()
    albedo, light, _, images = TC.maps(UV_ROWS, Su, UV_IMAGE)
    tv = R.project(verts, cam, 0.0, torch.float32)
    return {'verts': verts, 'faces': faces, 'cam': cam, 'uv': uv, 'uvfaces': uvfaces, 'mask': mask, 'fixed': fixed, 'uv_z': uv_z,
            'normals': normals, 'albedo': albedo, 'light': light, 'images': images, 'tv': tv}


def uv_set_aside(raw, amb, Su):
    """What the UV tests set aside: ambiguous texels of the table and meshed texels whose un-normalised normal is shorter than
    1e-3 x the median over the meshed texels (test_gpu_detail's definition) -> ([rows,S,S] bool, share per row)."""
    m = meshed(Su)
    ill = m[None] & (raw < 1e-3 * raw[:, m].median())
    aside = amb[None] | ill
    return aside, aside.reshape(aside.shape[0], -1).double().mean(1)

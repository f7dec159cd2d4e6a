"""CPU: the case lists of tests/render_seam_cases.py reach what tests/test_gpu_render_seams.py runs them for, shown with the restated
rules (tests/plan_rules.py) and the float64 restatements alone, and every cap of the GPU tests holds for the reference before a GPU
sees a case.

    the layer kernel   plan_rules.detail_plan is launch_conv / plan_conv as the sources state them; the ten cases give the plans the
                       issue lists, reach all eight classes (tile 16 | 64) x (up | plain) x (whole | sliced) and all seven seam
                       classes; the four cases of test_gpu_detail.UPCONV_CASES reach none of the seven (the gap this closes)
    FLAMETex           the row counts sit on both sides of every instance and group edge, the component counts around the prefetch
                       depth and at the LDS bound, the sizes on both load paths with the block counts claimed; no nearest index is
                       the identity; no two code rows are equal
    the sampler        F.grid_sample gives exactly 0 where the lists say nothing is sampled, the texel where a centre is exact
    the UV passes      set-aside shares under the 2 % cap at 13, 17 and 33 on the restatement's own table; the named texels
    the lattice        the small sizes are exact (the proof is test_cpu_shape_render's)
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import S, SEED
import detail_restatement as RD
import plan_rules as P
import render_seam_cases as RS
import shape_render_cases as C
import shape_render_restatement as R
import texture_cases as TC
import texture_restatement as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'stylegan_directions_face_reenactment_amd', 'csrc')


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return re.sub(r'\s+', ' ', fh.read())


# ---------------------------------------------------------------------------------------------------------------- the layer kernel
def test_detail_rule_is_the_one_the_sources_state():
    d, t = _source('detail.hip'), _source('conv_tile.h')
    assert 'const int bn = a.N <= 16 ? 16 : 64;' in d
    assert 'plan_conv(M, a.N, a.K, bn, conv_tiles(M, a.N, bn))' in d
    assert 'constexpr int BM = 64, BK = 16, kThreads = 256;' in t
    assert 'int S = whole ? 1 : std::min(512 / std::max(tiles, 1), nchunks / 8);' in t
    assert 'S = std::max(1, std::min(S, 32));' in t
    assert 'p.cps = (nchunks + S - 1) / S; p.S = (nchunks + p.cps - 1) / p.cps;' in t
    assert 'return ((M + BM - 1) / BM) * ((N + bn - 1) / bn);' in t
    assert 'if (p.S > 1) { hipLaunchKernelGGL(detail_finish_kernel' in d


def _slices(p):
    return [p.cps] * (p.S - 1) + [p.last]


def test_the_ten_cases_give_the_plans_they_are_listed_for():
    """Each line is what the issue's table says of the case, re-derived from the restated rule."""
    plan = lambda c, up: P.detail_plan(*c, up)
    seams = lambda c, up: P.detail_seams(*c, up)
    a, b, c, d, e, f, g, h, i, j = RS.UPCONV
    for up in (True, False):
        p = plan(a, up)                                                     # tile 16, 17 chunks in 9 + 8, K tail 5, a tile over two rows
        assert (p.bn, p.chunks, _slices(p), p.ktail) == (16, 17, [9, 8], 5) and 'tile_over_rows' in seams(a, up)
        assert p.Ho * p.Wo == (60 if up else 15)
        p = plan(b, up)                                                     # one channel wider: tile 64 with 17 of 64 live
        assert (p.bn, p.nt, _slices(p)) == (64, 1, [9, 8]) and b[2] == 17
        p = plan(c, up)                                                     # two channel tiles, the second with one live channel, sliced
        assert (p.bn, p.nt, c[2] - 64, p.S > 1) == (64, 2, 1, True) and {'partial_last_channel_tile', 'tile_over_rows'} <= seams(c, up)
        p = plan(d, up)                                                     # one texel high, whole, K tail 7
        assert (p.S, p.ktail, d[3]) == (1, 7, 1)
        p = plan(e, up)                                                     # 1 x 1 source, 12 + 11, second channel tile with 16 live
        assert (_slices(p), p.nt, e[2] - 64, e[3:]) == ([12, 11], 2, 16, (1, 1))
        p = plan(f, up)                                                     # five slices 9, 9, 9, 9, 5
        assert _slices(p) == [9, 9, 9, 9, 5] and (p.Ho * p.Wo) % 64 == (48 if up else 60)
        p = plan(g, up)                                                     # asks for 18, ends with 17, the last of 3 chunks
        assert (p.asked, p.S, p.last) == (18, 17, 3)
        p = plan(h, up)                                                     # the cap of 32, at the channel bound
        assert (p.asked, p.S, h[1], p.bn) == (32, 32, 1024, 16) and 'cap_32' in seams(h, up)
        p = plan(i, up)                                                     # one texel wide, whole, K tail 15, three rows in one tile
        assert (p.S, p.ktail, i[4], p.bn) == (1, 15, 1, 16) and (p.M <= 64) == (not up) and i[0] == 3      # (plain)
        assert 'tile_over_rows' in seams(i, up)
        p = plan(j, up)                                                     # 256 / 64 pixel tiles, whole
        assert (p.mt, p.S, p.bn) == (256 if up else 64, 1, 16)
    assert P.detail_plan(*c, False).mt == 1 and c[0] == 3                   # plain: three rows in one tile; up: tiles over two rows
    assert P.detail_plan(*c, True).mt == 3


def test_the_ten_cases_reach_every_class_and_every_seam():
    classes, seams = set(), set()
    for case in RS.UPCONV:
        for up in (True, False):
            classes.add(P.detail_class(*case, up))
            seams |= P.detail_seams(*case, up)
            p = P.detail_plan(*case, up)
            assert p.S == 1 or p.S * p.M * case[2] <= 512 * 64 * 64        # the partials fit the workspace launch_conv checks
            assert P.detail_counts(*case, up) == (1, int(p.S > 1))
    assert classes == set(P.DETAIL_CLASSES) and len(P.DETAIL_CLASSES) == 8
    assert seams == set(P.DETAIL_SEAMS[:-1]) | {'source_h_1', 'source_w_1'}
    for up in (True, False):                                                # the K tail is met sliced and whole, on both tiles
        tails = {(P.detail_plan(*c, up).bn, P.detail_plan(*c, up).S > 1) for c in RS.UPCONV if P.detail_plan(*c, up).ktail}
        assert tails == {(16, True), (16, False), (64, True), (64, False)}


def test_the_four_existing_cases_reach_none_of_the_seams():
    """The statement of the gap: whole, whole, two even slices, nine even slices, and nothing else."""
    from test_gpu_detail import UPCONV_CASES
    assert len(UPCONV_CASES) == 4
    for up in (True, False):
        assert [_slices(P.detail_plan(*c, up)) for c in UPCONV_CASES] == [[3], [9], [9, 9], [8] * 9]
        for c in UPCONV_CASES:
            assert P.detail_seams(*c, up) == set(), (c, up)


@pytest.mark.parametrize('case', RS.UPCONV, ids=RS.UPCONV_IDS)
def test_upconv_inputs_exercise_both_sides_of_the_activation(case):
    for up in (True, False):
        ref = RS.upconv_reference(case, up)
        assert 0.2 < float((ref < 0).double().mean()) < 0.8


# ---------------------------------------------------------------------------------------------------------------- FLAMETex
def test_flametex_lists_sit_on_the_seams():
    t = _source('texture.hip')
    assert 'constexpr int kRB = 8, kAhead = 8;' in t and 'kMaxTex = 200' in t
    assert 'if (rows <= kRB)' in t and 'else if (rows <= 2 * kRB)' in t
    inst = {r: RS.flametex_instance(r) for r in RS.FLAMETEX_ROWS}
    assert inst == {8: (1, 1), 9: (2, 1), 16: (2, 1), 17: (4, 1), 32: (4, 1), 33: (4, 2), 41: (4, 2)}
    # 17: wave 2 of the four-wave instance holds one row; 41: the second group's wave 0 is full, its wave 1 holds one row
    assert 17 - 16 == 1 and 41 - 32 - 8 == 1
    assert set(RS.FLAMETEX_COMPONENTS) >= {7, 8, 9, 16, 17, 1, 200}
    src, uv, n_tex = RS.FLAMETEX_BASE
    assert RS.flametex_path(3 * uv * uv) == (4, 1, 27) and n_tex == 9
    got = {u: RS.flametex_path(3 * u * u) for _, u in RS.FLAMETEX_PATHS}
    assert got == {5: (1, 2, 11), 10: (4, 2, 11), 11: (1, 6, 43), 12: (4, 2, 44)}


@pytest.mark.parametrize('source,uv', [RS.FLAMETEX_BASE[:2]] + list(RS.FLAMETEX_PATHS))
def test_flametex_nearest_index_is_not_the_identity(source, uv):
    from stylegan_directions_face_reenactment_amd.texture import nearest_index
    idx = nearest_index(source, uv)
    assert np.array_equal(idx, RT.interpolate_index(source, uv).numpy())
    assert not np.array_equal(idx, np.arange(uv)) and len(set(idx.tolist())) == uv


@pytest.mark.parametrize('n_tex', sorted(set(RS.FLAMETEX_COMPONENTS)))
def test_flametex_code_rows_are_distinct_and_the_rows_differ(n_tex):
    code = RS.flametex_code(n_tex)
    assert tuple(code.shape) == (41, n_tex) and len({tuple(r.tolist()) for r in code}) == 41
    source, uv, _ = RS.FLAMETEX_BASE
    mean, basis = RT.synthetic_space(S, SEED, source, n_tex)
    ref = RT.flametex(mean, basis, code, source, uv)
    gap = (ref[:, None] - ref[None]).abs().flatten(2).max(2).values + 1e9 * torch.eye(41)
    stock = RT.flametex(mean, basis, code, source, uv, dtype=torch.float32).double()
    dev = float((stock - ref).abs().max())
    bar = max(8 * dev, 1e-6 * float(ref.abs().max()))
    print('n_tex=%d: closest two rows differ by %.3e, the bar is %.3e' % (n_tex, float(gap.min()), bar))
    assert float(gap.min()) > 10 * bar                                      # a row taken for another is well beyond the bar


# ---------------------------------------------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize('H,W', RS.SAMPLER_IMAGES)
def test_sampler_points_mean_what_their_tags_say(H, W):
    r = RS.sampler_reference(H, W)
    pts, tags, img = r['pts'], r['tags'], r['image']
    n = pts.shape[0]
    assert n == len(tags) and n == len(RS.axis_coordinates(W)) * len(RS.axis_coordinates(H)) + RS.SAMPLER_GENERAL
    # where nothing is sampled: F.grid_sample itself says 0, on the points it can be handed (finite, within +-3)
    near = r['zero'] & (pts.abs() <= 3).all(1)
    assert int(near.sum()) > 20
    z = F.grid_sample(img.double(), pts[near].double().view(1, 1, -1, 2), mode='bilinear', padding_mode='zeros', align_corners=False)
    assert int(torch.count_nonzero(z)) == 0
    assert sum(t in (('nonfinite', 'centre'), ('centre', 'nonfinite'), ('far', 'edge'), ('outside', 'partial')) for t in tags) >= 8
    # an exact centre: the texel itself (in float64 to the rounding of the coordinate; bit for bit where the side is a power of two)
    ty, tx = r['texel']
    ex = r['exact']
    assert float((r['ref'][:, ex] - img[0].double()[:, ty[ex], tx[ex]]).abs().max()) <= 1e-6
    assert torch.equal(r['r32'][:, ex], img[0].double()[:, ty[ex], tx[ex]])   # the float32 restatement: the texel's bits
    want = sum(1 for j in range(W) if RS._dyadic(W) or 2 * j + 1 == W) * sum(1 for i in range(H) if RS._dyadic(H) or 2 * i + 1 == H)
    assert int(ex.sum()) >= want and want >= 1
    if RS._dyadic(H) and RS._dyadic(W):
        assert int(ex.sum()) == H * W
    # the rest carry a value: edges and partial neighbours are not 0, and the restatement in float64 is F.grid_sample
    live = ~r['zero']
    assert bool((r['ref'][:, live].abs() > 1e-3).all())
    again = RD.grid_sample(img.double(), torch.where(live[:, None], pts, torch.zeros(())).double().view(1, 1, -1, 2))[0, :, 0]
    assert float((again - r['ref'])[:, live].abs().max()) <= 1e-14
    d32 = float((r['r32'] - r['ref']).abs().max())
    print('sampler %d x %d: %d points, %d exactly 0, %d exact centres, %d seam points; d32 %.3e' % (H, W, n, int(r['zero'].sum()), int(ex.sum()),
                                                                                                int(r['seam'].sum()), d32))
    assert int(r['seam'].sum()) >= 20 and int(r['general'].sum()) == RS.SAMPLER_GENERAL


def test_sampler_table_hands_vertex_t_to_texel_t():
    pts, _ = RS.sampler_points(4, 4)
    for zero_vertex in (False, True):
        Su, V, faces, pix, bary = RS.sampler_table(pts.shape[0], zero_vertex)
        assert Su * Su >= pts.shape[0] > (Su - 1) ** 2 and V == Su * Su + int(zero_vertex)
        assert int(faces.min()) >= 0 and int(faces.max()) < V and int(pix.min()) >= 0 and int(pix.max()) < faces.shape[0]   # all in-table
        tv = RS.sampler_vertices(pts, Su, V)
        got = RD.world2uv(tv, faces.long(), pix.long(), bary, dtype=torch.float32)[0].reshape(3, -1)[:2, :pts.shape[0]].T
        fin = torch.isfinite(pts)
        assert torch.equal(got[fin], pts[fin])
        if zero_vertex:
            inf = torch.isinf(pts)
            assert torch.equal(got[inf], pts[inf]) and bool(torch.isnan(got[torch.isnan(pts)]).all())
        else:
            assert bool(torch.isnan(got[~fin]).all())                       # 0 * inf: the plain table hands NaN on for +-inf


# ---------------------------------------------------------------------------------------------------------------- the UV passes
@pytest.mark.parametrize('Su', RS.UV_SIZES)
def test_uv_sizes_keep_the_set_aside_share_under_the_cap(Su):
    i = RS.uv_inputs(Su)
    pix, bary, amb = TC.uv_table(i['uv'], i['uvfaces'], Su)
    args = (i['uv_z'], i['verts'], i['normals'], i['faces'], pix, bary, i['mask'], i['fixed'])
    n64, p64, raw = RD.displacement2normal(*args)
    n32, p32, _ = RD.displacement2normal(*args, dtype=torch.float32)
    aside, share = RS.uv_set_aside(raw, amb, Su)
    m = RS.meshed(Su)
    print('uv %d: covered %.3f, meshed %d texels, set aside %s' % (Su, float((pix >= 0).double().mean()), int(m.sum()), ['%.4f' % s for s in share.tolist()]))
    assert float(share.max()) <= TC.CAP                                     # per map: each row's own share
    keep = (~aside)[:, None].expand(-1, 3, -1, -1)
    assert 0 < float((n32.double() - n64)[keep].abs().max()) < 1e-4
    assert int(m.sum()) == (Su - 10) * (Su - 4) and int(m.sum()) >= 27
    assert int(torch.count_nonzero(n64.permute(0, 2, 3, 1)[:, ~m])) == 0
    assert float((n64.norm(dim=1)[m[None] & ~aside] - 1).abs().max()) < 1e-9
    # three cameras, three sheets: no two rows alike
    for a in range(RS.UV_ROWS):
        for b in range(a):
            assert float((n64[a] - n64[b]).abs().max()) > 1e-2 and float((i['tv'][a] - i['tv'][b]).abs().max()) > 1e-2
    # the texture pass on the same table: continuous in everything but the table
    r64 = RT.uv_textures(i['albedo'], n64.float(), i['light'], i['tv'], i['images'], i['faces'], pix, bary, i['mask'])
    r32 = RT.uv_textures(i['albedo'], n64.float(), i['light'], i['tv'], i['images'], i['faces'], pix, bary, i['mask'], dtype=torch.float32)
    for k in r64:
        assert float((r32[k].double() - r64[k]).abs().max()) <= 1e-5, k


@pytest.mark.parametrize('Su', RS.UV_SIZES)
def test_uv_named_texels(Su):
    """The last tile column and row of a size 16 k + 1 is one texel wide, and no dense face names a texel there (the meshed texels
    end at S - 3 and S - 6): such a tile stages its halo and writes zeros and its own dense vertices.  The halo that a normal does
    depend on is the one between two full tiles, first met at 33."""
    m = RS.meshed(Su)
    tiles = -(-Su // 16)
    if Su % 16 == 1:
        assert not bool(m[:, 16 * (tiles - 1):].any()) and not bool(m[16 * (tiles - 1):].any())
    i = RS.uv_inputs(Su)
    pix, _, amb = TC.uv_table(i['uv'], i['uvfaces'], Su)
    halo, last = RS.UV_HALO_TEXEL[Su], RS.UV_LAST_TILE_TEXEL[Su]
    crossing = [(y, x) for y in range(Su) for x in range(Su) if m[y, x] and (y // 16 != max(y - 1, 0) // 16 or y // 16 != (y + 1) // 16 or
                                                                             x // 16 != (x - 1) // 16 or x // 16 != (x + 1) // 16)]
    if halo is None:
        assert not crossing                                                 # every meshed texel and its neighbours lie in tile (0, 0)
    else:
        y, x = halo
        assert halo in crossing and bool(m[y, x]) and not bool(amb[y, x]) and int(pix[y, x]) >= 0
        assert y % 16 == 0 and x % 16 == 0 and bool(m[y - 1, x - 1])        # its upper and left neighbours come from three other tiles
    if last is None:
        assert tiles == 1
    else:
        y, x = last
        assert x == 16 * (tiles - 1) == Su - 1 and not bool(m[y, x]) and int(pix[y, x]) >= 0 and int(pix[x, y]) >= 0 and not bool(amb[y, x] | amb[x, y])


# ---------------------------------------------------------------------------------------------------------------- the lattice
def test_small_lattice_sizes_are_exact():
    from test_cpu_shape_render import check_small_pair
    pairs = C.small_pairs()
    assert len(pairs) == len(C.LATTICE) * len(C.SMALL_SIZES) - len(C.SMALL_DROPPED) and C.SMALL_SIZES == (1, 8, 17)
    assert not set(C.SMALL_SIZES) & set(C.SIZES)
    for name, size in pairs:
        check_small_pair(name, size)
    verts, faces = C.lattice_grid()
    for size in C.SMALL_SIZES:
        p64, p32 = (R.rasterize(verts[None], faces, size, d)[0][0] for d in (torch.float64, torch.float32))
        assert torch.equal(p64, p32)
    assert len(p64.unique()) > 100                                          # 17: the grid's faces are there

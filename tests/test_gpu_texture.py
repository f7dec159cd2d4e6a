"""GPU: DECA's texture side on the HIP kernels (texture.py on csrc/texture.hip, the texture and attribute instances of
csrc/shaperender.hip, flame.visofp) against the reference's own FLAMETex results (kat23) and the float64 restatements of
tests/texture_restatement.py, on the inputs tests/test_cpu_texture.py has proven usable.

Bars (none taken from the code under test).
  FlameTex: kat23 within 8 x the reference's own fp32-vs-fp64 deviation (the kat12 / kat22 convention); the small sizes within 8 x the
    deviation of the reference expression in float32 from the same in float64, floor 1e-6 max|y|.
  Everything behind the rasteriser and the UV pass: within 4 x d32 of the float64 restatement, d32 being the restatement's own deviation
    in float32.  Set aside, each share printed and capped at 2 % of its map: pixels that are ambiguous by the rasteriser's existing
    definition (TOL) and, for the two thresholded outputs only, those whose float64 decision value lies within TOL of -0.05 (pos_mask)
    or 0.1 (visofp).  The UV pass is given its table and sets nothing aside; neither does the lattice mesh stacked_quads, whose edges
    pass through pixel centres only where float32 is exact.
Each test prints its own figures.
"""
import pytest
import torch

from util import S, SEED, golden
import detail_restatement as RD
import shape_render_cases as C
import shape_render_restatement as R
import texture_cases as TC
import texture_restatement as RT

pytestmark = pytest.mark.gpu

KAT = 'kat23_deca_texture.npz'
_CACHE = {}


def _tx():
    from stylegan_directions_face_reenactment_amd import texture
    return texture


def _sr():
    from stylegan_directions_face_reenactment_amd import shape_render
    return shape_render


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _flametex(seed, n_tex, source, uv):
    key = ('T', seed, n_tex, source, uv)
    if key not in _CACHE:
        mean, basis = RT.synthetic_space(S, seed, source, n_tex)
        T = _tx().FlameTex(n_tex, source, uv)
        T.load_state_dict({'texture_mean': mean, 'texture_basis': basis})
        _CACHE[key] = (T.cuda(), mean, basis)
    return _CACHE[key]


def _layout(faces, uv, uvfaces, Su, mask=None, n_vertices=None):
    from stylegan_directions_face_reenactment_amd import detail
    mask = torch.ones(Su, Su) if mask is None else mask
    return detail.UvLayout(faces, uv, uvfaces, Su, mask, torch.zeros(Su, Su), n_vertices=n_vertices)


def _replays(fn):
    """Two eager calls and one graph replay give the same bits; returns the eager result (a dict or a tensor)."""
    flat = lambda r: list(r.values()) if isinstance(r, dict) else [r]
    eager, again = fn(), fn()
    for a, b in zip(flat(eager), flat(again)):
        assert _same(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = fn()
    for t in flat(held):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(flat(eager), flat(held)):
        assert _same(a, b)
    return eager


# ------------------------------------------------------------------------------------------------------------------ FlameTex
def test_flametex_matches_kat23():
    g = golden(KAT)
    seed, source, uv, n_tex = int(g['seed']), int(g['source']), int(g['uv']), int(g['n_tex'])
    T, _, _ = _flametex(seed, n_tex, source, uv)
    assert _same(T.packed(), T.host_pack())                                      # the prepack launch writes the documented layout
    for tag, rows in RT.KAT_BATCHES:
        code = S.counter_tensor(seed, 'kat23.tex.' + tag, (rows, n_tex), 0.0, 1.0).cuda()
        albedo = T(code)
        assert tuple(albedo.shape) == (rows, 3, uv, uv) and albedo.dtype == torch.float32
        sub, brd, sums = RT.digest(albedo.cpu())
        dev = float(g['dev_' + tag])
        e_sub = float((sub - torch.from_numpy(g['sub_' + tag]).double()).abs().max())
        e_brd = float((brd - torch.from_numpy(g['border_' + tag]).double()).abs().max())
        e_sum = float((sums - torch.from_numpy(g['sums_' + tag])).abs().max())
        print('kat23 %s: hip sample %.3e border %.3e = %.2f, %.2f x the reference fp32 deviation %.3e (bar 8 x); plane sums %.3e'
              % (tag, e_sub, e_brd, e_sub / dev, e_brd / dev, dev, e_sum))
        assert e_sub <= 8 * dev and e_brd <= 8 * dev and e_sum <= 8 * dev * uv * uv


@pytest.mark.parametrize('n_tex', [1, 3, 50])
@pytest.mark.parametrize('source,uv', RT.SMALL, ids=['%dto%d' % c for c in RT.SMALL])
def test_flametex_small_sizes_and_batch_independence(source, uv, n_tex):
    T, mean, basis = _flametex(SEED, n_tex, source, uv)
    assert _same(T.packed(), T.host_pack())
    code = S.counter_tensor(SEED, 'flametex.code.%d' % n_tex, (5, n_tex))
    got5 = T(code.cuda())
    got1 = T(code[:1].cuda())
    assert _same(got5[:1], got1)                                                 # B = 1 and B = 5: the same row, bit for bit
    many = T(code.repeat(8, 1).cuda())                                           # 40 rows: the 32-row instance, two passes
    assert _same(many[:5], got5) and _same(many[35:], got5)
    mid = T(code.repeat(3, 1)[:12].cuda())                                       # 12 rows: the two-wave instance
    assert _same(mid[:5], got5) and _same(mid[10:], got5[:2])
    ref, stock = RT.flametex(mean, basis, code, source, uv), RT.flametex(mean, basis, code, source, uv, dtype=torch.float32).double()
    dev, err, scale = float((stock - ref).abs().max()), float((got5.cpu().double() - ref).abs().max()), float(ref.abs().max())
    bar = max(8 * dev, 1e-6 * scale)
    print('flametex %d -> %d n_tex=%d: hip %.3e, stock fp32 %.3e, bar %.3e, max|y| %.3e' % (source, uv, n_tex, err, dev, bar, scale))
    assert err <= bar


# ------------------------------------------------------------------------------------------------------------------ the textured render
ALL = ('images', 'albedo_images', 'alpha_images', 'pos_mask', 'shading_images', 'grid', 'normal_images', 'normals', 'transformed_normals',
       'pix_to_face', 'zbuf', 'bary')
_PIXEL = {'images': 3, 'albedo_images': 3, 'alpha_images': 1, 'pos_mask': 1, 'shading_images': 3, 'normal_images': 3}


def _uncovered_shading(light):
    """c0 L0 - c8 L8 in float32, as the kernel's ascending sum leaves it at the zero normal."""
    c = RT.sh_constants(torch.float32)
    return (light[:, 0] * (1.0 * c[0])) + (light[:, 8] * (-1.0 * c[8]))


@pytest.mark.parametrize('size,Su,rows,to_border', TC.RENDER, ids=TC.RENDER_IDS)
def test_render_texture_matches_the_restatement(size, Su, rows, to_border):
    SR = _sr()
    verts, faces, cam, uv, uvfaces = TC.sheet(rows, to_border)
    albedo, light, uvn, _ = TC.maps(rows, Su)
    L = _layout(faces, uv, uvfaces, Su, n_vertices=verts.shape[1])
    topo = SR.MeshTopology(faces, verts.shape[1])
    v, c, a, l = verts.cuda(), cam.cuda(), albedo.cuda(), light.cuda()
    got = SR.render_texture(v, topo, L, a, lights=l, cam=c, size=size, want=ALL)
    assert list(got) == list(ALL)
    old = SR.render_shape(v, topo, cam=c, size=size, layout=L, detail_normals=uvn.cuda(), want=('shape', 'grid', 'alpha', 'pix_to_face', 'zbuf', 'bary'))
    for k in ('grid', 'pix_to_face', 'zbuf', 'bary'):                            # one rasteriser: the detail instance's bits
        assert _same(old[k], got[k]), k
    assert _same(got['alpha_images'], (old['pix_to_face'] >= 0).float()[:, None])
    assert bool((old['alpha'] <= got['alpha_images']).all()) and float((got['alpha_images'] - old['alpha']).sum()) > 0     # no front-facing mask
    for sub in (('images',), ('shading_images', 'pos_mask'), ('normals', 'transformed_normals'), ('albedo_images', 'grid', 'bary')):
        part = SR.render_texture(v, topo, L, a, lights=l, cam=c, size=size, want=sub)
        assert list(part) == [k for k in ALL if k in sub]
        for k in sub:
            assert _same(part[k], got[k]), k
    r64 = RT.texture_render(verts, faces, size, L.face_uv, albedo, light, cam=cam)
    r32 = RT.texture_render(verts, faces, size, L.face_uv, albedo, light, cam=cam, dtype=torch.float32)
    amb, pamb = r64['ambiguous'], r64['pos_ambiguous']
    share, pshare = amb.reshape(rows, -1).double().mean(1), (amb | pamb).reshape(rows, -1).double().mean(1)
    print('render S=%d Su=%d rows=%d: set aside %s; with the -0.05 rule %s' % (size, Su, rows, ['%.4f' % s for s in share.tolist()],
                                                                            ['%.4f' % s for s in pshare.tolist()]))
    assert float(pshare.max()) <= TC.CAP
    clear = ~amb
    assert torch.equal(got['pix_to_face'].cpu().long()[clear], r64['pix_to_face'][clear])
    fair = clear & (r32['pix_to_face'] == r64['pix_to_face'])
    for k in ('images', 'albedo_images', 'alpha_images', 'pos_mask', 'shading_images', 'normal_images', 'grid', 'normals', 'transformed_normals'):
        keep, keep32 = clear, fair
        if k == 'pos_mask':
            keep, keep32 = clear & ~pamb, fair & ~pamb
        g, a64, a32 = got[k].cpu().double(), r64[k], r32[k].double()
        if k in _PIXEL:
            g, a64, a32 = (t.permute(0, 2, 3, 1) for t in (g, a64, a32))
        if k in ('normals', 'transformed_normals'):
            d32, dev = float((a32 - a64).abs().max()), float((g - a64).abs().max())
        else:
            d32, dev = float((a32 - a64)[keep32].abs().max()), float((g - a64)[keep].abs().max())
        print('render S=%d Su=%d rows=%d: %-20s hip deviation %.3e   d32 %.3e   bar %.3e' % (size, Su, rows, k, dev, d32, 4 * d32))
        assert dev <= 4 * d32, (k, dev, d32)
    # the quirk that is kept: shading_images is not masked -- an uncovered pixel holds add_SHlight(0) = c0 L0 - c8 L8
    covered = r64['pix_to_face'] >= 0
    assert not bool(covered[:, 0, 0].any())
    const = _uncovered_shading(light)
    shading = got['shading_images'].cpu().permute(0, 2, 3, 1)
    assert torch.equal(shading[:, 0, 0], const)                                  # the corner pixel
    for b in range(rows):
        m = ~covered[b] & clear[b]
        assert torch.equal(shading[b][m], const[b].expand(int(m.sum()), 3))
    for k in ('images', 'albedo_images', 'normal_images', 'alpha_images', 'pos_mask', 'grid'):
        t = got[k].cpu()
        t = t.permute(0, 2, 3, 1) if k in _PIXEL else t
        assert int(torch.count_nonzero(t[~covered & clear])) == 0, k
    if to_border:
        near = covered & (r64['grid'][..., 0] > 1 - 1.0 / Su)
        print('render S=%d Su=%d: %d pixels sample the albedo across its border' % (size, Su, int(near.sum())))
        assert int(near.sum()) > 0


def test_render_texture_without_lights_and_wholly_outside():
    SR = _sr()
    verts, faces, cam, uv, uvfaces = TC.sheet(1)
    albedo, light, _, _ = TC.maps(1, 16)
    L = _layout(faces, uv, uvfaces, 16, n_vertices=verts.shape[1])
    topo = SR.MeshTopology(faces, verts.shape[1])
    lit = SR.render_texture(verts.cuda(), topo, L, albedo.cuda(), lights=light.cuda(), cam=cam.cuda(), size=24, want=ALL)
    dark = SR.render_texture(verts.cuda(), topo, L, albedo.cuda(), lights=None, cam=cam.cuda(), size=24, want=ALL)
    assert _same(dark['images'], dark['albedo_images']) and int(torch.count_nonzero(dark['shading_images'])) == 0    # renderer.py:175-177
    for k in ALL:
        if k not in ('images', 'shading_images'):
            assert _same(dark[k], lit[k]), k
    # projected= gives what cam= gives when handed the same projection
    proj = R.project(verts, cam, 0.0, torch.float32)
    by_proj = SR.render_texture(verts.cuda(), topo, L, albedo.cuda(), lights=light.cuda(), projected=proj.cuda(), size=24, want=ALL)
    for k in ALL:
        assert _same(by_proj[k], lit[k]), k
    # a mesh wholly outside the image: nothing but the unmasked shading constant
    pv, pf = C.LATTICE['wholly_outside']
    pv = pv.float()[None]
    Lo = _layout(pf, torch.tensor([[0.1, 0.1], [0.9, 0.1], [0.5, 0.9], [0.2, 0.3], [0.8, 0.3], [0.5, 0.7]], dtype=torch.float64), pf, 16, n_vertices=6)
    out = SR.render_texture(pv.cuda(), SR.MeshTopology(pf, 6), Lo, albedo.cuda(), lights=light.cuda(), projected=pv.cuda(), size=24, want=ALL)
    for k in ('images', 'albedo_images', 'alpha_images', 'pos_mask', 'grid', 'normal_images'):
        assert int(torch.count_nonzero(out[k])) == 0, k
    assert int((out['pix_to_face'] != -1).sum()) == 0
    assert torch.equal(out['shading_images'].cpu(), _uncovered_shading(light)[:, :, None, None].expand(-1, -1, 24, 24))


# ------------------------------------------------------------------------------------------------------------------ the UV pass
@pytest.mark.parametrize('Su,H,with_albedo,kind', TC.UV, ids=TC.UV_IDS)
def test_uv_textures_match_the_restatement(Su, H, with_albedo, kind):
    tx = _tx()
    rows = 2
    verts, faces, cam, uv, uvfaces = TC.sheet(rows)
    albedo, light, uvn, images = TC.maps(rows, Su, H)
    albedo = albedo if with_albedo else None
    mask = TC.mask_of(kind, Su)
    L = _layout(faces, uv, uvfaces, Su, mask=mask, n_vertices=verts.shape[1])
    tv = R.project(verts, cam, 0.0, torch.float32)
    want = ('uv_shading', 'uv_texture', 'uv_texture_gt', 'uv_pverts', 'uv_gt')
    cu = lambda t: None if t is None else t.cuda()
    got = tx.uv_textures(L, cu(albedo), uvn.cuda(), light.cuda(), tv.cuda(), images.cuda(), want=want)
    assert list(got) == [k for k in want if with_albedo or k != 'uv_texture']
    default = tx.uv_textures(L, cu(albedo), uvn.cuda(), light.cuda(), tv.cuda(), images.cuda())
    assert list(default) == [k for k in want[:3] if with_albedo or k != 'uv_texture']
    for k in default:
        assert _same(default[k], got[k]), k
    _, pix, bary, _, _, _ = L.tables('cuda')
    pix, bary = pix.cpu().long(), bary.cpu()
    r64 = RT.uv_textures(albedo, uvn, light, tv, images, faces, pix, bary, mask)
    r32 = RT.uv_textures(albedo, uvn, light, tv, images, faces, pix, bary, mask, dtype=torch.float32)
    for k in got:
        d32, dev = float((r32[k].double() - r64[k]).abs().max()), float((got[k].cpu().double() - r64[k]).abs().max())
        print('uv Su=%d H=%d %s %s: %-14s hip deviation %.3e   d32 %.3e   bar %.3e' % (Su, H, 'albedo' if with_albedo else 'plain', kind, k, dev, d32, 4 * d32))
        assert dev <= 4 * d32, (k, dev, d32)
    none = pix < 0
    assert Su == 16 or int(none.sum()) > 0
    if int(none.sum()):                                                          # the quirk that is kept: the image centre
        c = H // 2
        centre = images[:, :, c - 1:c + 1, c - 1:c + 1].mean((2, 3))
        assert int(torch.count_nonzero(got['uv_pverts'].cpu()[..., none])) == 0
        assert float((got['uv_gt'].cpu()[..., none] - centre[..., None]).abs().max()) <= 1e-6
    if kind == 'one':
        assert _same(got['uv_texture_gt'], got['uv_gt'])
    if kind == 'zero' and not with_albedo:
        assert float((got['uv_texture_gt'] - 0.7).abs().max()) <= 1e-7


def test_uv_shading_on_the_output_of_detail_normals():
    from stylegan_directions_face_reenactment_amd import detail
    tx, Su, rows = _tx(), 40, 2
    verts, faces, cam, uv, uvfaces = TC.sheet(rows)
    _, light, _, images = TC.maps(rows, Su, 8)
    L = detail.UvLayout(faces, uv, uvfaces, Su, TC.mask_of('mixed', Su), S.counter_tensor(SEED, 'texture.fixed', (Su, Su), 0.0, 0.003),
                        n_vertices=verts.shape[1])
    uv_z = S.counter_tensor(SEED, 'texture.uvz', (rows, 1, Su, Su), 0.0, 0.01)
    normals = R.vertex_normals(verts, faces).float()
    uvn = detail.detail_normals(L, uv_z.cuda(), verts.cuda(), normals.cuda())
    got = tx.uv_textures(L, None, uvn, light.cuda(), verts.cuda(), images.cuda(), want='uv_shading')['uv_shading']
    r64, r32 = RT.add_shlight(uvn.cpu(), light), RT.add_shlight(uvn.cpu(), light, dtype=torch.float32)
    d32, dev = float((r32.double() - r64).abs().max()), float((got.cpu().double() - r64).abs().max())
    print('uv_shading on detail_normals: hip deviation %.3e   d32 %.3e   bar %.3e' % (dev, d32, 4 * d32))
    assert dev <= 4 * d32 and float(uvn.abs().max()) > 0.5


# ------------------------------------------------------------------------------------------------------------------ visofp, normal, depth
@pytest.mark.parametrize('rows', [1, 2])
def test_visofp_render_normal_and_render_depth(rows):
    SR = _sr()
    from stylegan_directions_face_reenactment_amd import flame as FL
    p, faces, tn = TC.sheet_projected(rows)
    sp, sfaces, svalues = TC.stacked(rows)
    for name, proj, f, values, zoff in (('sheet', p, faces, tn, R.Z_OFFSET), ('stacked', sp, sfaces, svalues, 0.0)):
        V = proj.shape[1]
        topo = SR.MeshTopology(f, V)
        idx, w = TC.landmarks(len(f))
        vis = FL.visofp(FL.LandmarkTable(f, idx, w, V), values.cuda())
        v64, z64 = RT.visofp(values, f, idx, w)
        near = (z64 - RT.VIS_Z).abs() < R.TOL
        assert tuple(vis.shape) == (rows, TC.N_LMK, 1) and float(near.double().mean(1).max()) <= TC.CAP
        assert torch.equal(vis.cpu()[:, :, 0][~near].double(), v64[:, :, 0][~near])
        print('%s rows=%d visofp: %d landmarks set aside, visible share %.2f' % (name, rows, int(near.sum()), float(vis.mean())))
        for size in TC.ATTR_SIZES:
            got = SR.render_normal(proj.cuda(), values.cuda(), topo, size, z_offset=zoff)
            dgot = SR.render_depth(proj.cuda(), topo, size)
            assert tuple(got.shape) == (rows, 3, size, size) and tuple(dgot.shape) == (rows, 1, size, size)
            for what, g, (a64, amb, pix), (a32, _, pix32) in (
                    ('render_normal', got, RT.render_attr(proj, values, f, size, zoff), RT.render_attr(proj, values, f, size, zoff, dtype=torch.float32)),
                    ('render_depth', dgot, RT.render_depth(proj, f, size), RT.render_depth(proj, f, size, dtype=torch.float32))):
                if name == 'stacked':
                    amb = torch.zeros_like(amb)                                   # a lattice mesh: nothing is set aside
                share = amb.reshape(rows, -1).double().mean(1)
                assert float(share.max()) <= TC.CAP
                clear, fair = ~amb, ~amb & (pix32 == pix)
                g, a64, a32 = (t.permute(0, 2, 3, 1) for t in (g.cpu().double(), a64, a32.double()))
                d32, dev = float((a32 - a64)[fair].abs().max()), float((g - a64)[clear].abs().max())
                print('%s rows=%d S=%d %-13s hip deviation %.3e   d32 %.3e   bar %.3e; set aside %s'
                      % (name, rows, size, what, dev, d32, 4 * d32, ['%.4f' % s for s in share.tolist()]))
                assert dev <= 4 * d32, (what, dev, d32)
                assert int(torch.count_nonzero(g[(pix < 0) & clear])) == 0
            if rows > 1:                                                         # the minimum and maximum are the batch's, not a row's
                alone = SR.render_depth(proj[:1].cuda(), topo, size)
                assert float((alone - dgot[:1]).abs().max()) > 1e-3
            assert 0.0 <= float(dgot.min()) and float(dgot.max()) <= 1.0 + 1e-6


# ------------------------------------------------------------------------------------------------------------------ composition
def _deca_case():
    from test_gpu_detail import _decoder, _flame_case
    if 'deca' not in _CACHE:
        m, L, code, _, _ = _flame_case()
        D = _decoder(int(golden('kat22_deca_detail.npz')['seed']))
        T, _, _ = _flametex(SEED, 50, 256, 256)
        rows = code['pose'].shape[0]
        code = dict(code)
        code['tex'] = S.counter_tensor(SEED, 'texture.deca.tex', (rows, 50)).cuda()
        light = S.counter_tensor(SEED, 'texture.deca.light', (rows, 9, 3), 0.0, 0.3)
        light[:, 0] += 2.5
        code['light'] = light.cuda()
        code['images'] = S.counter_tensor(SEED, 'texture.deca.images', (rows, 3, 224, 224), 0.5, 0.2).cuda()
        _CACHE['deca'] = (m, D, L, T, code)
    return _CACHE['deca']


OPDICT = ['vertices', 'normals', 'transformed_vertices', 'landmarks2d', 'landmarks3d', 'uv_detail_normals', 'uv_texture_gt', 'displacement_map']
VISDICT = ['inputs', 'landmarks2d', 'landmarks3d', 'shape_images', 'shape_detail_images']


def test_decode_deca_keys_and_wiring():
    """deca.py:202-225: the key lists for both values of use_tex, the detail half's bits, and every other entry against the public
    function that makes it, fed what the composition feeds it."""
    tx, SR = _tx(), _sr()
    from stylegan_directions_face_reenactment_amd import detail, flame as FL
    m, D, L, T, code = _deca_case()
    before = {k: v.clone() for k, v in code.items()}
    op, vis = tx.decode_deca(m, D, L, code, flametex=T)
    op0, vis0 = tx.decode_deca(m, D, L, code)
    assert list(op) == OPDICT + ['albedo', 'uv_texture'] and list(vis) == VISDICT + ['rendered_images']
    assert list(op0) == OPDICT and list(vis0) == VISDICT
    for k, v in before.items():                                                  # nothing the caller passes is modified
        assert _same(code[k], v), k
    det = detail.decode_detail(m, D, L, code)
    for d in (vis, vis0):
        assert _same(d['shape_images'], det['shape_images']) and _same(d['shape_detail_images'], det['shape_detail_images'])
    assert _same(op['uv_detail_normals'], det['uv_detail_normals']) and _same(op['displacement_map'], det['displacement_map'])
    assert vis['inputs'] is code['images'] and vis['landmarks2d'] is op['landmarks2d'] and vis['landmarks3d'] is op['landmarks3d']
    rows = code['pose'].shape[0]
    assert tuple(op['landmarks2d'].shape) == (rows, 68, 2) and tuple(op['landmarks3d'].shape) == (rows, 68, 4)
    with torch.no_grad():
        verts, lm2d, lm3d = m(code['alpha_shp'], code['alpha_exp'], code['pose'])
        px2d, px3d, _ = FL.decode(m, {'shape': code['alpha_shp'], 'exp': code['alpha_exp'], 'pose': code['pose'], 'cam': code['cam']})
    assert _same(op['vertices'], verts)
    assert float((op['landmarks2d'] - px2d).abs().max()) <= 1e-3 and float((op['landmarks3d'][:, :, :3] - px3d).abs().max()) <= 1e-3    # pixels
    tv = R.project(verts.cpu(), code['cam'].cpu(), 0.0, torch.float32)
    assert float((op['transformed_vertices'].cpu() - tv).abs().max()) <= 1e-6   # the projected vertices, not the reference's z + 30
    topo = FL.topology(m)
    assert _same(op['albedo'], T(code['tex']))
    ops = SR.render_texture(verts, topo, L, op['albedo'], lights=code['light'], cam=code['cam'], want=('images', 'normals', 'transformed_normals'))
    assert _same(vis['rendered_images'], ops['images']) and _same(op['normals'], ops['normals']) and _same(op0['normals'], ops['normals'])
    assert _same(op['landmarks3d'][:, :, 3:], FL.visofp(m, ops['transformed_normals']))
    assert 0 < float(op['landmarks3d'][:, :, 3].mean()) <= 1
    maps = tx.uv_textures(L, op['albedo'], op['uv_detail_normals'], code['light'], op['transformed_vertices'], code['images'])
    assert _same(op['uv_texture'], maps['uv_texture']) and _same(op['uv_texture_gt'], maps['uv_texture_gt'])
    plain = tx.uv_textures(L, None, op['uv_detail_normals'], code['light'], op['transformed_vertices'], code['images'])
    assert _same(op0['uv_texture_gt'], plain['uv_texture_gt'])
    assert float(vis['rendered_images'].abs().max()) > 0.1


def test_replays_equal_the_eager_calls():
    tx, SR = _tx(), _sr()
    from stylegan_directions_face_reenactment_amd import flame as FL
    m, D, L, T, code = _deca_case()
    verts, faces, cam, uv, uvfaces = TC.sheet(2)
    albedo, light, uvn, images = TC.maps(2, 16, 8)
    Ls = _layout(faces, uv, uvfaces, 16, n_vertices=verts.shape[1])
    topo = SR.MeshTopology(faces, verts.shape[1])
    table = FL.LandmarkTable(faces, *TC.landmarks(len(faces)), verts.shape[1])
    v, c, a, l, n, im = (t.cuda() for t in (verts, cam, albedo, light, uvn, images))
    Ts, _, _ = _flametex(SEED, 3, 12, 6)
    code3 = S.counter_tensor(SEED, 'flametex.code.3', (5, 3)).cuda()
    _replays(lambda: Ts(code3))
    _replays(lambda: SR.render_texture(v, topo, Ls, a, lights=l, cam=c, size=24, want=ALL))
    _replays(lambda: tx.uv_textures(Ls, a, n, l, v, im))
    _replays(lambda: FL.visofp(table, v))
    _replays(lambda: SR.render_normal(v, v, topo, 24, z_offset=10.0))
    _replays(lambda: SR.render_depth(v, topo, 24))
    # visdict['inputs'] is the caller's own tensor: it is no output, and the replay must find it as it was
    merge = lambda pair: {('%d.' % i) + k: t for i, d in enumerate(pair) for k, t in d.items() if k != 'inputs'}
    eager = merge(tx.decode_deca(m, D, L, code, flametex=T))
    merged = _replays(lambda: merge(tx.decode_deca(m, D, L, code, flametex=T)))
    assert len(merged) == 15
    for k, t in eager.items():
        assert _same(merged[k], t), k


def test_refused_arguments():
    """Every refusal comes before the first launch."""
    tx, SR = _tx(), _sr()
    from stylegan_directions_face_reenactment_amd import flame as FL
    verts, faces, cam, uv, uvfaces = TC.sheet(1)
    albedo, light, uvn, images = TC.maps(1, 16, 8)
    L = _layout(faces, uv, uvfaces, 16, n_vertices=verts.shape[1])
    topo = SR.MeshTopology(faces, verts.shape[1])
    v, c, a, l, n, im = (t.cuda() for t in (verts, cam, albedo, light, uvn, images))
    with pytest.raises(RuntimeError, match='want must name'):
        SR.render_texture(v, topo, L, a, lights=l, cam=c, size=16, want=('images', 'shape'))
    with pytest.raises(RuntimeError, match='exactly one of cam and projected'):
        SR.render_texture(v, topo, L, a, lights=l, size=16)
    with pytest.raises(RuntimeError, match='UvLayout'):
        SR.render_texture(v, topo, None, a, lights=l, cam=c, size=16)
    with pytest.raises(RuntimeError, match='GPU'):
        SR.render_texture(v, topo, L, albedo, lights=l, cam=c, size=16)
    with pytest.raises(RuntimeError, match=r'albedo of shape \[1,3,16,16\]'):
        SR.render_texture(v, topo, L, a[:, :, :8], lights=l, cam=c, size=16)
    with pytest.raises(RuntimeError, match='point and directional lights'):
        SR.render_texture(v, topo, L, a, lights=torch.zeros(1, 5, 6, device='cuda'), cam=c, size=16)
    with pytest.raises(RuntimeError, match=r'lights of shape \[1,9,3\]'):
        SR.render_texture(v, topo, L, a, lights=l[:, :8], cam=c, size=16)
    with pytest.raises(RuntimeError, match='need an albedo'):
        SR.render_texture(v, topo, L, None, lights=l, cam=c, size=16, want=('images',))
    with pytest.raises(RuntimeError, match='forward only'):
        SR.render_texture(v.clone().requires_grad_(True), topo, L, a, lights=l, cam=c, size=16)
    with pytest.raises(RuntimeError, match='size must be'):
        SR.render_texture(v, topo, L, a, lights=l, cam=c, size=5000)
    other = SR.MeshTopology(faces[:100], verts.shape[1])
    with pytest.raises(RuntimeError, match='the layout is for a mesh'):
        SR.render_texture(v, other, L, a, lights=l, cam=c, size=16)
    with pytest.raises(RuntimeError, match=r'values of shape \[1,169,1..3\]'):
        SR.render_normal(v, torch.zeros(1, 169, 4, device='cuda'), topo, 16)
    with pytest.raises(RuntimeError, match='forward only'):
        SR.render_depth(v.clone().requires_grad_(True), topo, 16)
    with pytest.raises(RuntimeError, match='GPU'):
        SR.render_depth(verts, topo, 16)
    with pytest.raises(RuntimeError, match='want must name'):
        tx.uv_textures(L, a, n, l, v, im, want=('uv_normals',))
    with pytest.raises(RuntimeError, match=r'light of shape \[1,9,3\]'):
        tx.uv_textures(L, a, n, l[:, :, :2], v, im)
    with pytest.raises(RuntimeError, match=r'images of shape \[1,3,H,W\]'):
        tx.uv_textures(L, a, n, l, v, im[:, :2])
    with pytest.raises(RuntimeError, match=r'uv_detail_normals of shape \[1,3,16,16\]'):
        tx.uv_textures(L, a, n[:, :, :4], l, v, im)
    with pytest.raises(RuntimeError, match='forward only'):
        tx.uv_textures(L, a.clone().requires_grad_(True), n, l, v, im)
    with pytest.raises(RuntimeError, match='needs an albedo'):
        tx.uv_textures(L, None, n, l, v, im, want='uv_texture')
    T, _, _ = _flametex(SEED, 3, 12, 6)
    with pytest.raises(RuntimeError, match=r'texcode of shape \[B,3\]'):
        T(torch.zeros(2, 4, device='cuda'))
    with pytest.raises(RuntimeError, match='GPU'):
        T(torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match='forward only'):
        T(torch.zeros(2, 3, device='cuda', requires_grad=True))
    with pytest.raises(RuntimeError, match='FLAME module or a LandmarkTable'):
        FL.visofp(None, v)
    with pytest.raises(RuntimeError, match=r'\[B,169,3\]'):
        FL.visofp(FL.LandmarkTable(faces, *TC.landmarks(len(faces)), 169), v[:, :100])
    m, D, Lf, Tf, code = _deca_case()
    with pytest.raises(RuntimeError, match="codedict has no 'tex'"):
        tx.decode_deca(m, D, Lf, {k: t for k, t in code.items() if k != 'tex'}, flametex=Tf)
    with pytest.raises(RuntimeError, match=r'light of shape \[2,9,3\]'):
        tx.decode_deca(m, D, Lf, dict(code, light=code['light'].reshape(2, 27)), flametex=Tf)
    with pytest.raises(RuntimeError, match='FlameTex or None'):
        tx.decode_deca(m, D, Lf, code, flametex=D)
    with pytest.raises(RuntimeError, match='writes 6 x 6 maps'):
        tx.decode_deca(m, D, Lf, dict(code, tex=code['tex'][:, :3]), flametex=T)
    with pytest.raises(RuntimeError, match='forward only'):
        tx.decode_deca(m, D, Lf, dict(code, light=code['light'].clone().requires_grad_(True)), flametex=Tf)

"""GPU: DECA's detail path on the HIP kernels (detail.py on csrc/detail.hip, the detail entry of csrc/shaperender.hip, E_detail on
csrc/deca.hip) against the reference's own results (kat22), stock torch in fp64 and the restatements of tests/detail_restatement.py.

Bars (none taken from the code under test).
  Layer kernel: within 8 x the deviation of the stock fp32 chain (F.interpolate + F.conv2d on the CPU) from the same chain in fp64,
    floor 1e-6 max|y| -- the kat12 convention; the factor covers another summation order over K <= 1152.  Border rows and columns
    and the interior are compared and printed apart, so a clamp or padding slip is named.
  D_detail and E_detail: every stage and uv_z, and the 128 codes, within 8 x the reference's own fp32-vs-fp64 deviation (kat22 dev_*).
  UV pass and detail shade: within 4 x d32 of the float64 restatement on the same table, d32 being the restatement's own deviation in
    float32 (the bar of test_gpu_shape_render.py); set aside, under a cap of 2 % of the map: texels / pixels that are ambiguous by
    the rasteriser's existing definition and texels whose un-normalised normal is shorter in float64 than 1e-3 x the median over
    the meshed texels.  Uncovered texels are exactly 0.
Each test prints its own figures.
"""
import pytest
import torch

from util import S, SEED, golden
import deca_restatement as RE
import detail_restatement as RD
import shape_render_restatement as R
import shape_render_cases as C

pytestmark = pytest.mark.gpu

KAT = 'kat22_deca_detail.npz'
_CACHE = {}


def _dt():
    from stylegan_directions_face_reenactment_amd import detail
    return detail


def _decoder(seed):
    if ('D', seed) not in _CACHE:
        D = _dt().DetailDecoder()
        D.load_state_dict(S.synthetic_detail_decoder_state(seed), strict=True)
        _CACHE[('D', seed)] = D.cuda().eval()
    return _CACHE[('D', seed)]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ the layer kernel
UPCONV_CASES = [(1, 5, 3, 3, 5), (2, 16, 1, 8, 8), (1, 32, 16, 9, 7), (3, 128, 64, 8, 8)]


@pytest.mark.parametrize('up', [True, False], ids=['up', 'plain'])
@pytest.mark.parametrize('rows,cin,cout,h,w', UPCONV_CASES, ids=['%dx%d_%dto%d' % (c[3], c[4], c[1], c[2]) for c in UPCONV_CASES])
def test_upconv_matches_interpolate_and_conv2d(rows, cin, cout, h, w, up):
    key = 'detail.upconv.%d.%d.%d.%d' % (cin, cout, h, int(up))
    x = S.counter_tensor(SEED, key + '.x', (rows, cin, h, w))
    wt = S.counter_tensor(SEED, key + '.w', (cout, cin, 3, 3), 0.0, (2.0 / (9 * cin)) ** 0.5)
    b = S.counter_tensor(SEED, key + '.b', (cout,), 0.0, 0.1)
    slope = 1.0 if cout == 1 else 0.2                       # 1: no activation (the decoder's last conv)
    ref = RD.upconv(x, wt, b, slope, up)
    stock = RD.upconv(x, wt, b, slope, up, dtype=torch.float32).double()
    got = _dt().upconv(x.cuda(), wt.cuda(), b.cuda(), slope=slope, up=up)
    assert tuple(got.shape) == tuple(ref.shape)
    got = got.double().cpu()
    edge = torch.zeros(ref.shape[2:], dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    scale = float(ref.abs().max())
    for name, m in (('border', edge), ('interior', ~edge)):
        dev, err = float((stock - ref)[..., m].abs().max()), float((got - ref)[..., m].abs().max())
        bar = max(8 * dev, 1e-6 * scale)
        print('upconv %dx%d %d->%d up=%d %-8s hip %.3e, stock fp32 %.3e (ratio %.2f), bar %.3e, max|y| %.3e'
              % (h, w, cin, cout, up, name, err, dev, err / max(dev, 1e-30), bar, scale))
        assert err <= bar, (name, err, bar)
    assert float((ref < 0).double().mean()) > 0.2           # the activation's both sides are exercised


def test_upconv_refused_arguments():
    dt = _dt()
    x, w, b = torch.zeros(1, 4, 4, 4, device='cuda'), torch.zeros(2, 4, 3, 3, device='cuda'), torch.zeros(2, device='cuda')
    with pytest.raises(RuntimeError, match='GPU'):
        dt.upconv(x.cpu(), w, b)
    with pytest.raises(RuntimeError, match='expected x'):
        dt.upconv(x, w[:, :3], b)
    with pytest.raises(RuntimeError, match='sides 1..256'):
        dt.upconv(torch.zeros(1, 4, 257, 4, device='cuda'), w, b)
    with pytest.raises(ValueError, match='channel counts'):
        dt.upconv(torch.zeros(1, 1025, 2, 2, device='cuda'), torch.zeros(2, 1025, 3, 3, device='cuda'), b)


# ------------------------------------------------------------------------------------------------------------------ D_detail
@pytest.mark.parametrize('tag,rows', RD.BATCHES, ids=[b[0] for b in RD.BATCHES])
def test_decoder_stages_match_kat22(tag, rows):
    """Prints per stage the ratios (sample, border) / dev (bar 8)."""
    g = golden(KAT)
    D = _decoder(int(g['seed']))
    z = S.counter_tensor(int(g['seed']), 'kat22.latent.' + tag, (rows, 181), 0.0, 1.0).cuda()
    uv_z, taps = _dt().decode_uv(D, z, taps=True)
    assert tuple(uv_z.shape) == (rows, 1, 256, 256) and _same(D(z), uv_z)            # without taps: the two workspace buffers
    for s, (e_sub, e_brd, e_sum, dev, plane) in enumerate(RD.stage_errors(g, tag, taps + [uv_z])):
        print('kat22 %s stage %d: hip sample %.3e border %.3e = %.2f, %.2f x the reference fp32 deviation %.3e (bar 8 x); plane sums %.3e'
              % (tag, s, e_sub, e_brd, e_sub / dev, e_brd / dev, dev, e_sum))
        assert e_sub <= 8 * dev and e_brd <= 8 * dev and e_sum <= 8 * dev * plane
    assert 0.3 <= float(g['pre_tanh_std_' + tag]) <= 1.5


def test_decoder_refused_arguments():
    D = _decoder(int(golden(KAT)['seed']))
    with pytest.raises(RuntimeError, match=r'\[B,181\]'):
        D(torch.zeros(2, 180, device='cuda'))
    with pytest.raises(RuntimeError, match='GPU'):
        D(torch.zeros(2, 181))
    with pytest.raises(RuntimeError, match='forward only'):
        D(torch.zeros(2, 181, device='cuda', requires_grad=True))
    with pytest.raises(ValueError, match='batch'):
        D(torch.zeros(257, 181, device='cuda'))


# ------------------------------------------------------------------------------------------------------------------ E_detail
def test_detail_encoder_matches_kat22_and_leaves_encode_alone():
    from stylegan_directions_face_reenactment_amd import deca as D
    g = golden(KAT)
    Ed = D.ResnetEncoder(128)
    Ed.load_state_dict(S.synthetic_deca_detail_encoder_state(int(g['seed'])), strict=True)
    Ed = Ed.cuda().eval()
    E = D.ResnetEncoder()
    E.load_state_dict(S.synthetic_deca_encoder_state(int(g['kat12_seed'])), strict=True)
    E = E.cuda().eval()
    for name in RE.CASES:
        x, boxes, _ = RE.fixture_inputs(S, int(g['kat12_seed']), name)
        M = D.crop_matrix(boxes, x.shape[2:]).cuda()
        x = x.cuda()
        with torch.no_grad():
            alone = D.encode(E, x, M)
            both = D.encode(E, x, M, E_detail=Ed)
            params = D.run(E, x, M)[0]
        assert list(both) == list(alone)[:-1] + ['detail', 'images'] and 'detail' not in alone
        for k in alone:                                                              # bit for bit what E_flame alone gives
            assert _same(alone[k], both[k]), k
        assert _same(torch.cat([alone[k].flatten(1) for k in ('shape', 'tex', 'exp', 'pose', 'cam', 'light')], 1), params)
        codes = both['detail']
        assert tuple(codes.shape) == (x.shape[0], 128) and not codes.requires_grad and _same(Ed(x, M), codes)
        dev = float(g['dev_codes_' + name])
        err = float((codes.double().cpu() - torch.from_numpy(g['codes_' + name])).abs().max())
        print('kat22 %s detail codes: hip deviation %.3e = %.2f x the reference fp32 deviation %.3e (bar 8 x)' % (name, err, err / dev, dev))
        assert err <= 8 * dev
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match='no gradient'):
        D.run(Ed, xg, M)
    code = D.encode(E, xg, M, E_detail=Ed)                                          # E_flame's gradient stays; the detail code has none
    assert code['shape'].requires_grad and not code['detail'].requires_grad


# ------------------------------------------------------------------------------------------------------------------ UV space
def _sheet(S_, rows=2, to_border=False):
    """smooth_grid with the seam atlas as a UvLayout at uv_size S_, a seeded mask (about a quarter off), fixed_dis and uv_z."""
    verts, faces, cam = C.smooth_grid(5, rows=rows)
    uv, uvfaces = RD.seam_atlas(faces, to_border=to_border)
    mask = (S.counter_tensor(SEED, 'detail.mask.%d' % S_, (S_, S_)) > -0.7).float()
    fixed = S.counter_tensor(SEED, 'detail.fixed.%d' % S_, (S_, S_), 0.0, 0.003)
    uv_z = S.counter_tensor(SEED, 'detail.uvz.%d' % S_, (rows, 1, S_, S_), 0.0, 0.01)
    L = _dt().UvLayout(faces, uv, uvfaces, S_, mask, fixed, n_vertices=verts.shape[1])
    return verts, faces, cam, uv, uvfaces, mask, fixed, uv_z, L


def _meshed(S_):
    m = torch.zeros(S_, S_, dtype=torch.bool)
    m[5:S_ - 5, 2:S_ - 2] = True                            # the vertices util.generate_triangles(S, S) names
    return m


@pytest.mark.parametrize('S_', [16, 40, 256])
def test_uv_pass_matches_the_restatement(S_):
    dt = _dt()
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    verts, faces, _, uv, uvfaces, mask, fixed, uv_z, L = _sheet(S_)
    _, pix, bary, _, _, _ = L.tables('cuda')
    pix, bary = pix.cpu().long(), bary.cpu()
    # the table against the restatement's own rasterisation of the float32 UV vertices
    pr, _, _, amb = R.rasterize(L.uv_vertices.double()[None], uvfaces, S_)
    pr, amb = pr[0], amb[0]
    print('uv %d: covered %.3f, ambiguous %.4f, table differs on %d texels' % (S_, float((pix >= 0).double().mean()), float(amb.double().mean()),
                                                                             int((pix != pr).sum())))
    assert torch.equal(pix[~amb], pr[~amb])
    normals = R.vertex_normals(verts, faces).float()
    # world2uv
    got = dt.world2uv(L, verts.cuda()).cpu()
    w64, w32 = RD.world2uv(verts, faces, pix, bary), RD.world2uv(verts, faces, pix, bary, dtype=torch.float32)
    d32 = float((w32.double() - w64)[..., ~amb].abs().max())
    err = float((got.double() - w64)[..., ~amb].abs().max())
    print('uv %d world2uv: hip deviation %.3e   d32 %.3e   bar %.3e' % (S_, err, d32, 4 * d32))
    assert err <= 4 * d32
    assert int(torch.count_nonzero(got[..., pix < 0])) == 0 and (S_ == 16 or int((pix < 0).sum()) > 0)
    # displacement2normal
    uvn, dense = dt.detail_normals(L, uv_z.cuda(), verts.cuda(), normals.cuda(), dense_vertices=True)
    assert _same(dt.detail_normals(L, uv_z.cuda(), verts.cuda(), normals.cuda()), uvn)
    n64, p64, raw = RD.displacement2normal(uv_z, verts, normals, faces, pix, bary, mask, fixed)
    n32, p32, _ = RD.displacement2normal(uv_z, verts, normals, faces, pix, bary, mask, fixed, dtype=torch.float32)
    meshed = _meshed(S_)
    ill = meshed[None] & (raw < 1e-3 * raw[:, meshed].median())
    aside = amb[None] | ill
    share = aside.reshape(aside.shape[0], -1).double().mean(1)
    print('uv %d: set aside %s of the map (ill-conditioned %d texels)' % (S_, ['%.4f' % s for s in share.tolist()], int(ill.sum())))
    assert float(share.max()) <= 0.02
    keep = (~aside)[:, None].expand(-1, 3, -1, -1)
    d32 = float((n32.double() - n64)[keep].abs().max())
    err = float((uvn.cpu().double() - n64)[keep].abs().max())
    print('uv %d detail normals: hip deviation %.3e   d32 %.3e   bar %.3e' % (S_, err, d32, 4 * d32))
    assert err <= 4 * d32
    dp32 = float((p32.double() - p64).abs().max())
    perr = float((dense.cpu().double() - p64).abs().max())
    print('uv %d dense vertices: hip deviation %.3e   d32 %.3e   bar %.3e' % (S_, perr, dp32, 4 * dp32))
    assert perr <= 4 * dp32
    assert int(torch.count_nonzero(uvn.cpu()[..., ~meshed])) == 0              # a texel no dense face names
    assert float((uvn.cpu().norm(dim=1)[meshed[None] & ~aside] - 1).abs().max()) < 1e-5
    # on the device: the fused kernel against the mesh kernel on the dense faces, fed the fused kernel's own dense vertices
    vn = SR.vertex_normals(dense, L.dense_topology()).reshape(-1, S_, S_, 3).permute(0, 3, 1, 2)
    cross = float((vn - uvn)[keep.cuda()].abs().max())
    print('uv %d fused kernel against shape_render.vertex_normals on its dense vertices: %.3e (bar %.3e)' % (S_, cross, 4 * d32))
    assert cross <= 4 * d32


def test_uv_refused_arguments():
    dt = _dt()
    verts, faces, _, uv, uvfaces, mask, fixed, uv_z, L = _sheet(16)
    n = torch.zeros_like(verts).cuda()
    with pytest.raises(RuntimeError, match='UvLayout'):
        dt.world2uv(None, verts.cuda())
    with pytest.raises(RuntimeError, match='GPU'):
        dt.world2uv(L, verts)
    with pytest.raises(RuntimeError, match=r'\[B,169,3\]'):
        dt.world2uv(L, verts.cuda()[:, :100])
    with pytest.raises(RuntimeError, match='uv_z of shape'):
        dt.detail_normals(L, uv_z.cuda()[:, :, :8], verts.cuda(), n)
    with pytest.raises(RuntimeError, match='GPU'):
        dt.detail_normals(L, uv_z, verts.cuda(), n)


# ------------------------------------------------------------------------------------------------------------------ the detail shade
ALL = ('shape', 'shape_detail', 'grid', 'detail_normal_images', 'alpha', 'pix_to_face', 'zbuf', 'bary')
SHADE_CASES = [(16, 16, 1, False, False), (24, 40, 2, False, True), (40, 16, 2, True, False), (40, 40, 1, True, True)]


@pytest.mark.parametrize('size,Su,rows,to_border,background', SHADE_CASES,
                         ids=['S%d_Su%d_rows%d%s%s' % (c[0], c[1], c[2], '_border' if c[3] else '', '_images' if c[4] else '') for c in SHADE_CASES])
def test_detail_shade_matches_the_restatement(size, Su, rows, to_border, background):
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    verts, faces, cam, uv, uvfaces, mask, fixed, _, L = _sheet(Su, rows=rows, to_border=to_border)
    uvn = S.counter_tensor(SEED, 'detail.shade.uvn.%d' % Su, (rows, 3, Su, Su))
    uvn = uvn / uvn.norm(dim=1, keepdim=True)
    images = S.counter_tensor(SEED, 'detail.shade.bg.%d' % size, (rows, 3, size, size), 0.5, 0.2) if background else None
    topo = SR.MeshTopology(faces, verts.shape[1])
    kw = {'cam': cam.cuda(), 'size': size, 'images': None if images is None else images.cuda()}
    got = SR.render_shape(verts.cuda(), topo, layout=L, detail_normals=uvn.cuda(), want=ALL, **kw)
    old = SR.render_shape(verts.cuda(), topo, want=('shape', 'alpha', 'pix_to_face', 'zbuf', 'bary'), **kw)
    for k in old:                                                                    # one rasterisation, the old entry's bits
        assert _same(old[k], got[k]), k
    only = SR.render_shape(verts.cuda(), topo, layout=L, detail_normals=uvn.cuda(), want=('shape', 'shape_detail'), **kw)
    assert _same(only['shape_detail'], got['shape_detail']) and _same(only['shape'], old['shape'])
    face_uv = L.face_uv
    r64 = R.render(verts, faces, size, cam=cam, images=images)
    r32 = R.render(verts, faces, size, cam=cam, images=images, dtype=torch.float32)
    d64 = RD.detail_shade(r64, face_uv, uvn, images=images)
    d32s = RD.detail_shade(r32, face_uv, uvn, images=images, dtype=torch.float32)
    amb = r64['ambiguous']
    share = amb.reshape(rows, -1).double().mean(1)
    assert float(share.max()) <= 0.02, share
    clear = ~amb
    assert torch.equal(got['pix_to_face'].cpu().long()[clear], r64['pix_to_face'][clear])
    fair = clear & (r32['pix_to_face'] == r64['pix_to_face'])
    sel = {'grid': lambda m: m[..., None].expand(-1, -1, -1, 2), 'detail_normal_images': lambda m: m[:, None].expand(-1, 3, -1, -1),
           'shape_detail': lambda m: m[:, None].expand(-1, 3, -1, -1)}
    for k in ('grid', 'detail_normal_images', 'shape_detail'):
        d32 = float((d32s[k].double() - d64[k])[sel[k](fair)].abs().max())
        dev = float((got[k].cpu().double() - d64[k])[sel[k](clear)].abs().max())
        print('shade S=%d Su=%d rows=%d: %-20s hip deviation %.3e   d32 %.3e   bar %.3e' % (size, Su, rows, k, dev, d32, 4 * d32))
        assert dev <= 4 * d32, (k, dev, d32)
    covered = r64['pix_to_face'] >= 0
    assert int(torch.count_nonzero(got['grid'].cpu()[~covered])) == 0 and int(torch.count_nonzero(got['detail_normal_images'].cpu().permute(0, 2, 3, 1)[~covered])) == 0
    assert float((got['shape_detail'] - got['shape']).abs().max()) > 0.05          # the detail normals do change the panel
    if to_border:
        near = covered & (d64['grid'][..., 0] > 1 - 1.0 / Su)                         # g.x within half a texel of +1: a neighbour outside
        print('shade S=%d Su=%d: %d pixels sample the UV map across its border' % (size, Su, int(near.sum())))
        assert int(near.sum()) > 0


def test_detail_shade_refused_arguments():
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    verts, faces, cam, _, _, _, _, _, L = _sheet(16, rows=1)
    topo = SR.MeshTopology(faces, verts.shape[1])
    v, c, n = verts.cuda(), cam.cuda(), torch.zeros(1, 3, 16, 16, device='cuda')
    with pytest.raises(RuntimeError, match='together'):
        SR.render_shape(v, topo, cam=c, size=16, layout=L)
    with pytest.raises(RuntimeError, match='together'):
        SR.render_shape(v, topo, cam=c, size=16, detail_normals=n)
    with pytest.raises(RuntimeError, match='want'):
        SR.render_shape(v, topo, cam=c, size=16, want=('shape', 'shape_detail'))
    with pytest.raises(RuntimeError, match='detail_normals of shape'):
        SR.render_shape(v, topo, cam=c, size=16, layout=L, detail_normals=n[:, :, :8])
    with pytest.raises(RuntimeError, match='GPU'):
        SR.render_shape(v, topo, cam=c, size=16, layout=L, detail_normals=n.cpu())


# ------------------------------------------------------------------------------------------------------------------ composition
def _flame_case():
    """The synthetic FLAME of the shape renderer's tests, a UV atlas that gives every face of its soup a cell of its own on a 100 x 100
    grid, drawn large enough to overlap its neighbours so that the map is covered (all UV vertices sit at depth 1: where two overlap
    the table takes the lower face, and the restatement is given that table), seeded maps and codes."""
    from stylegan_directions_face_reenactment_amd.flame import FLAME
    from test_cpu_flame import flame_state
    from test_cpu_shape_render import FLAME_ROWS, FLAME_SEED, flame_codedict
    if 'flame' not in _CACHE:
        m = FLAME()
        m.load_state_dict(flame_state(FLAME_SEED))
        faces = m.faces_tensor.long()
        nf = faces.shape[0]
        f = torch.arange(nf, dtype=torch.float64)
        cell = torch.stack([f % 100, torch.div(f, 100, rounding_mode='floor')], 1) / 100.0
        corner = torch.tensor([[-0.41, -0.39], [1.73, -0.31], [-0.33, 1.69]], dtype=torch.float64) / 100.0
        uv = (cell[:, None] + corner[None]).reshape(-1, 2)
        uvfaces = torch.arange(3 * nf).reshape(nf, 3)
        mask = (S.counter_tensor(SEED, 'detail.flame.mask', (256, 256)) > -0.7).float()
        fixed = S.counter_tensor(SEED, 'detail.flame.fixed', (256, 256), 0.0, 0.003)
        L = _dt().UvLayout(faces, uv, uvfaces, 256, mask, fixed, n_vertices=int(m.v_template.shape[0]))
        code = {k: v.cuda() for k, v in flame_codedict().items()}
        code['detail'] = S.counter_tensor(SEED, 'detail.flame.code', (FLAME_ROWS, 128)).cuda()
        _CACHE['flame'] = (m.cuda(), L, code, mask, fixed)
    return _CACHE['flame']


def test_decode_detail_end_to_end():
    """The composition on the synthetic FLAME, B = 2, a 224 image and a 256 UV map.  Every stage is compared on the inputs the device
    gave it (uv_z from the device for the normals, the device's normal map for the shade): the wiring is what is checked here --
    the latent's order, the mask, fixed_dis, the coarse normals, one rasterisation for both panels."""
    dt = _dt()
    from stylegan_directions_face_reenactment_amd import flame as FL
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    m, L, code, mask, fixed = _flame_case()
    D = _decoder(int(golden(KAT)['seed']))
    out = dt.decode_detail(m, D, L, code)
    assert list(out) == ['uv_z', 'displacement_map', 'uv_detail_normals', 'shape_images', 'shape_detail_images', 'detail_normal_images']
    again = dt.decode_detail(m, D, L, code)
    for k in out:
        assert _same(out[k], again[k]), k
    assert _same(FL.shape_detail_images(m, D, L, code), out['shape_detail_images'])
    assert _same(FL.shape_images(m, code), out['shape_images'])
    # D_detail on the latent of deca.py:167
    z = torch.cat([code['pose'][:, 3:], code['alpha_exp'], code['detail']], 1).cpu()
    folded = [t.cpu() for t in D.folded(torch.float64)]
    z64, z32 = RD.decoder_chain(folded, z, D.out_scale)[0], RD.decoder_chain(folded, z, D.out_scale, dtype=torch.float32)[0]
    dev, err = float((z32.double() - z64).abs().max()), float((out['uv_z'].cpu().double() - z64).abs().max())
    print('decode_detail uv_z: hip deviation %.3e = %.2f x the stock fp32 chain\'s %.3e (bar 8 x)' % (err, err / dev, dev))
    assert err <= 8 * dev
    assert _same(out['displacement_map'], out['uv_z'] + fixed.cuda()[None, None])
    # the UV pass on the device's uv_z, vertices and coarse normals
    with torch.no_grad():
        verts = m(code['alpha_shp'], code['alpha_exp'], code['pose'])[0].contiguous()
    topo = FL.topology(m)
    normals = SR.vertex_normals(verts, topo)
    faces = m.faces_tensor.cpu().long()
    _, pix, bary, _, _, _ = L.tables('cuda')
    args = (out['uv_z'].cpu(), verts.cpu(), normals.cpu(), faces, pix.cpu().long(), bary.cpu(), mask, fixed)
    n64, _, raw = RD.displacement2normal(*args)
    n32, _, _ = RD.displacement2normal(*args, dtype=torch.float32)
    meshed = _meshed(256)
    ill = meshed[None] & (raw < 1e-3 * raw[:, meshed].median())
    share = ill.reshape(ill.shape[0], -1).double().mean(1)
    keep = (~ill)[:, None].expand(-1, 3, -1, -1)
    d32, err = float((n32.double() - n64)[keep].abs().max()), float((out['uv_detail_normals'].cpu().double() - n64)[keep].abs().max())
    print('decode_detail uv_detail_normals: hip deviation %.3e   d32 %.3e   bar %.3e; ill-conditioned share %s' % (err, d32, 4 * d32, share.tolist()))
    assert float(share.max()) <= 0.02 and err <= 4 * d32
    # the two panels on the device's normal map
    cam = code['cam'].cpu()
    r64, r32 = R.render(verts.cpu(), faces, 224, cam=cam), R.render(verts.cpu(), faces, 224, cam=cam, dtype=torch.float32)
    uvn = out['uv_detail_normals'].cpu()
    d64, d32s = RD.detail_shade(r64, L.face_uv, uvn), RD.detail_shade(r32, L.face_uv, uvn, dtype=torch.float32)
    clear = ~r64['ambiguous']
    fair = (clear & (r32['pix_to_face'] == r64['pix_to_face']))[:, None].expand(-1, 3, -1, -1)
    clear = clear[:, None].expand(-1, 3, -1, -1)
    for k, name in (('detail_normal_images', 'detail_normal_images'), ('shape_detail', 'shape_detail_images')):
        d32 = float((d32s[k].double() - d64[k])[fair].abs().max())
        err = float((out[name].cpu().double() - d64[k])[clear].abs().max())
        print('decode_detail %s: hip deviation %.3e   d32 %.3e   bar %.3e' % (name, err, d32, 4 * d32))
        assert err <= 4 * d32
    assert float((out['shape_detail_images'] - out['shape_images']).abs().max()) > 0.01


def test_decode_detail_graph_replay_equals_the_eager_call():
    dt = _dt()
    m, L, code, _, _ = _flame_case()
    D = _decoder(int(golden(KAT)['seed']))
    eager = dt.decode_detail(m, D, L, code, gan_range=True)                          # packs and the UV table exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = dt.decode_detail(m, D, L, code, gan_range=True)
    for k in held:
        held[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert _same(held[k], eager[k]), k
    assert float(eager['shape_detail_images'].min()) >= -1 and float(eager['shape_detail_images'].max()) <= 1


def test_decode_detail_refused_arguments():
    """Every refusal comes before the first launch: the outputs of an earlier call stay as they are."""
    dt = _dt()
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    m, L, code, mask, fixed = _flame_case()
    D = _decoder(int(golden(KAT)['seed']))
    bad = dict(code, detail=code['detail'][:, :100])                                 # a latent of 153 columns
    with pytest.raises(RuntimeError, match=r'detail code of shape \[2,128\]'):
        dt.decode_detail(m, D, L, bad)
    with pytest.raises(RuntimeError, match='GPU'):
        dt.decode_detail(m, D, L, dict(code, detail=code['detail'].cpu()))
    with pytest.raises(RuntimeError, match='size must be'):
        dt.decode_detail(m, D, L, code, size=5000)
    with pytest.raises(RuntimeError, match='UvLayout'):
        dt.decode_detail(m, D, None, code)
    small = dt.UvLayout(L.faces, torch.rand(30, 2, dtype=torch.float64), torch.randint(0, 30, tuple(L.faces.shape)), 40, torch.ones(40, 40),
                        torch.zeros(40, 40), n_vertices=L.n_vertices)
    with pytest.raises(RuntimeError, match='uv_size=40'):
        dt.decode_detail(m, D, small, code)
    with torch.no_grad():
        verts = m(code['alpha_shp'], code['alpha_exp'], code['pose'])[0].contiguous()
    with pytest.raises(RuntimeError, match='together'):
        SR.render_shape(verts, SR.MeshTopology.from_flame(m), cam=code['cam'], layout=L)

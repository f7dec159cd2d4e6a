"""GPU: the DECA render-side kernels (csrc/detail.hip, csrc/texture.hip, csrc/mesh_sample.h) at the wave, tile, slice and size seams
their feature tests leave open.  The cases are tests/render_seam_cases.py; tests/test_cpu_render_seams.py proves on the CPU, with
tests/plan_rules.py and the restatements alone, what each case reaches and that every cap holds.  Every comparison is with a float64
computation on the CPU; two HIP runs are compared only where their bits must be equal, on top of that.

Bars (none taken from the code under test; each is the one the project already uses for the quantity).
  Layer kernel  max(8 x dev, 1e-6 max|y|), dev = the stock fp32 chain (F.interpolate + F.conv2d) against the same in fp64, for border
                rows, border columns and the interior apart, at slope 0.2 and at slope 1; detail_finish_kernel launches = the rule's.
  FLAMETex      max(8 x dev, 1e-6 max|y|) for every row of every batch, dev = texture_restatement.flametex in fp32 against fp64 on
                the same rows; row r of a batch is the one-row call's bits.
  Sampler       exactly 0 where nothing is sampled; the texel's bits at a centre float32 holds exactly; else 4 x d32 of
                detail_restatement.grid_sample in float32 against F.grid_sample in float64, floor 1e-6 max|image|.
  UV passes     4 x d32 of the float64 restatement on the same table; ambiguous and short-normal texels set aside under the 2 % cap;
                uncovered texels exactly 0.  Lattice coverage at 1, 8 and 17: pix_to_face equal, nothing excluded.
Each test prints its own figures.

What could not be built as the issue words it, and what stands in its place:
  * `every texel centre bit for bit`: (2j + 1)/3 - 1 and (2j + 1)/5 - 1 are no float32 numbers, so on the 5 x 3 image only the
    centres whose restated float32 index is the integer itself are held to the texel's bits (8 of 15); the others to the general bar.
  * +-inf through the table the issue gives (faces (f, f, f), bary (1, 0, 0)) reaches the sampler as NaN, 0 x inf.  That table is
    run as given; a second one, faces (f, Z, Z) with Z a vertex of zeros inside the table, hands +-inf on unchanged.
  * the unaligned FLAMETex call: FlameTex.forward allocates its output and takes the pack from the module's cache, so the Python entry
    cannot be handed a view off a 16-byte boundary, and no API is added for it.  The C entry is called through _native with the
    same pack and output four bytes further on; it must give the aligned call's bits.
  * the last tile column and row of a UV size 16 k + 1 hold no meshed texel (the dense faces end at S - 3 and S - 6), so no normal
    there can come from a halo.  Checked instead: at 33 the texel (16, 16), whose upper and left neighbours are staged through
    the halo from three other tiles, is meshed, not set aside and within the bar; the covered texels (8, 16) at 17 and (16, 32) at
    33 of the one-texel tiles get their dense vertex and a normal of exactly 0.
  * the detail shade's `grid` path is not fed the chosen coordinates: its grid is interpolated from face_uv by the rasteriser's
    barycentrics, which cannot place a coordinate exactly.

Measured on an MI355X (DESIGN.md 4.34 has the table per case):
  layer kernel  worst region of each case, hip deviation / its bar: 1.3e-7 / 1.5e-6 ... 2.0e-6 / 6.9e-6 ((2, 29, 17, 5, 3) plain, the
                largest share of a bar, 0.29); 0.19 ... 2.29 x the stock fp32 chain's deviation; conv and finish launches as planned.
  FLAMETex      rows 8 ... 41: 3.9e-8 ... 6.0e-8 (bars 1.0e-6); components 1 ... 17: 3.7e-8 ... 6.8e-8 (bars 0.9 ... 1.2e-6), 200:
                7.3e-7 (stock 2.4e-7, bar 2.0e-6); uv 5, 10, 11, 12: 4.8e-8 ... 6.7e-8 (bars 0.9 ... 1.1e-6); every row equal to its
                one-row call; off the 16-byte boundary (pack, output, both) the aligned bits.
  sampler       4 x 4, 5 x 3, 1 x 1: 297 / 225 / 231 points exactly 0, 16 / 8 / 1 centres equal their texel; seam points 0 / 1.5e-7 /
                0, general points 8.6e-8 / 2.2e-7 / 9.1e-8 = d32 (bars 8.9e-7 / 9.4e-7 / 9.1e-7, the floor).
  UV passes     13, 17, 33: nothing set aside; world2uv 6.7e-8 / 7.9e-8 / 8.5e-8 (bars 2.7e-7 / 3.2e-7 / 3.4e-7), normals 3.9e-7 /
                5.1e-7 / 1.3e-6 (bars 1.6e-6 / 2.1e-6 / 5.2e-6), dense vertices 1.0e-7 / 1.2e-7 / 1.1e-7 (bars 4.1e-7 / 4.9e-7 /
                4.5e-7), the five texture maps 6.0e-8 ... 2.9e-7 (bars 2.4e-7 ... 1.2e-6); texel (16, 16) at 33: 2.8e-7.
  wall time of the module: 5 s for its 75 cases.
Found and fixed: nothing in the kernels.

What each test is known to catch, from a mutation of the kernels (built apart, never committed; each changes values only and
touches no memory the unmutated launch does not):
  in flametex_kernel at WAVES = 4, wave 1's accumulators reading the code rows of wave 0 (`c` eight rows down in the LDS table, the
      row range unchanged): test_flametex_rows_across_the_instances[17, 32, 33, 41], all of
      test_flametex_components_around_the_prefetch_depth and test_flametex_paths_and_blocks; test_gpu_texture passes with it;
  the store guard `row0 + r < rows` as `row0 + r + 1 < rows` (the last valid row is skipped): every FLAMETex test here, the unaligned
      ones included, and test_gpu_texture's (its 40-row batch does compare row 39);
  for_each_output's `bb` taken from the tile's first pixel, `p` left right (a tile's second row filed under its first): the twelve
      test_upconv_across_its_plan cases with a tile over rows, and of the earlier tests only those that run the decoder at three rows
      (kat22 b3) or compose it; the four earlier upconv cases pass;
  grid_sample3's `x >= W` as `x >= W - 1` (the neighbour in the last column dropped): the three
      test_grid_sample3_at_chosen_coordinates cases and the three UV sizes here, and three of six test_uv_textures cases;
  load_w's channel guard `gn < N` dropped where the neighbouring word lies inside the pack: NOT caught, by nothing old or new, and
      it cannot be: the weight rows beyond Cout feed accumulator rows that for_each_output never stores (`gn >= N`), so this
      mutant computes the same output.  What the partial channel tiles do prove is the store guard: the 65- and 80-channel cases
      compare every channel and would show a neighbour's values in channel 64 .. 79 or a write beyond them.
"""
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

pytestmark = pytest.mark.gpu

_CACHE = {}


def _dt():
    from stylegan_directions_face_reenactment_amd import detail
    return detail


def _tx():
    from stylegan_directions_face_reenactment_amd import texture
    return texture


def _N():
    from stylegan_directions_face_reenactment_amd import _native
    return _native


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- the layer kernel
def _detail_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return out, (sum('detail_conv_kernel' in n for n in names), sum('detail_finish_kernel' in n for n in names))


@pytest.mark.parametrize('up', [True, False], ids=['up', 'plain'])
@pytest.mark.parametrize('case', RS.UPCONV, ids=RS.UPCONV_IDS)
def test_upconv_across_its_plan(case, up):
    rows, cin, cout, h, w = case
    plan = P.detail_plan(*case, up)
    x, wt, b = RS.upconv_inputs(case)
    pre64, pre32 = RS.upconv_reference(case, up), RS.upconv_reference(case, up, dtype=torch.float32)
    assert 0.2 < float((pre64 < 0).double().mean()) < 0.8                   # the activation's both sides are exercised
    xc, wc, bc = x.cuda(), wt.cuda(), b.cuda()
    print('upconv %s up=%d: tile %d, %d x %d tiles, %d chunks in %d slices of %d (last %d), K tail %d, seams %s'
          % (case, up, plan.bn, plan.mt, plan.nt, plan.chunks, plan.S, plan.cps, plan.last, plan.ktail, sorted(P.detail_seams(*case, up))))
    for slope in RS.SLOPES:
        got, counts = _detail_launches(lambda: _dt().upconv(xc, wc, bc, slope=slope, up=up))
        assert counts == P.detail_counts(*case, up), (counts, plan)
        ref, stock = F.leaky_relu(pre64, slope), F.leaky_relu(pre32, slope).double()
        assert tuple(got.shape) == tuple(ref.shape) == (rows, cout, plan.Ho, plan.Wo)
        got = got.double().cpu()
        scale = float(ref.abs().max())
        for name, m in RS.border_masks(plan.Ho, plan.Wo):
            if not bool(m.any()):
                print('upconv %s up=%d slope %.1f %-11s no such pixel' % (case, up, slope, name))
                continue
            dev, err = float((stock - ref)[..., m].abs().max()), float((got - ref)[..., m].abs().max())
            bar = max(8 * dev, 1e-6 * scale)
            print('upconv %s up=%d slope %.1f %-11s hip %.3e, stock fp32 %.3e (ratio %.2f), bar %.3e, max|y| %.3e'
                  % (case, up, slope, name, err, dev, err / max(dev, 1e-30), bar, scale))
            assert err <= bar, (name, err, bar)


# ---------------------------------------------------------------------------------------------------------------- FLAMETex
def _flametex(n_tex, source, uv):
    """Per space, once per process: the module on the device, the float64 and stock float32 albedo of all 41 code rows, and the
    one-row call of every row."""
    key = ('T', n_tex, source, uv)
    if key not in _CACHE:
        mean, basis = RT.synthetic_space(S, SEED, source, n_tex)
        T = _tx().FlameTex(n_tex, source, uv)
        T.load_state_dict({'texture_mean': mean, 'texture_basis': basis})
        T = T.cuda()
        assert _same(T.packed(), T.host_pack())                             # the prepack launch writes the documented layout
        code = RS.flametex_code(n_tex)
        ref = RT.flametex(mean, basis, code, source, uv)
        stock = RT.flametex(mean, basis, code, source, uv, dtype=torch.float32).double()
        _CACHE[key] = (T, code.cuda(), ref, stock)
    return _CACHE[key]


def _single_rows(T, code, rows):
    return torch.cat([T(code[r:r + 1]) for r in range(rows)])


def _check_flametex(tag, n_tex, source, uv, rows, singles=None):
    T, code, ref, stock = _flametex(n_tex, source, uv)
    got = T(code[:rows])
    assert tuple(got.shape) == (rows, 3, uv, uv) and got.dtype == torch.float32
    g = got.double().cpu()
    err = (g - ref[:rows]).abs().flatten(1).max(1).values                   # per row
    dev, scale = float((stock[:rows] - ref[:rows]).abs().max()), float(ref[:rows].abs().max())
    bar = max(8 * dev, 1e-6 * scale)
    worst = int(err.argmax())
    print('flametex %s: %d -> %d n_tex=%d rows=%d path %s instance %s: hip %.3e (row %d), stock fp32 %.3e, bar %.3e, max|y| %.3e'
          % (tag, source, uv, n_tex, rows, RS.flametex_path(3 * uv * uv), RS.flametex_instance(rows), float(err.max()), worst, dev, bar, scale))
    assert bool((err <= bar).all()), [(r, float(e)) for r, e in enumerate(err) if e > bar]
    singles = _single_rows(T, code, rows) if singles is None else singles[:rows]
    same = (got == singles).flatten(1).all(1)
    assert bool(same.all()), 'rows that differ from their one-row call: %s' % (~same).nonzero().flatten().tolist()
    return got


@pytest.mark.parametrize('rows', RS.FLAMETEX_ROWS)
def test_flametex_rows_across_the_instances(rows):
    source, uv, n_tex = RS.FLAMETEX_BASE
    T, code, _, _ = _flametex(n_tex, source, uv)
    if 'singles' not in _CACHE:
        _CACHE['singles'] = _single_rows(T, code, RS.FLAMETEX_MAX_ROWS)
    _check_flametex('rows', n_tex, source, uv, rows, _CACHE['singles'])


@pytest.mark.parametrize('n_tex', RS.FLAMETEX_COMPONENTS)
def test_flametex_components_around_the_prefetch_depth(n_tex):
    source, uv, _ = RS.FLAMETEX_BASE
    _check_flametex('components', n_tex, source, uv, 17)


@pytest.mark.parametrize('source,uv', RS.FLAMETEX_PATHS, ids=['%dto%d' % c for c in RS.FLAMETEX_PATHS])
def test_flametex_paths_and_blocks(source, uv):
    _check_flametex('paths', RS.FLAMETEX_BASE[2], source, uv, 17)


@pytest.mark.parametrize('source,uv', [RS.FLAMETEX_BASE[:2], RS.FLAMETEX_PATHS[3]], ids=['12to6', '17to12'])
def test_flametex_off_a_16_byte_boundary_gives_the_aligned_bits(source, uv):
    """3 uv^2 is a multiple of 4 here: the aligned call takes 16-byte loads, the same data four bytes further on the dword path."""
    N = _N()
    n_tex, rows = RS.FLAMETEX_BASE[2], 17
    T, code, ref, _ = _flametex(n_tex, source, uv)
    P_ = 3 * uv * uv
    assert P_ % 4 == 0
    aligned = T(code[:rows])
    pack = T.packed()
    shifted = torch.empty(pack.numel() + 1, dtype=torch.float32, device='cuda')
    shifted[1:].copy_(pack)
    c = code[:rows].contiguous()
    assert pack.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
    for tag, pk, off in (('pack', shifted[1:], 0), ('output', pack, 1), ('both', shifted[1:], 1)):
        out = torch.full((rows * P_ + 1,), float('nan'), dtype=torch.float32, device='cuda')
        view = out[off:off + rows * P_]
        assert (view.data_ptr() % 16 != 0) == bool(off) and (pk.data_ptr() % 16 != 0) == (tag != 'output')
        N.call('sgdfr_flametex_forward_f32', N.ptr(c), rows, N.ptr(pk), uv, n_tex, N.ptr(view), N.stream())
        assert _same(view.view(rows, 3, uv, uv), aligned), tag
        rest = out[rows * P_:] if off == 0 else out[:1]
        assert bool(torch.isnan(rest).all()), tag                           # nothing is written beside the rows
    print('flametex %d -> %d off the boundary (pack, output, both): the aligned bits; max |hip - fp64| %.3e'
          % (source, uv, float((aligned.double().cpu() - ref[:rows]).abs().max())))


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _uv_pass(tv, image, Su, V, faces, pix, bary):
    """sgdfr_texture_uv_f32 on a hand-made table: -> (uv_pverts, uv_gt) [1,3,Su,Su]"""
    N = _N()
    from stylegan_directions_face_reenactment_amd.shape_render import sh_constants
    dev = 'cuda'
    uvn = torch.zeros(1, 3, Su, Su, device=dev)
    uvn[:, 2] = 1.0
    light, mask = torch.zeros(1, 9, 3, device=dev), torch.ones(Su, Su, device=dev)
    tvc, im, fc, pc, bc = tv.cuda().contiguous(), image.cuda().contiguous(), faces.cuda(), pix.cuda(), bary.cuda().contiguous()
    pverts, gt = torch.full((1, 3, Su, Su), 7.0, device=dev), torch.full((1, 3, Su, Su), 7.0, device=dev)
    N.call('sgdfr_texture_uv_f32', None, N.ptr(uvn), N.ptr(light), sh_constants(), N.ptr(tvc), N.ptr(im), 1, V, image.shape[2], image.shape[3],
           N.ptr(fc), faces.shape[0], N.ptr(pc), N.ptr(bc), N.ptr(mask), Su, None, None, None, N.ptr(pverts), N.ptr(gt), N.stream())
    torch.cuda.synchronize()
    return pverts.cpu(), gt.cpu()


@pytest.mark.parametrize('H,W', RS.SAMPLER_IMAGES, ids=['%dx%d' % s for s in RS.SAMPLER_IMAGES])
def test_grid_sample3_at_chosen_coordinates(H, W):
    r = RS.sampler_reference(H, W)
    pts, tags, img = r['pts'], r['tags'], r['image']
    n = pts.shape[0]
    finite = torch.isfinite(pts)
    results = {}
    for zero_vertex in (False, True):
        Su, V, faces, pix, bary = RS.sampler_table(n, zero_vertex)
        tv = RS.sampler_vertices(pts, Su, V)
        pverts, gt = _uv_pass(tv, img, Su, V, faces, pix, bary)
        # first: the table hands the chosen coordinate to the sampler, bit for bit
        pv = pverts[0].reshape(3, -1)
        got_xy = pv[:2, :n].T
        assert torch.equal(got_xy[finite], pts[finite]) and torch.equal(pv[2], tv[0, :Su * Su, 2])
        if zero_vertex:
            assert torch.equal(got_xy[torch.isinf(pts)], pts[torch.isinf(pts)]) and bool(torch.isnan(got_xy[torch.isnan(pts)]).all())
        else:
            assert bool(torch.isnan(got_xy[~finite]).all())                 # 1 v + 0 v + 0 v with v = +-inf
        results[zero_vertex] = gt[0].reshape(3, -1)[:, :n]
        # the texels behind the last point sample (0, 0), the image centre: never the filler
        assert bool((gt != 7.0).all())
    assert _same(results[False], results[True])
    got = results[True]
    # nothing sampled: exactly 0 in every channel (outside, far, non-finite, alone and in every combination)
    zero = r['zero']
    by = lambda tag: torch.tensor([tag in t for t in tags])
    for tag in RS.ZERO_TAGS:
        m = by(tag)
        assert int(m.sum()) > 0 and int(torch.count_nonzero(got[:, m])) == 0, tag
    assert int(torch.count_nonzero(got[:, zero])) == 0 and not bool(torch.isnan(got).any())
    # an exact centre: the texel's bits
    ex, (ty, tx) = r['exact'], r['texel']
    assert torch.equal(got[:, ex], img[0][:, ty[ex], tx[ex]])
    # the rest: the seam points (edges, partial neighbours, centres float32 cannot hold) and the general points, apart
    floor = 1e-6 * float(img.abs().max())
    for name, m in (('seam', r['seam']), ('general', r['general'])):
        d32 = float((r['r32'] - r['ref'])[:, m].abs().max())
        err = float((got.double() - r['ref'])[:, m].abs().max())
        bar = max(4 * d32, floor)
        print('sampler %d x %d %-8s %3d points: hip deviation %.3e   d32 %.3e   bar %.3e' % (H, W, name, int(m.sum()), err, d32, bar))
        assert err <= bar, (name, err, bar)
    print('sampler %d x %d: %d points exactly 0, %d exact centres equal their texel' % (H, W, int(zero.sum()), int(ex.sum())))


# ---------------------------------------------------------------------------------------------------------------- the UV passes
@pytest.mark.parametrize('Su', RS.UV_SIZES)
def test_uv_passes_at_small_and_tile_edge_sizes(Su):
    dt, tx = _dt(), _tx()
    i = RS.uv_inputs(Su)
    rows = RS.UV_ROWS
    L = dt.UvLayout(i['faces'], i['uv'], i['uvfaces'], Su, i['mask'], i['fixed'], n_vertices=i['verts'].shape[1])
    _, pix, bary, _, _, _ = L.tables('cuda')
    pix, bary = pix.cpu().long(), bary.cpu()
    pr, _, _, amb = R.rasterize(L.uv_vertices.double()[None], i['uvfaces'], Su)
    pr, amb = pr[0], amb[0]
    assert torch.equal(pix[~amb], pr[~amb])
    none = pix < 0
    v, nrm, z = i['verts'].cuda(), i['normals'].cuda(), i['uv_z'].cuda()
    # world2uv
    got = dt.world2uv(L, v)
    w64 = RD.world2uv(i['verts'], i['faces'], pix, bary)
    w32 = RD.world2uv(i['verts'], i['faces'], pix, bary, dtype=torch.float32)
    d32, err = float((w32.double() - w64)[..., ~amb].abs().max()), float((got.cpu().double() - w64)[..., ~amb].abs().max())
    print('uv %d world2uv: hip deviation %.3e   d32 %.3e   bar %.3e; %d texels uncovered' % (Su, err, d32, 4 * d32, int(none.sum())))
    assert err <= 4 * d32 and int(torch.count_nonzero(got.cpu()[..., none])) == 0
    # displacement2normal
    uvn, dense = dt.detail_normals(L, z, v, nrm, dense_vertices=True)
    args = (i['uv_z'], i['verts'], i['normals'], i['faces'], pix, bary, i['mask'], i['fixed'])
    n64, p64, raw = RD.displacement2normal(*args)
    n32, p32, _ = RD.displacement2normal(*args, dtype=torch.float32)
    aside, share = RS.uv_set_aside(raw, amb, Su)
    print('uv %d: set aside %s of the map' % (Su, ['%.4f' % s for s in share.tolist()]))
    assert float(share.max()) <= TC.CAP
    keep = (~aside)[:, None].expand(-1, 3, -1, -1)
    d32, err = float((n32.double() - n64)[keep].abs().max()), float((uvn.cpu().double() - n64)[keep].abs().max())
    print('uv %d detail normals: hip deviation %.3e   d32 %.3e   bar %.3e' % (Su, err, d32, 4 * d32))
    assert err <= 4 * d32
    dp32, perr = float((p32.double() - p64).abs().max()), float((dense.cpu().double() - p64).abs().max())
    print('uv %d dense vertices: hip deviation %.3e   d32 %.3e   bar %.3e' % (Su, perr, dp32, 4 * dp32))
    assert perr <= 4 * dp32
    m = RS.meshed(Su)
    assert int(torch.count_nonzero(uvn.cpu().permute(0, 2, 3, 1)[:, ~m])) == 0          # a texel no dense face names
    assert float((uvn.cpu().norm(dim=1)[m[None] & ~aside] - 1).abs().max()) < 1e-5
    # the named texels
    halo, last = RS.UV_HALO_TEXEL[Su], RS.UV_LAST_TILE_TEXEL[Su]
    if halo is not None:
        y, x = halo
        assert bool(m[y, x]) and not bool(aside[:, y, x].any())
        herr = float((uvn.cpu().double() - n64)[:, :, y, x].abs().max())
        print('uv %d texel (%d, %d), neighbours through the halo: hip deviation %.3e   bar %.3e' % (Su, y, x, herr, 4 * d32))
        assert herr <= 4 * d32 and float(uvn[:, :, y, x].norm(dim=1).min()) > 0.99
    if last is not None:
        y, x = last
        dn = dense.cpu().reshape(rows, Su, Su, 3)
        for yy, xx in ((y, x), (x, y)):                                      # the last tile column, the last tile row
            assert int(pix[yy, xx]) >= 0 and float(dn[:, yy, xx].abs().max()) > 0.1
            assert float((dn[:, yy, xx].double() - p64.reshape(rows, Su, Su, 3)[:, yy, xx]).abs().max()) <= 4 * dp32
            assert int(torch.count_nonzero(uvn[:, :, yy, xx])) == 0
    # the texture pass
    want = ('uv_shading', 'uv_texture', 'uv_texture_gt', 'uv_pverts', 'uv_gt')
    a, l, tv, im = i['albedo'].cuda(), i['light'].cuda(), i['tv'].cuda(), i['images'].cuda()
    maps = tx.uv_textures(L, a, uvn, l, tv, im, want=want)
    uvn_c = uvn.cpu()
    r64 = RT.uv_textures(i['albedo'], uvn_c, i['light'], i['tv'], i['images'], i['faces'], pix, bary, i['mask'])
    r32 = RT.uv_textures(i['albedo'], uvn_c, i['light'], i['tv'], i['images'], i['faces'], pix, bary, i['mask'], dtype=torch.float32)
    for k in want:
        d32, err = float((r32[k].double() - r64[k]).abs().max()), float((maps[k].cpu().double() - r64[k]).abs().max())
        print('uv %d %-14s hip deviation %.3e   d32 %.3e   bar %.3e' % (Su, k, err, d32, 4 * d32))
        assert err <= 4 * d32, (k, err, d32)
    if int(none.sum()):
        assert int(torch.count_nonzero(maps['uv_pverts'].cpu()[..., none])) == 0
    # row b of the batch is the one-row call, bit for bit; the rows differ
    for b in range(rows):
        s = slice(b, b + 1)
        assert _same(dt.world2uv(L, v[s]), got[s])
        n1, d1 = dt.detail_normals(L, z[s], v[s], nrm[s], dense_vertices=True)
        assert _same(n1, uvn[s]) and _same(d1, dense[s])
        one = tx.uv_textures(L, a[s], uvn[s], l[s], tv[s], im[s], want=want)
        for k in want:
            assert _same(one[k], maps[k][s]), (k, b)
        for c in range(b):
            assert float((uvn[b] - uvn[c]).abs().max()) > 1e-2 and float((maps['uv_gt'][b] - maps['uv_gt'][c]).abs().max()) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- the lattice
@pytest.mark.parametrize('name,size', C.small_pairs(), ids=['%s_%d' % p for p in C.small_pairs()])
def test_lattice_coverage_is_exact_at_the_small_sizes(name, size):
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    verts, faces = C.LATTICE[name]
    want = R.rasterize(verts[None], faces, size)[0]
    pix, zbuf, bary = SR.rasterize(verts.float()[None].cuda(), SR.MeshTopology(faces, verts.shape[0]), size)
    assert pix.dtype == torch.int32 and torch.equal(pix.cpu().long(), want), (name, size)
    none = (pix < 0).cpu()
    assert bool((zbuf.cpu()[none] == -1).all()) and bool((bary.cpu()[none] == -1).all())
    assert bool((zbuf.cpu()[~none] >= 0).all()) and bool((bary.cpu()[~none] > 0).all())


def test_lattice_grid_at_the_small_sizes():
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    verts, faces = C.lattice_grid()
    topo = SR.MeshTopology(faces, verts.shape[0])
    for size in C.SMALL_SIZES:
        want = R.rasterize(verts[None], faces, size)[0]
        pix = SR.rasterize(verts.float()[None].cuda(), topo, size)[0].cpu().long()
        assert torch.equal(pix, want), size
    assert len(want.unique()) > 100

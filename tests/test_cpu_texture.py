"""CPU: the restatements of tests/texture_restatement.py against the reference's own FLAMETex results (kat23) and torch itself, the
host side of texture.FlameTex (the nearest-neighbour index rule, the pack layout, the SH constants), and the inputs of
tests/test_gpu_texture.py: for each of them the restatement alone, float32 against float64, keeps its set-aside share under the cap,
so the inputs are known to be usable before a GPU sees them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import S, golden
import detail_restatement as RD
import shape_render_restatement as R
import texture_cases as TC
import texture_restatement as RT

KAT = 'kat23_deca_texture.npz'


def test_restated_flametex_equals_kat23():
    g = golden(KAT)
    source, uv, n_tex, seed = int(g['source']), int(g['uv']), int(g['n_tex']), int(g['seed'])
    assert (source, uv, n_tex, seed) == (512, 256, 50, RT.KAT_SEED)
    mean, basis = RT.synthetic_space(S, seed, source, n_tex)
    for tag, rows in RT.KAT_BATCHES:
        code = S.counter_tensor(seed, 'kat23.tex.' + tag, (rows, n_tex), 0.0, 1.0)
        sub, brd, sums = RT.digest(RT.flametex_kept(mean, basis, code, source, uv))
        dev = float(g['dev_' + tag])
        e_sub = float((sub - torch.from_numpy(g['sub_' + tag]).double()).abs().max())
        e_brd = float((brd - torch.from_numpy(g['border_' + tag]).double()).abs().max())
        e_sum = float((sums - torch.from_numpy(g['sums_' + tag])).abs().max())
        print('kat23 %s: restatement sample %.3e border %.3e plane sums %.3e; the reference fp32 deviation %.3e' % (tag, e_sub, e_brd, e_sum, dev))
        assert e_sub <= dev and e_brd <= dev and e_sum <= dev * uv * uv
        assert tuple(g['sub_' + tag].shape) == (rows, 3, uv // RT.KAT_SUB, uv // RT.KAT_SUB)


@pytest.mark.parametrize('source,uv', RT.SMALL)
def test_the_two_flametex_restatements_agree(source, uv):
    mean, basis = RT.synthetic_space(S, 7, source, 3)
    code = S.counter_tensor(7, 'code', (2, 3))
    whole, kept = RT.flametex(mean, basis, code, source, uv), RT.flametex_kept(mean, basis, code, source, uv)
    assert tuple(whole.shape) == (2, 3, uv, uv) and float((whole - kept).abs().max()) <= 1e-14


@pytest.mark.parametrize('source,uv', [(512, 256)] + list(RT.SMALL))
def test_nearest_index_equals_interpolate(source, uv):
    from stylegan_directions_face_reenactment_amd.texture import nearest_index
    ours = nearest_index(source, uv)
    assert ours.shape == (uv,) and np.array_equal(ours, RT.interpolate_index(source, uv).numpy())
    x = torch.arange(source * source, dtype=torch.float32).view(1, 1, source, source)              # and in two dimensions at once
    assert torch.equal(F.interpolate(x, [uv, uv])[0, 0], x[0, 0][torch.from_numpy(ours)[:, None], torch.from_numpy(ours)[None, :]])


@pytest.mark.parametrize('source,uv', RT.SMALL)
def test_pack_layout_round_trips(source, uv):
    from stylegan_directions_face_reenactment_amd.texture import FlameTex
    n_tex = 3
    T = FlameTex(n_tex, source, uv)
    mean, basis = RT.synthetic_space(S, 11, source, n_tex)
    T.load_state_dict({'texture_mean': mean, 'texture_basis': basis})
    assert [k for k, _ in T.state_dict().items()] == ['texture_mean', 'texture_basis']
    pack = T.host_pack()
    assert pack.numel() == (1 + n_tex) * 3 * uv * uv
    m, b = T.unpack(pack)
    rows = RT.kept_rows(source, uv)                                        # [uv,uv,3]
    assert torch.equal(m, mean.reshape(-1)[rows].permute(2, 0, 1))
    assert torch.equal(b, basis.reshape(-1, n_tex)[rows].permute(3, 2, 0, 1))
    code = S.counter_tensor(11, 'code', (2, n_tex))
    again = m[None].double() + torch.einsum('kcyx,bk->bcyx', b.double(), code.double())            # the pack alone gives the albedo
    assert float((again - RT.flametex(mean, basis, code, source, uv)).abs().max()) <= 1e-14


def test_flametex_refuses_sizes_out_of_range():
    from stylegan_directions_face_reenactment_amd.texture import FlameTex
    for kw in ({'n_tex': 0}, {'n_tex': 201}, {'uv_size': 1025}, {'source_size': 0}, {'n_tex': 2.5}):
        with pytest.raises(RuntimeError, match='must be an int in'):
            FlameTex(**dict({'n_tex': 2, 'source_size': 4, 'uv_size': 2}, **kw))


def test_sh_constants_equal_the_reference_expression():
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    ref = RT.sh_constants(torch.float32)
    assert len(SR.SH_CONSTANTS) == 9 and torch.equal(torch.tensor(SR.SH_CONSTANTS, dtype=torch.float64).float(), ref)
    n = torch.zeros(1, 3, 1, 1, dtype=torch.float64)                       # add_SHlight at the zero normal: c0 L0 - c8 L8
    light = S.counter_tensor(3, 'light', (1, 9, 3)).double()
    c = RT.sh_constants()
    assert torch.allclose(RT.add_shlight(n, light)[0, :, 0, 0], c[0] * light[0, 0] - c[8] * light[0, 8], rtol=0, atol=1e-15)


def test_restated_grid_sample_is_torchs():
    x = S.counter_tensor(5, 'gs.x', (2, 3, 8, 6)).double()
    g = S.counter_tensor(5, 'gs.g', (2, 7, 5, 2), 0.0, 0.7).double()
    g[0, 0, 0] = 0.0                                                       # the image centre, where an uncovered texel samples
    assert float((RD.grid_sample(x, g) - F.grid_sample(x, g, mode='bilinear', padding_mode='zeros', align_corners=False)).abs().max()) <= 1e-14


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize('size,Su,rows,to_border', TC.RENDER, ids=TC.RENDER_IDS)
def test_render_inputs_keep_the_set_aside_share_under_the_cap(size, Su, rows, to_border):
    verts, faces, cam, uv, uvfaces = TC.sheet(rows, to_border)
    albedo, light, _, _ = TC.maps(rows, Su)
    face_uv = RD.uv_vertices(uv).float()[uvfaces][:, :, :2]
    r64 = RT.texture_render(verts, faces, size, face_uv, albedo, light, cam=cam)
    r32 = RT.texture_render(verts, faces, size, face_uv, albedo, light, cam=cam, dtype=torch.float32)
    aside = r64['ambiguous'] | r64['pos_ambiguous']
    share = aside.reshape(rows, -1).double().mean(1)
    covered = r64['pix_to_face'] >= 0
    print('render S=%d Su=%d rows=%d: set aside %s, covered %.3f' % (size, Su, rows, ['%.4f' % s for s in share.tolist()], float(covered.double().mean())))
    assert float(share.max()) <= TC.CAP
    assert torch.equal(r32['pix_to_face'][~aside], r64['pix_to_face'][~aside])
    assert torch.equal(r32['pos_mask'][:, 0][~aside], r64['pos_mask'][:, 0][~aside].float())
    assert not bool(covered[:, 0, 0].any()) and 0.3 < float(covered.double().mean()) < 0.95       # an uncovered corner, a covered middle
    both = r64['pos_mask'][:, 0][covered]
    assert 0 < float(both.mean()) < 1                                       # the -0.05 threshold is crossed inside the mesh


@pytest.mark.parametrize('rows', [1, 2])
def test_attribute_and_landmark_inputs_keep_the_share_under_the_cap(rows):
    p, faces, tn = TC.sheet_projected(rows)
    sp, sfaces, svalues = TC.stacked(rows)
    for name, proj, f, values, zoff in (('sheet', p, faces, tn, R.Z_OFFSET), ('stacked', sp, sfaces, svalues, 0.0)):
        for size in TC.ATTR_SIZES:
            _, amb, pix = RT.render_attr(proj, values, f, size, zoff)
            _, _, pix32 = RT.render_attr(proj, values, f, size, zoff, dtype=torch.float32)
            _, damb, _ = RT.render_depth(proj, f, size)
            if name == 'stacked':
                # a lattice mesh (shape_render_cases.py): the edges that pass through pixel centres do so where float32 is exact, so
                # NOTHING is set aside for it -- the centres on an edge belong to no face in either precision
                assert torch.equal(pix32, pix) and int(amb.sum()) > 0
                continue
            share = amb.reshape(rows, -1).double().mean(1)
            print('%s S=%d rows=%d: set aside %s' % (name, size, rows, ['%.4f' % s for s in share.tolist()]))
            assert float(share.max()) <= TC.CAP and torch.equal(pix32[~amb], pix[~amb])
            assert float(damb.reshape(rows, -1).double().mean(1).max()) <= TC.CAP
        idx, w = TC.landmarks(len(f))
        vis, z = RT.visofp(values, f, idx, w)
        near = (z - RT.VIS_Z).abs() < R.TOL
        print('%s rows=%d: %d of %d landmarks within TOL of the threshold, visible share %.2f' % (name, rows, int(near.sum()), near.numel(), float(vis.mean())))
        assert float(near.double().mean(1).max()) <= TC.CAP
    assert 0 < float(RT.visofp(tn, faces, *TC.landmarks(len(faces)))[0].mean()) < 1               # both sides of 0.1 occur on the sheet
    if rows > 1:
        z = p[:, :, 2]
        assert float(z[1].max() - z[1].min()) > 1.2 * float(z[0].max() - z[0].min())             # the rows' z ranges differ


@pytest.mark.parametrize('Su,H,with_albedo,kind', TC.UV, ids=TC.UV_IDS)
def test_uv_inputs_are_well_formed(Su, H, with_albedo, kind):
    """The UV pass is continuous in everything but the table, which it is given: nothing is set aside.  What is checked here is that the
    inputs exercise it: covered and (above 16) uncovered texels, projected vertices inside and outside the image."""
    rows = 2
    verts, faces, cam, uv, uvfaces = TC.sheet(rows)
    albedo, light, uvn, images = TC.maps(rows, Su, H)
    pix, bary, _ = TC.uv_table(uv, uvfaces, Su)
    tv = R.project(verts, cam, 0.0, torch.float32)
    mask = TC.mask_of(kind, Su)
    r64 = RT.uv_textures(albedo if with_albedo else None, uvn, light, tv, images, faces, pix, bary, mask)
    r32 = RT.uv_textures(albedo if with_albedo else None, uvn, light, tv, images, faces, pix, bary, mask, dtype=torch.float32)
    assert ('uv_texture' in r64) == with_albedo
    for k in r64:
        d32 = float((r32[k].double() - r64[k]).abs().max())
        print('uv Su=%d H=%d %-14s d32 %.3e of max %.3e' % (Su, H, k, d32, float(r64[k].abs().max())))
        assert d32 <= 1e-5
    assert int((pix >= 0).sum()) > 0.5 * Su * Su and (Su == 16 or int((pix < 0).sum()) > 0)
    if int((pix < 0).sum()):
        c = H // 2
        centre = images[:, :, c - 1:c + 1, c - 1:c + 1].double().mean((2, 3))
        assert float((r64['uv_gt'][..., pix < 0] - centre[..., None]).abs().max()) <= 1e-12        # an uncovered texel: the image centre

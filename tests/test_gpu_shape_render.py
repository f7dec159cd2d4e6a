"""GPU: the HIP shape renderer (shape_render.py, csrc/shaperender.hip) against the float64 restatement
(tests/shape_render_restatement.py): exact coverage on lattice meshes at the tile, chunk and image edges; general meshes with the
ambiguous pixels set aside under a cap; vertex normals; the options; shape_panels; graph replay; the refused arguments.

Bars.  Lattice cases: pix_to_face equal, no pixel excluded (tests/shape_render_cases.py says why they are exact).  General cases: a
pixel is ambiguous when, in float64, some face has its smallest barycentric within 1e-4 of 0, the two nearest covering faces differ
in z by less than 1e-4, or |Tz - 0.15| < 1e-4 (1e-4 is about 100 x the float32 error of a barycentric); at most 2 % of an image's
pixels may be ambiguous, pix_to_face is equal on all others, and there every value lies within 4 x d32 of the float64 restatement,
d32 being the largest deviation of the restatement run in float32 on the same inputs (the factor covers another summation order and
the device's division and square root).  Normals: the same 4 x d32.
Measured on an MI355X (DESIGN.md 4.26 has the table): ambiguous shares 0 ... 0.34 % of an image; deviations 0.9 ... 1.4 x d32 (the
kernels keep the restatement's order of operations); alpha equal on every pixel compared.
"""
import numpy as np
import pytest
import torch

from util import S as SY, SEED
import shape_render_cases as C
import shape_render_restatement as R
from test_cpu_flame import flame_state
from test_cpu_shape_render import FLAME_ROWS, FLAME_SEED, FLAME_SIZE, SMOOTH_SEED, SMOOTH_SIZE, flame_codedict

pytestmark = pytest.mark.gpu

ALL = ('shape', 'alpha', 'pix_to_face', 'zbuf', 'bary')
VALUES = ('shape', 'alpha', 'zbuf', 'bary')
_CACHE = {}


def _sr():
    from stylegan_directions_face_reenactment_amd import shape_render
    return shape_render


def _topo(faces, n_vertices):
    return _sr().MeshTopology(faces, n_vertices)


def _flame():
    from stylegan_directions_face_reenactment_amd.flame import FLAME
    if 'flame' not in _CACHE:
        m = FLAME()
        m.load_state_dict(flame_state(FLAME_SEED))
        _CACHE['flame'] = m.cuda()
    return _CACHE['flame']


def _code(rows=None):
    c = {k: v.cuda() for k, v in flame_codedict().items()}
    return c if rows is None else {k: v[:rows] for k, v in c.items()}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _same_dict(a, b):
    return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------------------ exact coverage
@pytest.mark.parametrize('name', sorted(C.LATTICE))
def test_lattice_coverage_is_exact(name):
    verts, faces = C.LATTICE[name]
    topo = _topo(faces, verts.shape[0])
    for size in C.SIZES:                                                    # 24 and 40 leave partial tiles
        want = R.rasterize(verts[None], faces, size)[0]
        pix, zbuf, bary = _sr().rasterize(verts.float()[None].cuda(), topo, size)
        assert pix.dtype == torch.int32 and torch.equal(pix.cpu().long(), want), (name, size)
        none = (pix < 0).cpu()
        assert bool((zbuf.cpu()[none] == -1).all()) and bool((bary.cpu()[none] == -1).all())
        assert bool((zbuf.cpu()[~none] >= 0).all()) and bool((bary.cpu()[~none] > 0).all())


def test_lattice_grid_across_two_chunk_edges():
    verts, faces = C.lattice_grid()
    topo = _topo(faces, verts.shape[0])
    for size in C.SIZES:
        want = R.rasterize(verts[None], faces, size)[0]
        pix = _sr().rasterize(verts.float()[None].cuda(), topo, size)[0].cpu().long()
        assert torch.equal(pix, want), size
    for f in (255, 256, 512):                                               # size 40: the last face of chunk 0, the first of chunk 1, chunk 2
        assert int((want == f).sum()) > 0 and torch.equal(pix == f, want == f)


def test_rows_do_not_depend_on_the_batch():
    verts, faces, cam = C.smooth_grid(SMOOTH_SEED + 1, rows=3)
    topo = _topo(faces, verts.shape[1])
    v, c = verts.cuda(), cam.cuda()
    whole = _sr().render_shape(v, topo, cam=c, size=SMOOTH_SIZE, want=ALL)
    assert len({float(x) for x in cam[:, 0]}) == 3
    for b in range(3):
        one = _sr().render_shape(v[b:b + 1], topo, cam=c[b:b + 1], size=SMOOTH_SIZE, want=ALL)
        for k in ALL:
            assert _same(whole[k][b:b + 1], one[k]), (b, k)
    assert not torch.equal(whole['pix_to_face'][0], whole['pix_to_face'][1])


# ------------------------------------------------------------------------------------------------------------------ general meshes
def _compare(label, got, verts, faces, size, **kw):
    """got: render_shape's dict for inputs verts / kw (CPU float32 tensors).  Prints and returns the figures it asserts."""
    r64 = R.render(verts, faces, size, dtype=torch.float64, **kw)
    r32 = R.render(verts, faces, size, dtype=torch.float32, **kw)
    amb = r64['ambiguous']
    share = amb.reshape(amb.shape[0], -1).double().mean(1)
    print('%s: ambiguous share per image %s' % (label, ['%.4f' % s for s in share.tolist()]))
    assert float(share.max()) <= 0.02, share
    clear = ~amb
    pix = got['pix_to_face'].cpu().long()
    assert torch.equal(pix[clear], r64['pix_to_face'][clear]), int((pix != r64['pix_to_face'])[clear].sum())
    fair = clear & (r32['pix_to_face'] == r64['pix_to_face'])               # d32 is taken where float32 itself picks the same face
    figures = {}
    for k in VALUES:
        sel = {'shape': lambda m: m[:, None].expand(-1, 3, -1, -1), 'alpha': lambda m: m[:, None], 'zbuf': lambda m: m,
               'bary': lambda m: m[..., None].expand(-1, -1, -1, 3)}[k]
        d32 = float((r32[k].double() - r64[k])[sel(fair)].abs().max())
        dev = float((got[k].cpu().double() - r64[k])[sel(clear)].abs().max())
        figures[k] = (dev, d32)
        print('%s: %-5s hip deviation %.3e   d32 %.3e   bar %.3e' % (label, k, dev, d32, 4 * d32))
    for k, (dev, d32) in figures.items():
        assert dev <= 4 * d32, (label, k, dev, d32)
    return figures


def test_smooth_grid_matches_the_restatement():
    verts, faces, cam = C.smooth_grid(SMOOTH_SEED)
    got = _sr().render_shape(verts.cuda(), _topo(faces, verts.shape[1]), cam=cam.cuda(), size=SMOOTH_SIZE, want=ALL)
    _compare('smooth grid', got, verts, faces, SMOOTH_SIZE, cam=cam)
    covered = got['pix_to_face'] >= 0
    assert float(got['alpha'].mean()) > 0.2 and int((got['alpha'][:, 0][covered] == 0).sum()) > 20        # back-facing cells


def test_flame_shape_images_match_the_restatement():
    from stylegan_directions_face_reenactment_amd import flame as FL
    m, code = _flame(), _code()
    with torch.no_grad():
        verts = m(code['alpha_shp'], code['alpha_exp'], code['pose'])[0].contiguous()
    got = _sr().render_shape(verts, FL.topology(m), cam=code['cam'], size=FLAME_SIZE, want=ALL)
    images = FL.shape_images(m, code, size=FLAME_SIZE)
    assert tuple(images.shape) == (FLAME_ROWS, 3, FLAME_SIZE, FLAME_SIZE) and _same(images, got['shape'])
    assert _same(FL.shape_images(m, {'shape': code['alpha_shp'], 'exp': code['alpha_exp'], 'pose': code['pose'], 'cam': code['cam']},
                                 size=FLAME_SIZE), images)             # DECA's own key names
    # the restatement takes the vertices the device decoded: the renderer is compared, not FLAME (tests/test_gpu_flame.py does that)
    _compare('synthetic FLAME', got, verts.cpu(), m.faces_tensor.cpu(), FLAME_SIZE, cam=code['cam'].cpu())
    covered = (got['pix_to_face'] >= 0).reshape(FLAME_ROWS, -1).sum(1)
    assert int(covered.min()) > 50 and float(images.max()) > 0.1


# ------------------------------------------------------------------------------------------------------------------ normals
def test_vertex_normals_with_a_fan_and_an_unreferenced_vertex():
    verts, faces = C.fan(300)
    topo = _topo(faces, verts.shape[1])
    assert int(topo.offsets[1] - topo.offsets[0]) == 300
    got = _sr().vertex_normals(verts.cuda(), topo).cpu()
    n64, n32 = R.vertex_normals(verts, faces), R.vertex_normals(verts, faces, torch.float32)
    d32, dev = float((n32.double() - n64).abs().max()), float((got.double() - n64).abs().max())
    print('fan normals: hip deviation %.3e   d32 %.3e   bar %.3e' % (dev, d32, 4 * d32))
    assert dev <= 4 * d32
    assert bool((got[:, -1] == 0).all()) and float(n64[:, 0].norm(dim=-1).min()) > 0.999
    m = _flame()
    from stylegan_directions_face_reenactment_amd import flame as FL
    v = SY.counter_tensor(SEED, 'shape_render.normals', (2, FL.V, 3), 0.0, 0.08)
    got = _sr().vertex_normals(v.cuda(), FL.topology(m)).cpu()
    n64, n32 = R.vertex_normals(v, m.faces_tensor.cpu()), R.vertex_normals(v, m.faces_tensor.cpu(), torch.float32)
    d32, dev = float((n32.double() - n64).abs().max()), float((got.double() - n64).abs().max())
    print('FLAME-sized normals: hip deviation %.3e   d32 %.3e   bar %.3e' % (dev, d32, 4 * d32))
    assert dev <= 4 * d32


# ------------------------------------------------------------------------------------------------------------------ options
def _smooth_inputs(rows=2):
    verts, faces, cam = C.smooth_grid(SMOOTH_SEED + 2, rows=rows)
    return verts.cuda(), _topo(faces, verts.shape[1]), cam.cuda(), verts, faces, cam


def test_two_calls_are_bit_identical():
    from stylegan_directions_face_reenactment_amd import flame as FL
    m, code = _flame(), _code()
    a = FL.shape_images(m, code, size=FLAME_SIZE)
    assert _same(FL.shape_images(m, code, size=FLAME_SIZE), a)
    v, topo, cam = _smooth_inputs()[:3]
    assert _same_dict(_sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, want=ALL), _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, want=ALL))


def test_projected_vertices_background_and_gan_range():
    v, topo, cam, verts, faces, cam_cpu = _smooth_inputs()
    plain = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, want=('shape', 'alpha'))
    assert list(plain) == ['shape', 'alpha'] and tuple(plain['alpha'].shape) == (2, 1, SMOOTH_SIZE, SMOOTH_SIZE)
    alpha = plain['alpha']
    assert set(alpha.unique().tolist()) == {0.0, 1.0} and float(plain['shape'].max()) > 0.5
    # projected = what the cam path computes, without the z offset; the caller's tensor is left alone
    s, tx, ty = cam[:, None, 0], cam[:, None, 1], cam[:, None, 2]
    proj = torch.stack([s * (v[..., 0] + tx), -(s * (v[..., 1] + ty)), -(s * v[..., 2])], -1).contiguous()
    keep = proj.clone()
    assert _same_dict(_sr().render_shape(v, topo, projected=proj, size=SMOOTH_SIZE, want=('shape', 'alpha')), plain) and torch.equal(proj, keep)
    images = SY.counter_tensor(SEED, 'shape_render.bg', (2, 3, SMOOTH_SIZE, SMOOTH_SIZE), 0.0, 0.5).cuda()
    over = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, images=images, want=('shape', 'alpha'))
    assert _same(over['alpha'], alpha)
    assert _same(over['shape'], plain['shape'] + images * (1 - alpha))      # shaded alpha + images (1 - alpha), in that order
    assert bool((over['shape'] == images)[(alpha == 0).expand(-1, 3, -1, -1)].all())
    gan = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, images=images, gan_range=True)['shape']
    assert _same(gan, over['shape'].clamp(0, 1) * 2 - 1)
    assert float(gan.min()) >= -1.0 and float(gan.max()) <= 1.0


@pytest.mark.parametrize('n_lights,light_rows', [(1, 1), (8, 1), (3, 2)])
def test_lights(n_lights, light_rows):
    v, topo, cam, verts, faces, cam_cpu = _smooth_inputs()
    lights = SY.counter_tensor(SEED, 'shape_render.lights.%d.%d' % (n_lights, light_rows), (light_rows, n_lights, 6), 0.0, 1.0)
    lights[..., 3:] = lights[..., 3:].abs() + 0.5
    got = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, lights=lights.cuda(), want=ALL)
    _compare('lights %d x %d' % (light_rows, n_lights), got, verts, faces, SMOOTH_SIZE, cam=cam_cpu, lights=lights)
    default = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE)['shape']
    explicit = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, lights=torch.tensor(R.DEFAULT_LIGHTS).cuda()[None])['shape']
    assert _same(default, explicit) and not torch.equal(default, got['shape'])


# ------------------------------------------------------------------------------------------------------------------ shape_panels
def test_shape_panels():
    from stylegan_directions_face_reenactment_amd import flame as FL
    from stylegan_directions_face_reenactment_amd.reenact import images_to_uint8, shape_panels, video_frames_px
    m, P = _flame(), 64
    c = SY.synthetic_flame_coeffs(SEED, 'shape_render.panels', 5, [0.2, -0.1, 0.0, 0.4, -0.3])
    c['cam'][:, 0] = 1.0
    params = {'alpha_shp': c['shape'].cuda(), 'alpha_exp': c['exp'].cuda(), 'pose': c['pose'].cuda(), 'cam': c['cam'].cuda()}
    ok = torch.tensor([True, False, True, True, False]).cuda()
    whole = shape_panels(m, params, size=P, batch=8)
    assert tuple(whole.shape) == (5, 3, P, P) and whole.dtype == torch.float32
    assert float(whole.min()) >= -1.0 and float(whole.max()) <= 1.0 and float(whole.max()) > -1.0
    assert _same(whole, FL.shape_images(m, params, size=P, gan_range=True))
    assert _same(shape_panels(m, params, size=P, batch=2), whole)           # chunks of 2, 2, 1 against one chunk
    masked = shape_panels(m, params, ok, size=P, batch=2)
    assert bool((masked[~ok] == 0.0).all()) and _same(masked[ok], whole[ok])
    x = SY.counter_tensor(SEED, 'shape_render.x', (5, 3, P, P), 0.0, 0.5).cuda()
    crops = (SY.counter_tensor(SEED, 'shape_render.crops', (5, P, P, 3), 0.0, 1.0).abs() * 120).clamp(0, 255).to(torch.uint8).cuda()
    video = video_frames_px(x, [crops, masked])
    assert tuple(video.shape) == (5, P, 3 * P, 3)
    assert torch.equal(video[:, :, P:2 * P], images_to_uint8(masked))
    assert torch.equal(video[:, :, 2 * P:], images_to_uint8(x))


# ------------------------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_equals_the_eager_call():
    v, topo, cam = _smooth_inputs()[:3]
    images = torch.zeros(2, 3, SMOOTH_SIZE, SMOOTH_SIZE, device='cuda')
    eager = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, images=images, want=ALL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _sr().render_shape(v, topo, cam=cam, size=SMOOTH_SIZE, images=images, want=ALL)
    for k in held:
        held[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_dict(held, eager)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refused_arguments():
    v, topo, cam, verts, faces, cam_cpu = _smooth_inputs()
    render = _sr().render_shape
    with pytest.raises(RuntimeError, match='no CPU path'):
        render(verts, topo, cam=cam)
    with pytest.raises(RuntimeError, match='no CPU path'):
        render(v, topo, cam=cam_cpu)
    with pytest.raises(RuntimeError, match='exactly one of cam and projected'):
        render(v, topo, cam=cam, projected=v)
    with pytest.raises(RuntimeError, match='exactly one of cam and projected'):
        render(v, topo)
    with pytest.raises(RuntimeError, match='int32 or int64'):
        _sr().MeshTopology(faces.float(), verts.shape[1])
    with pytest.raises(RuntimeError, match=r'lights of shape \[1 or 2, 1..8, 6\]'):
        render(v, topo, cam=cam, lights=torch.ones(1, 9, 6).cuda())
    with pytest.raises(RuntimeError, match=r'\[2,169,3\]'):
        render(v, topo, projected=v[:, :-1])
    with pytest.raises(RuntimeError, match=r'images of shape \[2,3,40,40\]'):
        render(v, topo, cam=cam, size=SMOOTH_SIZE, images=torch.zeros(2, 3, 41, 40).cuda())
    with pytest.raises(RuntimeError, match='size must be an int'):
        render(v, topo, cam=cam, size=0)
    with pytest.raises(RuntimeError, match='expected float32'):
        render(v.double(), topo, cam=cam)

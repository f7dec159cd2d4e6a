"""CPU: the host side of the shape renderer (shape_render.MeshTopology, the C ABI of csrc/shaperender.hip, the argument checks) and
the restatement the GPU tests compare with (tests/shape_render_restatement.py): a hand-computed triangle, the reference's order of
summation for the vertex normals, the lattice cases in exact rational arithmetic, and the share of ambiguous pixels of the general
cases, which has to stay under 1 % here so that the GPU test's 2 % cap has room."""
import copy
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import shape_render_cases as C
import shape_render_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the general cases of tests/test_gpu_shape_render.py: seeds and camera scale picked here, on the restatement alone
SMOOTH_SEED, SMOOTH_SIZE = 3, 40
FLAME_SEED, FLAME_KEY, FLAME_SIZE, FLAME_ROWS = 11, 'shape_render.flame', 224, 2
# The synthetic FLAME tables draw their 9976 faces as random index triples: a soup in which every vertex pair is as likely as any
# other, so at DECA's camera scale (about 8: the vertices spread over the whole image) every pixel lies under about a thousand faces
# and within 1e-4 of some edge or of a second face at the same depth.  The soup is therefore rendered small: scale FLAME_CAM_SCALE puts
# it into a blob of about 25 pixels across, where the same faces, chunks and depth order are exercised on a share of the image small
# enough for the cap.
FLAME_CAM_SCALE = 0.55


def flame_codedict():
    from stylegan_directions_face_reenactment_amd import synthetic as S
    c = S.synthetic_flame_coeffs(FLAME_SEED, FLAME_KEY, FLAME_ROWS, [0.3, -0.4])
    c['cam'][:, 0] = torch.tensor([FLAME_CAM_SCALE, 0.8 * FLAME_CAM_SCALE])
    c['cam'][:, 1:] *= 10.0                                    # off-centre blobs: different tiles per row
    return {'alpha_shp': c['shape'], 'alpha_exp': c['exp'], 'pose': c['pose'], 'cam': c['cam']}


# ------------------------------------------------------------------------------------------------------------------ topology
def test_csr_counts_order_and_validation():
    from stylegan_directions_face_reenactment_amd.shape_render import MeshTopology
    g = torch.Generator().manual_seed(5)
    V, F = 37, 90
    faces = torch.randint(0, V - 1, (F, 3), generator=g)                    # vertex V-1 stays unreferenced
    for f in (faces, faces.to(torch.int32)):
        t = MeshTopology(f, V)
        assert t.faces.dtype == t.offsets.dtype == t.entries.dtype == torch.int32
        assert (t.n_vertices, t.n_faces) == (V, F) and tuple(t.offsets.shape) == (V + 1,) and tuple(t.entries.shape) == (3 * F,)
        counts = np.bincount(faces.reshape(-1).numpy(), minlength=V)
        assert np.array_equal(np.diff(t.offsets.numpy()), counts) and counts[V - 1] == 0
        off, ent = R.csr(faces, V)
        assert np.array_equal(t.offsets.numpy(), off) and np.array_equal(t.entries.numpy(), ent)
        for v in range(V):
            e = t.entries[t.offsets[v]:t.offsets[v + 1]].numpy()
            assert np.all(np.diff(e) > 0)                                   # by face, then corner
            assert np.all(faces.reshape(-1).numpy()[e] == v)
    for bad in (faces.clone().index_put_((torch.tensor(3), torch.tensor(1)), torch.tensor(V)),
                faces.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(-1))):
        with pytest.raises(RuntimeError, match='outside 0..36'):
            MeshTopology(bad, V)
    for bad in (faces.reshape(-1), faces[:, :2], faces[None], torch.zeros((0, 3), dtype=torch.long)):
        with pytest.raises(RuntimeError, match=r'\[F,3\]'):
            MeshTopology(bad, V)
    with pytest.raises(RuntimeError, match='int32 or int64'):
        MeshTopology(faces.float(), V)
    with pytest.raises(RuntimeError, match='n_vertices'):
        MeshTopology(faces, 0)


def test_topology_copies_pickles_and_comes_from_flame():
    from stylegan_directions_face_reenactment_amd.shape_render import MeshTopology
    from stylegan_directions_face_reenactment_amd import flame as FL
    verts, faces = C.LATTICE['equal_depth']
    t = MeshTopology(faces, verts.shape[0])
    t.tables('cpu')
    for u in (copy.deepcopy(t), pickle.loads(pickle.dumps(t))):
        assert u._device == {} and torch.equal(u.entries, t.entries) and torch.equal(u.faces, t.faces) and u.n_vertices == t.n_vertices
    m = FL.FLAME()
    m.faces_tensor.copy_(torch.arange(FL.FACES * 3).reshape(FL.FACES, 3) % FL.V)
    topo = FL.topology(m)
    assert (topo.n_vertices, topo.n_faces) == (FL.V, FL.FACES) and FL.topology(m) is topo
    assert torch.equal(MeshTopology.from_flame(m).entries, topo.entries)
    m.faces_tensor[0, 0] = 7                                                # an edit of the buffer rebuilds the table
    assert FL.topology(m) is not topo and int(FL.topology(m).faces[0, 0]) == 7
    pickle.loads(pickle.dumps(m))
    copy.deepcopy(m)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_and_validate_their_arguments():
    from stylegan_directions_face_reenactment_amd import _native as N
    header = open(os.path.join(ROOT, 'include', 'sgdfr.h')).read()
    names = ('sgdfr_shaperender_normals_f32', 'sgdfr_shaperender_forward_f32')
    for name in names:
        assert name in N.SIGNATURES and re.search(r'\b%s\s*\(' % name, header)
    assert N.SIZE_QUERIES['sgdfr_shaperender_workspace_bytes'] == 3 and 'sgdfr_shaperender_workspace_bytes(' in header
    assert len(N.SIGNATURES[names[0]]) == 9 and len(N.SIGNATURES[names[1]]) == 24
    lib = N.load()
    assert lib.sgdfr_abi_version() == N.ABI_VERSION                         # symbols appended, nothing moved
    need = lib.sgdfr_shaperender_workspace_bytes(2, 5023, 9976)
    assert need >= 2 * (5023 * 7 * 4 + 9976 * 56)
    assert lib.sgdfr_shaperender_workspace_bytes(0, 10, 10) == -1 and lib.sgdfr_shaperender_workspace_bytes(1, 0, 10) == -1
    one = 1                                                                 # any non-null pointer: validation comes before every launch

    def forward(**kw):
        a = dict(vertices=one, projected=None, cam=one, rows=1, V=4, F=2, S=16, lights=one, light_rows=1, L=5, shape=one, ws=one,
                 ws_bytes=1 << 30)
        a.update(kw)
        return lib.sgdfr_shaperender_forward_f32(a['vertices'], a['projected'], a['cam'], 10.0, a['rows'], a['V'], one, a['F'], one, one,
                                                 a['S'], a['lights'], a['light_rows'], a['L'], None, 0, a['shape'], None, None, None, None,
                                                 a['ws'], a['ws_bytes'], None)

    for kw, text in ((dict(S=0), b'size=0'), (dict(S=4097), b'size=4097'), (dict(projected=one), b'exactly one'), (dict(cam=None), b'exactly one'),
                     (dict(L=9), b'9 lights'), (dict(L=0), b'0 lights'), (dict(light_rows=2), b'lights for 2 rows'), (dict(rows=0), b'rows=0'),
                     (dict(ws_bytes=16), b'workspace of 16 bytes'), (dict(shape=None), b'no output'), (dict(vertices=None), b'cam needs')):
        assert forward(**kw) != 0 and text in lib.sgdfr_last_error(), (kw, lib.sgdfr_last_error())
    assert lib.sgdfr_shaperender_normals_f32(None, 1, 4, one, 2, one, one, one, None) != 0 and b'null pointer' in lib.sgdfr_last_error()


def test_cpu_tensors_and_bad_arguments_are_refused():
    from stylegan_directions_face_reenactment_amd import shape_render as SR
    from stylegan_directions_face_reenactment_amd.reenact import shape_panels
    verts, faces = C.LATTICE['equal_depth']
    topo = SR.MeshTopology(faces, verts.shape[0])
    v = verts.float()[None]
    for call in (lambda: SR.vertex_normals(v, topo), lambda: SR.rasterize(v, topo, 16), lambda: SR.render_shape(v, topo, projected=v),
                 lambda: shape_panels(None, {k: torch.zeros(2, 3) for k in ('alpha_shp', 'alpha_exp', 'pose', 'cam')})):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()
    with pytest.raises(RuntimeError, match='exactly one of cam and projected'):
        SR.render_shape(v, topo)
    with pytest.raises(RuntimeError, match='exactly one of cam and projected'):
        SR.render_shape(v, topo, cam=torch.zeros(1, 3), projected=v)
    with pytest.raises(RuntimeError, match='MeshTopology'):
        SR.render_shape(v, faces, projected=v)
    with pytest.raises(RuntimeError, match='want'):
        SR.render_shape(v, topo, projected=v, want=('alpha',))
    with pytest.raises(RuntimeError, match='params must be a dict'):
        shape_panels(None, {'pose': torch.zeros(2, 6)})


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_a_hand_computed_triangle():
    """S = 4: centres at -0.75, -0.25, 0.25, 0.75.  The triangle (-1,-1), (0.5,-1), (-1,0.5) holds the centres with x + y < -0.5
    strictly: (-0.75,-0.75), (-0.25,-0.75), (-0.75,-0.25); (0.25,-0.75) and (-0.25,-0.25) and (-0.75,0.25) lie on the hypotenuse."""
    P = torch.tensor([[-1.0, -1.0, 2.0], [0.5, -1.0, 2.0], [-1.0, 0.5, 4.0]])
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        for dtype in (torch.float64, torch.float32):
            pix, zbuf, bary, amb = R.rasterize(P[None], faces, 4, dtype)
            want = torch.full((4, 4), -1, dtype=torch.long)
            want[0, 0] = want[0, 1] = want[1, 0] = 0                        # [row, column]: the top-left pixel is the one nearest (-1, -1)
            assert torch.equal(pix[0], want)
            assert torch.equal(R.centres(4, dtype), torch.tensor([-0.75, -0.25, 0.25, 0.75], dtype=dtype))
            # pixel (row 1, column 0) = (-0.75, -0.25): barycentrics of corners 0, 1, 2 = 1/3, 1/6, 1/2; z = (1/3 + 1/6) 2 + (1/2) 4 = 3
            b = bary[0, 1, 0] if faces == [[0, 1, 2]] else bary[0, 1, 0][[0, 2, 1]]
            assert torch.allclose(b.double(), torch.tensor([1 / 3, 1 / 6, 1 / 2], dtype=torch.float64), atol=1e-6)
            assert abs(float(zbuf[0, 1, 0]) - 3.0) < 1e-5 and float(zbuf[0, 3, 3]) == -1.0
            assert bool(amb[0, 0, 2]) and bool(amb[0, 1, 1]) and bool(amb[0, 2, 0]) and not bool(amb[0, 0, 0])


def test_restated_normals_equal_the_reference_order_of_summation():
    g = torch.Generator().manual_seed(9)
    V, F = 60, 200
    verts = torch.randn(3, V, 3, generator=g, dtype=torch.float64)
    faces = torch.randint(0, V - 2, (F, 3), generator=g)
    a, b = R.vertex_normals(verts, faces), R.reference_order_normals(verts, faces)
    assert float((a - b).abs().max()) < 1e-13
    assert float(a[:, V - 2:].abs().max()) == 0.0                           # unreferenced: exact zeros
    used = a[:, :V - 2].norm(dim=-1)
    assert float((used - 1).abs().max()) < 1e-12
    # one triangle in the xy plane, counter-clockwise: +z at all three corners
    n = R.vertex_normals(torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]]), [[0, 1, 2]])
    assert torch.equal(n, torch.tensor([[[0.0, 0, 1]] * 3], dtype=torch.float64))


def _exact_raster(verts, faces, S):
    """pix_to_face in rational arithmetic, and whether float arithmetic could decide a pixel differently: a rounded centre (S not a
    power of two) exactly on an edge that is neither axis-aligned nor on x = y, or a covering face whose z is within 1e-5 of 0"""
    fr = lambda t: [[Fraction(float(x)) for x in row] for row in t]
    P, eps = fr(verts), Fraction(1e-8)
    pix = np.full((S, S), -1, dtype=np.int64)
    unsafe, rounded = False, S & (S - 1) != 0
    for i in range(S):
        for j in range(S):
            px, py = Fraction(2 * j + 1, S) - 1, Fraction(2 * i + 1, S) - 1
            best = None
            for f, (i0, i1, i2) in enumerate(faces.tolist()):
                a, b, c = P[i0], P[i1], P[i2]
                edge = lambda p, u, v: (p[0] - u[0]) * (v[1] - u[1]) - (p[1] - u[1]) * (v[0] - u[0])
                area = edge(c, a, b)
                if abs(area) <= eps or (a[2] < 0 and b[2] < 0 and c[2] < 0):
                    continue
                for u, v in ((b, c), (c, a), (a, b)):
                    if rounded and edge((px, py), u, v) == 0 and u[0] != v[0] and u[1] != v[1] and not (u[0] == u[1] and v[0] == v[1]):
                        unsafe = True
                w = [edge((px, py), u, v) / (area + eps) for u, v in ((b, c), (c, a), (a, b))]
                z = w[0] * a[2] + w[1] * b[2] + w[2] * c[2]
                if min(w) > 0 and z >= 0:
                    unsafe = unsafe or z < Fraction(1, 100000)
                    if best is None or z < best:
                        best, pix[i, j] = z, f
    return pix, unsafe


@pytest.mark.parametrize('name', sorted(C.LATTICE))
def test_lattice_cases_are_exact_in_every_precision(name):
    verts, faces = C.LATTICE[name]
    for S in C.SIZES:
        exact, unsafe = _exact_raster(verts, faces, S)
        assert not unsafe, S
        for dtype in (torch.float64, torch.float32):
            assert np.array_equal(R.rasterize(verts[None], faces, S, dtype)[0][0].numpy(), exact), (S, dtype)
    owned = set(np.unique(exact).tolist())
    want = {'quad_diagonal': {-1, 0, 1}, 'nearer_wins': {-1, 0, 1, 2, 3}, 'nearer_wins_listed_first': {-1, 0, 1, 2, 3},
            'equal_depth': {-1, 0, 1}, 'reversed_winding': {-1, 0}, 'zero_area': {-1, 1}, 'partly_outside': {-1, 0},
            'wholly_outside': {-1}, 'covers_every_tile': {0}, 'behind': {-1, 1}}[name]
    assert owned == want
    if name == 'quad_diagonal':
        assert exact[20, 20] == -1 and exact[20, 21] == 0 and exact[21, 20] == 1     # S = 40: on, right of and below the diagonal
    if name in ('nearer_wins', 'nearer_wins_listed_first'):
        # S = 40, pixel (row 22, column 18) = (-0.075, 0.125) is in the overlap, below both quads' diagonals: faces 1 and 3
        assert exact[22, 18] == {'nearer_wins': 3, 'nearer_wins_listed_first': 1}[name]


def check_small_pair(name, S):
    """One LATTICE mesh at one of the small sizes: safe by the rule of _exact_raster, and both precisions give the exact faces."""
    verts, faces = C.LATTICE[name]
    exact, unsafe = _exact_raster(verts, faces, S)
    assert not unsafe, (name, S)
    for dtype in (torch.float64, torch.float32):
        assert np.array_equal(R.rasterize(verts[None], faces, S, dtype)[0][0].numpy(), exact), (name, S, dtype)
    return exact


@pytest.mark.parametrize('name,S', C.small_pairs(), ids=['%s_%d' % p for p in C.small_pairs()])
def test_lattice_cases_are_exact_at_the_small_sizes(name, S):
    exact = check_small_pair(name, S)
    if S == 1:                                                              # the one centre is the origin
        inside = {'covers_every_tile': 0, 'partly_outside': 0, 'reversed_winding': 0}
        assert exact.shape == (1, 1) and int(exact[0, 0]) == inside.get(name, -1)
    if name == 'quad_diagonal' and S == 17:
        assert exact[8, 8] == -1 and exact[8, 9] == 0 and exact[9, 8] == 1  # on, right of and below the diagonal


def test_the_dropped_small_pairings_cannot_be_proven():
    """What SMALL_DROPPED leaves out is exactly what the rule calls unsafe: nothing is dropped for convenience."""
    unsafe = {(name, S) for name in sorted(C.LATTICE) for S in C.SMALL_SIZES if _exact_raster(*C.LATTICE[name], S)[1]}
    assert unsafe == set(C.SMALL_DROPPED)


def test_lattice_grid_crosses_two_chunks_and_float32_agrees():
    verts, faces = C.lattice_grid()
    assert tuple(faces.shape) == (513, 3)
    for S in C.SIZES:
        p64, p32 = (R.rasterize(verts[None], faces, S, d)[0][0] for d in (torch.float64, torch.float32))
        assert torch.equal(p64, p32)
    for f in (255, 256, 512):
        assert int((p64 == f).sum()) > 0                                    # S = 40
    assert all(int(p64[i, i]) == 512 for i in range(40))                    # the cells' shared diagonals on x = y fall through


def _share(amb):
    return amb.reshape(amb.shape[0], -1).double().mean(1)


def test_general_cases_stay_under_one_percent_ambiguous():
    verts, faces, cam = C.smooth_grid(SMOOTH_SEED)
    r = R.render(verts, faces, SMOOTH_SIZE, cam=cam)
    share = _share(r['ambiguous'])
    print('smooth grid: ambiguous share %s, covered %.3f' % (share.tolist(), float((r['pix_to_face'] >= 0).double().mean())))
    assert float(share.max()) < 0.01 and float((r['pix_to_face'] >= 0).double().mean()) > 0.4
    covered = r['pix_to_face'] >= 0
    assert int((r['alpha'][:, 0][covered] == 0).sum()) > 20 and float(r['shape'].max()) > 0.3        # back-facing cells under coverage


@pytest.fixture(scope='module')
def flame_case():
    import flame_restatement as FR
    from test_cpu_flame import flame_state
    state = flame_state(FLAME_SEED)
    code = flame_codedict()
    T = FR.tables(state)
    c = {'shape': code['alpha_shp'].double(), 'exp': code['alpha_exp'].double(), 'pose': code['pose'].double(), 'cam': code['cam'].double()}
    verts = FR.decode(T, c)[3]['vertices']
    return verts, state['faces_tensor'], code['cam']


def test_flame_case_stays_under_one_percent_ambiguous(flame_case):
    verts, faces, cam = flame_case
    r = R.render(verts, faces, FLAME_SIZE, cam=cam)
    share = _share(r['ambiguous'])
    covered = (r['pix_to_face'] >= 0).reshape(FLAME_ROWS, -1).sum(1)
    print('synthetic FLAME: ambiguous share %s, covered pixels %s' % (share.tolist(), covered.tolist()))
    assert float(share.max()) < 0.01 and int(covered.min()) > 50

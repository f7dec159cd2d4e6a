"""Meshes for the shape renderer's tests (tests/test_cpu_shape_render.py, tests/test_gpu_shape_render.py).

LATTICE: small meshes whose x, y are multiples of 1/64.  At S = 16 every pixel centre is a multiple of 1/16 and every edge function
is exact in float32.  At S = 24 and 40 a centre (2j+1)/S - 1 is rounded, but an edge function that is not zero in exact arithmetic is
at least 1/(64 * 64 * 40) = 6e-6 away from zero, far beyond the rounding; and the edges that do pass through centres here do so where
float arithmetic is exact too: axis-aligned edges (a centre equal to k/64 is a dyadic number, so it is computed exactly) and the line
x = y (pixel (i, i) has the same x and y in any precision).  tests/test_cpu_shape_render.py proves the small cases with exact
rationals.  Faces are given as (projected vertices [V,3], faces [F,3]); z is the depth the rasteriser sees (no offset).
"""
import numpy as np
import torch

SIZES = (16, 24, 40)
# One pixel (its centre is the origin), half a tile, and a tile plus one row and column of pixels.  At 1 and 8 every centre is dyadic;
# at 17 the argument above for 24 and 40 holds with 1/(64 * 64 * 17).  tests/test_cpu_shape_render.py proves each pairing with exact
# rationals; the two it cannot prove are left out (no tolerance is added for them): at 17 a rounded centre lies exactly on the line
# through an edge of `behind` and of `wholly_outside` that is neither axis-aligned nor x = y.
SMALL_SIZES = (1, 8, 17)
SMALL_DROPPED = (('behind', 17), ('wholly_outside', 17))


def small_pairs():
    """(name, size) of every LATTICE mesh at every SMALL_SIZES size that is proven exact"""
    return [(name, size) for name in sorted(LATTICE) for size in SMALL_SIZES if (name, size) not in SMALL_DROPPED]


def _mesh(verts, faces):
    return torch.tensor(verts, dtype=torch.float64), torch.tensor(faces, dtype=torch.int64)


def _square(lo, hi, z):
    return [[lo, lo, z], [hi, lo, z], [hi, hi, z], [lo, hi, z]]


def quad_diagonal():
    """two faces that share the diagonal x = y: the centres on it belong to neither"""
    return _mesh(_square(-0.5, 0.5, 1.0), [[0, 1, 2], [0, 2, 3]])


def stacked_quads(z_far, z_near):
    """faces 0, 1 at z_far, faces 2, 3 at z_near, overlapping in [-0.25, 0.25]^2"""
    return _mesh(_square(-0.75, 0.25, z_far) + _square(-0.25, 0.75, z_near), [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])


def coincident_quads():
    """faces 2, 3 repeat faces 0, 1 on vertices of their own with the same coordinates: every pixel computes the same z for both in any
    precision, so only the tie rule decides.  (Two quads that merely overlap at one depth do not tie in floating point: z is a sum of
    three rounded quotients, and the quotients differ between the quads.)"""
    return _mesh(_square(-0.5, 0.5, 1.0) * 2, [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])


def reversed_winding():
    return _mesh([[-0.5, -0.625, 1.0], [0.75, -0.25, 1.0], [-0.125, 0.6875, 1.0]], [[0, 2, 1]])


def zero_area():
    """face 0 has three collinear corners; face 1 is there to show that the image is not simply empty"""
    return _mesh([[-0.5, -0.5, 1.0], [0.0, 0.0, 1.0], [0.5, 0.5, 1.0], [-0.75, 0.25, 1.0], [-0.25, 0.25, 1.0], [-0.5, 0.875, 1.0]],
                 [[0, 1, 2], [3, 4, 5]])


def partly_outside():
    return _mesh([[-1.5, -0.5, 1.0], [0.5, -15 / 64.0, 1.0], [-17 / 64.0, 1.5, 1.0]], [[0, 1, 2]])


def wholly_outside():
    return _mesh([[1.25, -0.5, 1.0], [2.0, 0.0, 1.0], [1.5, 0.75, 1.0], [-0.5, -1.75, 1.0], [0.5, -1.75, 1.0], [0.0, -1.125, 1.0]],
                 [[0, 1, 2], [3, 4, 5]])


def covers_every_tile():
    return _mesh([[-4.0, -4.0, 1.0], [4.0, -4.0, 1.0], [0.0, 4.0, 1.0]], [[0, 1, 2]])


def behind():
    """face 0 has every corner at Z < 0 and is skipped; face 1 straddles Z = 0: it renders where the interpolated z is >= 0"""
    return _mesh([[-0.5, -0.5, -1.0], [0.5, -0.5, -2.0], [0.0, 0.5, -0.5], [-0.75, -0.75, -1.0], [0.75, -0.75, 3.0], [0.75, 0.75, 1.0]],
                 [[0, 1, 2], [3, 4, 5]])


LATTICE = {
    'quad_diagonal': quad_diagonal(), 'nearer_wins': stacked_quads(2.0, 1.0), 'nearer_wins_listed_first': stacked_quads(1.0, 2.0),
    'equal_depth': coincident_quads(), 'reversed_winding': reversed_winding(), 'zero_area': zero_area(),
    'partly_outside': partly_outside(), 'wholly_outside': wholly_outside(), 'covers_every_tile': covers_every_tile(), 'behind': behind(),
}


def grid_faces(n):
    """(n-1)^2 cells of an n x n vertex grid, two faces each, split along the diagonal from vertex (m, r) to (m+1, r+1)"""
    faces = []
    for r in range(n - 1):
        for m in range(n - 1):
            v = r * n + m
            faces += [[v, v + 1, v + n + 1], [v, v + n + 1, v + n]]
    return faces


def lattice_grid():
    """17 x 17 vertices spaced 7/64 from -56/64 (512 faces, depth 1 ... 1.32) and one triangle behind everything as face 512: F = 513
    crosses two chunks of 256.  The cell diagonals are x - y = 7 (m - r) / 64; a centre lies on one only for m = r (the line x = y),
    so those pixels fall through to face 512."""
    n = 17
    verts = [[(-56 + 7 * m) / 64.0, (-56 + 7 * r) / 64.0, 1.0 + 0.01 * (m + r)] for r in range(n) for m in range(n)]
    verts += [[-4.0, -4.0, 5.0], [4.0, -4.0, 5.0], [0.0, 4.0, 5.0]]
    return _mesh(verts, grid_faces(n) + [[n * n, n * n + 1, n * n + 2]])


def smooth_grid(seed, n=13, rows=1):
    """World vertices of a smoothly bent n x n sheet, off every lattice, and a camera per row: (vertices [rows,V,3], faces, cam
    [rows,3]), float32-representable.  The 4 x 4 cells of one corner are wound the other way: they face backwards (alpha 0 under
    coverage), and across their border the interpolated normal passes through the 0.15 threshold."""
    rng = np.random.RandomState(seed)
    u, v = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    out, cams = [], []
    for _ in range(rows):
        ph = rng.uniform(0, 2 * np.pi, 6)
        x = 0.8 * u + 0.07 * np.sin(2.3 * v + ph[0]) + 0.05 * np.sin(3.1 * u + ph[1])
        y = 0.8 * v + 0.07 * np.sin(2.7 * u + ph[2]) + 0.05 * np.sin(1.9 * v + ph[3])
        z = 0.3 * np.cos(1.5 * u + ph[4]) * np.cos(1.2 * v + ph[5]) - 0.25 * (u * u + v * v)
        out.append(np.stack([x, y, z], -1).reshape(-1, 3))
        cams.append([rng.uniform(0.85, 1.15), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
    verts = torch.tensor(np.array(out), dtype=torch.float32)
    faces = torch.tensor(grid_faces(n), dtype=torch.int64)
    cell = torch.arange(len(faces)) // 2
    back = (cell // (n - 1) < 4) & (cell % (n - 1) < 4)
    faces[back] = faces[back][:, [0, 2, 1]]
    return verts, faces, torch.tensor(cams, dtype=torch.float32)


def fan(valence=300):
    """A closed fan around vertex 0 (valence `valence`), an unreferenced vertex at the end, float32: (vertices [2,V,3], faces)."""
    k = np.arange(valence)
    ang = 2 * np.pi * k / valence
    ring = np.stack([np.cos(ang) * (1 + 0.1 * np.sin(5 * ang)), np.sin(ang), 0.2 * np.cos(3 * ang)], -1)
    v0 = np.concatenate([[[0.05, -0.02, 0.6]], ring, [[9.0, 9.0, 9.0]]], 0)
    v1 = v0 * np.array([1.3, 0.7, -1.1]) + 0.01
    faces = [[0, 1 + i, 1 + (i + 1) % valence] for i in range(valence)]
    return torch.tensor(np.stack([v0, v1]), dtype=torch.float32), torch.tensor(faces, dtype=torch.int64)

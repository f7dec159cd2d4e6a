"""DECA's shape renderer on the HIP kernels of csrc/shaperender.hip: the grey, lit mesh image DECA.decode_deca returns as
`shape_images` (libs/DECA/decalib/utils/renderer.py:237-293 SRenderY.render_shape, with utils/util.py vertex_normals and pytorch3d's
rasterize_meshes at the fixed settings of renderer.py:40-47).  Forward only: the reference detaches everything the picture depends on.

    topo = MeshTopology.from_flame(F)                                   # or MeshTopology(faces [F,3], n_vertices): any mesh
    out = render_shape(vertices, topo, cam=cam, size=224)               # {'shape': [B,3,224,224]} in the reference's value range
    out = render_shape(vertices, topo, projected=trans_verts, images=x, want=('shape', 'alpha', 'pix_to_face'))
    normals = vertex_normals(vertices, topo)                            # util.vertex_normals
    pix_to_face, zbuf, bary = rasterize(projected, topo, 256)           # rasterize_meshes: one face per pixel, blur_radius 0

    ops = render_texture(vertices, topo, layout, albedo, lights=sh, cam=cam, want=('images', 'grid', 'normals'))      # SRenderY.forward
    normal_images = render_normal(projected, normals, topo, 224)        # SRenderY.render_normal, render_depth likewise

Five launches (project, normals of the world and of the projected vertices, face setup, raster + shade), no atomics and a fixed face
order: results are bit-identical from call to call; no host synchronisation, so a call captures into a graph.  The rasteriser's rules
are restated from pytorch3d's documented behaviour (include/sgdfr.h); on equal depth the lower face index wins.
"""
import numpy as np
import torch

from . import _native as N

# renderer.py:244-254: five directional lights at intensity 1.7
DEFAULT_LIGHTS = tuple((x, y, z, 1.7, 1.7, 1.7) for x, y, z in ((-1, 1, 1), (1, 1, 1), (-1, -1, 1), (1, -1, 1), (0, 0, 1)))
Z_OFFSET = 10.0                                     # renderer.py:255
_WANT = ('shape', 'alpha', 'pix_to_face', 'zbuf', 'bary')
_WANT_DETAIL = ('shape_detail', 'grid', 'detail_normal_images')      # with layout and detail_normals only
_WANT_TEXTURE = ('images', 'albedo_images', 'alpha_images', 'pos_mask', 'shading_images', 'grid', 'normal_images', 'normals',
                 'transformed_normals', 'pix_to_face', 'zbuf', 'bary')      # render_texture
# renderer.py:114-119, evaluated in double and rounded to float once
_PI = np.pi
SH_CONSTANTS = tuple(float(np.float32(c)) for c in (
    [1 / np.sqrt(4 * _PI)] + [((2 * _PI) / 3) * np.sqrt(3 / (4 * _PI))] * 3 + [(_PI / 4) * 3 * np.sqrt(5 / (12 * _PI))] * 3
    + [(_PI / 4) * (3 / 2) * np.sqrt(5 / (12 * _PI)), (_PI / 4) * (1 / 2) * np.sqrt(5 / (4 * _PI))]))


class MeshTopology:
    """The faces of a triangle mesh, [F,3] integer indices into n_vertices vertices, with the vertex -> (face, corner) table the
    normals gather over: offsets [V+1], entries [3F] = face * 3 + corner, ascending per vertex.  Validated and built once on the
    host; the int32 tables are moved to a device on first use and kept per device.  Plain tensors only (no library handle), so it
    deep-copies and pickles; the device copies are dropped on pickling."""

    def __init__(self, faces, n_vertices):
        if isinstance(n_vertices, bool) or not isinstance(n_vertices, int) or n_vertices < 1:
            raise RuntimeError('MeshTopology: n_vertices must be a positive int, got %r' % (n_vertices,))
        if not torch.is_tensor(faces) or faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise RuntimeError('MeshTopology: expected faces of shape [F,3], got %s'
                               % (tuple(faces.shape) if torch.is_tensor(faces) else type(faces),))
        if faces.dtype not in (torch.int32, torch.int64):
            raise RuntimeError('MeshTopology: faces must be int32 or int64, got %s' % faces.dtype)
        f = faces.detach().cpu().to(torch.int64).contiguous()
        if int(f.min()) < 0 or int(f.max()) >= n_vertices:
            raise RuntimeError('MeshTopology: faces hold vertex indices outside 0..%d' % (n_vertices - 1))
        flat = f.reshape(-1).numpy()
        order = np.argsort(flat, kind='stable')                 # flat position = face * 3 + corner: stable keeps that order per vertex
        offsets = np.zeros(n_vertices + 1, dtype=np.int64)
        np.cumsum(np.bincount(flat, minlength=n_vertices), out=offsets[1:])
        self.n_vertices, self.n_faces = n_vertices, int(f.shape[0])
        self.faces = f.to(torch.int32)
        self.offsets = torch.from_numpy(offsets.astype(np.int32))
        self.entries = torch.from_numpy(order.astype(np.int32))
        self._device = {}

    @classmethod
    def from_flame(cls, flame):
        """The topology of a flame.FLAME module (its faces_tensor buffer)."""
        return cls(flame.faces_tensor, int(flame.v_template.shape[0]))

    def tables(self, device):
        """(faces, offsets, entries) as int32 tensors on `device`."""
        key = str(device)
        if key not in self._device:
            self._device[key] = tuple(t.to(device).contiguous() for t in (self.faces, self.offsets, self.entries))
        return self._device[key]

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_device'] = {}
        return state

    def __deepcopy__(self, memo):
        new = MeshTopology.__new__(MeshTopology)
        new.__dict__.update(self.__getstate__())        # the host tables are never written: shared
        return new


def _check_topology(who, topo):
    if not isinstance(topo, MeshTopology):
        raise RuntimeError('%s: topo must be a MeshTopology, got %s' % (who, type(topo)))


def _check_map(who, name, t, shape, text=None):
    """The one tensor check: t must be a tensor on a GPU whose shape fits `shape` -- per dimension an int, None (any size >= 1) or a
    container of the sizes allowed -> t detached, float32, contiguous.  `text` words the expectation where the plain list does not."""
    if not torch.is_tensor(t):
        raise RuntimeError('%s: %s must be a tensor, got %s' % (who, name, type(t)))
    N.require_device(t)
    fits = lambda n, s: n >= 1 if s is None else n == s if isinstance(s, int) else n in s
    if t.ndim != len(shape) or not all(fits(n, s) for n, s in zip(t.shape, shape)):
        raise RuntimeError('%s: expected %s, got %s' % (who, text or '%s of shape [%s]' % (name, ','.join(map(str, shape))), tuple(t.shape)))
    return N.f32c(t.detach())


def _check_vertices(who, name, t, n_vertices, rows=None):
    return _check_map(who, name, t, (rows, n_vertices, 3), '%s of shape [%s,%d,3]' % (name, 'B' if rows is None else rows, n_vertices))


def _check_size(who, size):
    if isinstance(size, bool) or not isinstance(size, int) or not 1 <= size <= N.SHAPERENDER_MAX_SIZE:
        raise RuntimeError('%s: size must be an int in 1..%d, got %r' % (who, N.SHAPERENDER_MAX_SIZE, size))


def _prepare(who, vertices, topo, cam, projected, size):
    """What the renderers check first: the topology, exactly one of cam / projected beside world vertices (vertices None: projected
    alone), the size, one device -> (vertices, cam, projected) checked as _check_map returns them, the batch and the device."""
    _check_topology(who, topo)
    if vertices is not None and (cam is None) == (projected is None):
        raise RuntimeError('%s: exactly one of cam and projected must be given' % who)
    if vertices is None:
        v, projected = None, _check_vertices(who, 'projected', projected, topo.n_vertices)
    else:
        v = _check_vertices(who, 'vertices', vertices, topo.n_vertices)
    _check_size(who, size)
    lead = projected if v is None else v
    if cam is not None:
        cam = _check_map(who, 'cam', cam, (lead.shape[0], 3))
    elif v is not None:
        projected = _check_vertices(who, 'projected', projected, topo.n_vertices, lead.shape[0])
    _check_device(who, lead.device, cam, projected)
    return v, cam, projected, lead.shape[0], lead.device


def _check_device(who, device, *tensors):
    if any(t is not None and t.device != device for t in tensors):
        raise RuntimeError('%s: all tensors must live on the vertices\' device %s' % (who, device))


def _check_mesh_layout(who, layout, topo):
    from .detail import UvLayout
    if not isinstance(layout, UvLayout):
        raise RuntimeError('%s: layout must be a detail.UvLayout, got %s' % (who, type(layout)))
    if layout.n_faces != topo.n_faces or layout.n_vertices != topo.n_vertices:
        raise RuntimeError('%s: the layout is for a mesh of %d vertices and %d faces, topo has %d and %d'
                           % (who, layout.n_vertices, layout.n_faces, topo.n_vertices, topo.n_faces))


def _alloc(want, shapes, device):
    """The output dict: an empty tensor for every name of `shapes` that `want` holds, in the order of `shapes`."""
    return {k: torch.empty(s, dtype=torch.int32 if k == 'pix_to_face' else torch.float32, device=device) for k, s in shapes.items() if k in want}


def _workspace(rows, topo, device):
    return N.workspace('sgdfr_shaperender_workspace_bytes', device, rows, topo.n_vertices, topo.n_faces,
                       error='shape render: unsupported sizes (%d rows, %d vertices, %d faces)' % (rows, topo.n_vertices, topo.n_faces))


def vertex_normals(vertices, topo):
    """util.vertex_normals: vertices [B,V,3] -> unit normals [B,V,3] (zeros for a vertex no face names)."""
    _check_topology('vertex_normals', topo)
    v = _check_vertices('vertex_normals', 'vertices', vertices, topo.n_vertices)
    faces, offsets, entries = topo.tables(v.device)
    out = torch.empty_like(v)
    N.call('sgdfr_shaperender_normals_f32', N.ptr(v), v.shape[0], topo.n_vertices, N.ptr(faces), topo.n_faces, N.ptr(offsets), N.ptr(entries),
           N.ptr(out), N.stream())
    return out


def rasterize(projected, topo, size):
    """rasterize_meshes at blur_radius 0, one face per pixel, no perspective correction, with the x, y flip of renderer.py:53 folded
    in: projected [B,V,3] in normalised image space (+x right, +y down, smaller z nearer) -> (pix_to_face [B,S,S] int32, -1 where no
    face covers, the index counting within the mesh; zbuf [B,S,S]; bary [B,S,S,3]; both -1 where no face covers)."""
    _, _, p, B, dev = _prepare('rasterize', None, topo, None, projected, size)
    faces, _, _ = topo.tables(dev)
    out = _alloc(_WANT, {'pix_to_face': (B, size, size), 'zbuf': (B, size, size), 'bary': (B, size, size, 3)}, dev)
    ws, nbytes = _workspace(B, topo, dev)
    N.call('sgdfr_shaperender_forward_f32', None, N.ptr(p), None, 0.0, B, topo.n_vertices, N.ptr(faces), topo.n_faces, None, None, size,
           None, 0, 0, None, 0, None, None, N.ptr(out['pix_to_face']), N.ptr(out['zbuf']), N.ptr(out['bary']), N.ptr(ws), nbytes, N.stream())
    return out['pix_to_face'], out['zbuf'], out['bary']


_LIGHTS = {}


def _default_lights(device):
    key = str(device)
    if key not in _LIGHTS:
        _LIGHTS[key] = torch.tensor(DEFAULT_LIGHTS, dtype=torch.float32).unsqueeze(0).to(device)
    return _LIGHTS[key]


def render_shape(vertices, topo, cam=None, projected=None, size=224, images=None, lights=None, gan_range=False, want=('shape',),
                 layout=None, detail_normals=None):
    """SRenderY.render_shape: world vertices [B,V,3] and exactly one of cam [B,3] = (s, tx, ty) (projected here as DECA.decode
    does: batch_orth_proj, then y and z negated) and projected [B,V,3] (trans_verts) -> a dict with 'shape' [B,3,S,S] and whatever
    else `want` names of 'alpha' [B,1,S,S], 'pix_to_face' [B,S,S] int32, 'zbuf' [B,S,S], 'bary' [B,S,S,3].

    images: a background [B,3,S,S] (None: black).  lights: [1 or B, L <= 8, 6] = direction, intensity (None: the reference's five
    at 1.7).  'shape' is in the reference's value range, not clamped (it can exceed 1); gan_range=True gives clamp(shape, 0, 1) * 2 - 1,
    the [-1,1] range a float panel of video_frames_px expects.  The reference adds 10 to the z of the caller's projected vertices in
    place; here no argument is modified.

    layout (a detail.UvLayout of this mesh) and detail_normals (the UV normal map [B,3,Su,Su] of detail.detail_normals), both or
    neither: `want` may then also name 'shape_detail' [B,3,S,S] (render_shape(..., detail_normal_images=...) of deca.py:189: the same
    expression with the shading normal sampled from the map), 'grid' [B,S,S,2] (ops['grid']) and 'detail_normal_images' [B,3,S,S],
    all from the one rasterisation; 'shape' keeps the bits it has without them."""
    who = 'render_shape'
    _check_topology(who, topo)
    want = (want,) if isinstance(want, str) else tuple(want)
    if (layout is None) != (detail_normals is None):
        raise RuntimeError('%s: layout and detail_normals must be given together' % who)
    detail = layout is not None
    allowed = _WANT + _WANT_DETAIL if detail else _WANT
    if 'shape' not in want or any(w not in allowed for w in want):
        raise RuntimeError("%s: want must name 'shape' and any of %s, got %r" % (who, allowed[1:], want))
    v, cam, projected, B, dev = _prepare(who, vertices, topo, cam, projected, size)
    S, MAXL = size, N.SHAPERENDER_MAX_LIGHTS
    if images is not None:
        images = _check_map(who, 'images', images, (B, 3, S, S))
    lights = _default_lights(dev) if lights is None else _check_map(who, 'lights', lights, ((1, B), range(1, MAXL + 1), 6),
                                                                    'lights of shape [1 or %d, 1..%d, 6]' % (B, MAXL))
    if detail:
        _check_mesh_layout(who, layout, topo)
        detail_normals = _check_map(who, 'detail_normals', detail_normals, (B, 3, layout.uv_size, layout.uv_size))
    _check_device(who, dev, images, lights, detail_normals)
    faces, offsets, entries = topo.tables(dev)
    out = _alloc(want, {'shape': (B, 3, S, S), 'alpha': (B, 1, S, S), 'pix_to_face': (B, S, S), 'zbuf': (B, S, S), 'bary': (B, S, S, 3),
                        'shape_detail': (B, 3, S, S), 'grid': (B, S, S, 2), 'detail_normal_images': (B, 3, S, S)}, dev)
    ws, nbytes = _workspace(B, topo, dev)
    head = (N.ptr(v), N.ptr(projected), N.ptr(cam), Z_OFFSET, B, topo.n_vertices, N.ptr(faces), topo.n_faces, N.ptr(offsets), N.ptr(entries), S,
            N.ptr(lights), lights.shape[0], lights.shape[1], N.ptr(images), int(bool(gan_range)))
    tail = (N.ptr(out.get('alpha')), N.ptr(out.get('pix_to_face')), N.ptr(out.get('zbuf')), N.ptr(out.get('bary')), N.ptr(ws), nbytes, N.stream())
    if detail:
        N.call('sgdfr_shaperender_detail_f32', *head, N.ptr(layout.tables(dev)[5]), N.ptr(detail_normals), layout.uv_size, N.ptr(out['shape']),
               N.ptr(out.get('shape_detail')), N.ptr(out.get('grid')), N.ptr(out.get('detail_normal_images')), *tail)
    else:
        N.call('sgdfr_shaperender_forward_f32', *head, N.ptr(out['shape']), *tail)
    return out


def _forward_only(who, *tensors):
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise RuntimeError('%s: forward only (no gradient reaches its inputs); call it under torch.no_grad() or on detached tensors' % who)


def sh_constants():
    """The nine factors as the host array the texture entries take."""
    import ctypes
    return (ctypes.c_float * 9)(*SH_CONSTANTS)


def render_texture(vertices, topo, layout, albedo, lights=None, cam=None, projected=None, size=224, want=('images',)):
    """SRenderY.forward (renderer.py:121-191) from one rasterisation: world vertices [B,V,3], exactly one of cam [B,3] and projected
    [B,V,3] (as render_shape takes them), layout (a detail.UvLayout of this mesh), albedo [B,3,Su,Su] at the layout's uv_size (None
    where neither 'images' nor 'albedo_images' is wanted) and lights [B,9,3] (spherical harmonics; None: no shading) -> a dict of what `want` names:

      'images' [B,3,S,S] = albedo_images * shading_images * alpha ('albedo_images' with lights=None);
      'albedo_images' = grid_sample(albedo, grid) * alpha;  'alpha_images' [B,1,S,S]: the coverage, with no front-facing mask;
      'pos_mask' [B,1,S,S]: interpolated transformed-normal z < -0.05;  'normal_images' = the interpolated world normal * alpha;
      'shading_images' = add_SHlight of the interpolated world normal, not renormalised and NOT masked by alpha, as in the reference: an
        uncovered pixel has normal 0 and the value c0 L0 - c8 L8 (0 everywhere with lights=None);
      'grid' [B,S,S,2], bit for bit render_shape's;  'normals', 'transformed_normals' [B,V,3];  'pix_to_face', 'zbuf', 'bary'.

    Point and directional lights ([B,L,6] through SRenderY.forward) are not built.  No argument is modified."""
    who = 'render_texture'
    _check_topology(who, topo)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _WANT_TEXTURE for w in want):
        raise RuntimeError('%s: want must name at least one of %s, got %r' % (who, _WANT_TEXTURE, want))
    _forward_only(who, vertices, albedo, lights, cam, projected)
    v, cam, projected, B, dev = _prepare(who, vertices, topo, cam, projected, size)
    _check_mesh_layout(who, layout, topo)
    Su = layout.uv_size
    if albedo is None:
        if 'images' in want or 'albedo_images' in want:
            raise RuntimeError("%s: 'images' and 'albedo_images' need an albedo" % who)
    else:
        albedo = _check_map(who, 'albedo', albedo, (B, 3, Su, Su))
    if lights is not None:
        if torch.is_tensor(lights) and lights.ndim == 3 and lights.shape[2] == 6:
            raise RuntimeError('%s: point and directional lights [B,L,6] have no HIP kernel here; pass spherical-harmonic lights [B,9,3]' % who)
        lights = _check_map(who, 'lights', lights, (B, 9, 3))
    _check_device(who, dev, albedo, lights)
    faces, offsets, entries = topo.tables(dev)
    V, S = topo.n_vertices, size
    out = _alloc(want, {'images': (B, 3, S, S), 'albedo_images': (B, 3, S, S), 'alpha_images': (B, 1, S, S), 'pos_mask': (B, 1, S, S),
                        'shading_images': (B, 3, S, S), 'grid': (B, S, S, 2), 'normal_images': (B, 3, S, S), 'normals': (B, V, 3),
                        'transformed_normals': (B, V, 3), 'pix_to_face': (B, S, S), 'zbuf': (B, S, S), 'bary': (B, S, S, 3)}, dev)
    ws, nbytes = _workspace(B, topo, dev)
    face_uv = layout.tables(dev)[5]
    N.call('sgdfr_shaperender_texture_f32', N.ptr(v), N.ptr(projected), N.ptr(cam), Z_OFFSET, B, V, N.ptr(faces), topo.n_faces, N.ptr(offsets),
           N.ptr(entries), S, N.ptr(lights), sh_constants(), N.ptr(face_uv), N.ptr(albedo), Su, *[N.ptr(out.get(k)) for k in _WANT_TEXTURE],
           N.ptr(ws), nbytes, N.stream())
    return out


def _render_attr(who, projected, values, topo, size, z_offset):
    _forward_only(who, projected, values)
    _, _, p, B, dev = _prepare(who, None, topo, None, projected, size)
    V = topo.n_vertices
    a = _check_map(who, 'the per-vertex values', values, (B, V, (1, 2, 3)), 'per-vertex values of shape [%d,%d,1..3]' % (B, V))
    if a.device != dev:
        raise RuntimeError('%s: all tensors must live on one device' % who)
    D = a.shape[2]
    faces, _, _ = topo.tables(dev)
    out = torch.empty((B, D, size, size), dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(B, topo, dev)
    N.call('sgdfr_shaperender_attr_f32', N.ptr(p), float(z_offset), B, V, N.ptr(faces), topo.n_faces, size, N.ptr(a), D, N.ptr(out), None, None,
           None, N.ptr(ws), nbytes, N.stream())
    return out


def render_normal(projected, normals, topo, size=224, z_offset=0.0):
    """SRenderY.render_normal (renderer.py:316-329): per-vertex values [B,V,3] interpolated over the rasterisation of projected
    [B,V,3] -> [B,3,S,S], 0 where no face covers.  The reference rasterises what it is given -- by the time DECA calls it, 10 has been
    added to z in place -- so z_offset is 0 here; pass z_offset=10 for vertices that still hold DECA's projected z."""
    return _render_attr('render_normal', projected, normals, topo, size, z_offset)


def render_depth(projected, topo, size=224):
    """SRenderY.render_depth (renderer.py:295-314): [B,1,S,S], 1 for the nearest vertex of the whole batch, 0 for the farthest and
    where no face covers.  The minimum and maximum over the batch are torch reductions on the device in front of the launch (no host
    synchronisation); the vertices are rasterised at z - min(z) + 10, and the caller's tensor is not modified."""
    who = 'render_depth'
    _forward_only(who, projected)
    p = _prepare(who, None, topo, None, projected, size)[2]
    z = p[:, :, 2:] - p[:, :, 2].min()
    d = -z
    d = d - d.min()
    d = d / d.max()
    return _render_attr(who, torch.cat([p[:, :, :2], z], 2), d, topo, size, Z_OFFSET)

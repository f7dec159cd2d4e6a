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


def _check_vertices(who, name, t, topo, rows=None):
    if not torch.is_tensor(t):
        raise RuntimeError('%s: %s must be a tensor, got %s' % (who, name, type(t)))
    N.require_device(t)
    if t.ndim != 3 or t.shape[0] < 1 or tuple(t.shape[1:]) != (topo.n_vertices, 3) or (rows is not None and t.shape[0] != rows):
        raise RuntimeError('%s: expected %s of shape [%s,%d,3], got %s' % (who, name, 'B' if rows is None else rows, topo.n_vertices, tuple(t.shape)))
    return N.f32c(t.detach())


def _check_size(who, size):
    if isinstance(size, bool) or not isinstance(size, int) or not 1 <= size <= N.SHAPERENDER_MAX_SIZE:
        raise RuntimeError('%s: size must be an int in 1..%d, got %r' % (who, N.SHAPERENDER_MAX_SIZE, size))


def _workspace(rows, topo, device):
    return N.workspace('sgdfr_shaperender_workspace_bytes', device, rows, topo.n_vertices, topo.n_faces,
                       error='shape render: unsupported sizes (%d rows, %d vertices, %d faces)' % (rows, topo.n_vertices, topo.n_faces))


def vertex_normals(vertices, topo):
    """util.vertex_normals: vertices [B,V,3] -> unit normals [B,V,3] (zeros for a vertex no face names)."""
    _check_topology('vertex_normals', topo)
    v = _check_vertices('vertex_normals', 'vertices', vertices, topo)
    faces, offsets, entries = topo.tables(v.device)
    out = torch.empty_like(v)
    N.call('sgdfr_shaperender_normals_f32', N.ptr(v), v.shape[0], topo.n_vertices, N.ptr(faces), topo.n_faces, N.ptr(offsets), N.ptr(entries),
           N.ptr(out), N.stream())
    return out


def rasterize(projected, topo, size):
    """rasterize_meshes at blur_radius 0, one face per pixel, no perspective correction, with the x, y flip of renderer.py:53 folded
    in: projected [B,V,3] in normalised image space (+x right, +y down, smaller z nearer) -> (pix_to_face [B,S,S] int32, -1 where no
    face covers, the index counting within the mesh; zbuf [B,S,S]; bary [B,S,S,3]; both -1 where no face covers)."""
    _check_topology('rasterize', topo)
    p = _check_vertices('rasterize', 'projected', projected, topo)
    _check_size('rasterize', size)
    B, dev = p.shape[0], p.device
    faces, _, _ = topo.tables(dev)
    pix = torch.empty((B, size, size), dtype=torch.int32, device=dev)
    zbuf = torch.empty((B, size, size), dtype=torch.float32, device=dev)
    bary = torch.empty((B, size, size, 3), dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(B, topo, dev)
    N.call('sgdfr_shaperender_forward_f32', None, N.ptr(p), None, 0.0, B, topo.n_vertices, N.ptr(faces), topo.n_faces, None, None, size,
           None, 0, 0, None, 0, None, None, N.ptr(pix), N.ptr(zbuf), N.ptr(bary), N.ptr(ws), nbytes, N.stream())
    return pix, zbuf, bary


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
    if detail:
        if 'shape' not in want or any(w not in _WANT + _WANT_DETAIL for w in want):
            raise RuntimeError("%s: want must name 'shape' and any of %s, got %r" % (who, _WANT[1:] + _WANT_DETAIL, want))
    elif 'shape' not in want or any(w not in _WANT for w in want):
        raise RuntimeError("%s: want must name 'shape' and any of %s, got %r" % (who, _WANT[1:], want))
    if (cam is None) == (projected is None):
        raise RuntimeError('%s: exactly one of cam and projected must be given' % who)
    v = _check_vertices(who, 'vertices', vertices, topo)
    _check_size(who, size)
    B, dev = v.shape[0], v.device
    if cam is not None:
        if not torch.is_tensor(cam):
            raise RuntimeError('%s: cam must be a tensor, got %s' % (who, type(cam)))
        N.require_device(cam)
        if tuple(cam.shape) != (B, 3):
            raise RuntimeError('%s: expected cam of shape [%d,3], got %s' % (who, B, tuple(cam.shape)))
        cam = N.f32c(cam.detach())
    else:
        projected = _check_vertices(who, 'projected', projected, topo, B)
    if images is not None:
        if not torch.is_tensor(images):
            raise RuntimeError('%s: images must be a tensor, got %s' % (who, type(images)))
        N.require_device(images)
        if tuple(images.shape) != (B, 3, size, size):
            raise RuntimeError('%s: expected images of shape [%d,3,%d,%d], got %s' % (who, B, size, size, tuple(images.shape)))
        images = N.f32c(images.detach())
    if lights is None:
        lights = _default_lights(dev)
    else:
        if not torch.is_tensor(lights):
            raise RuntimeError('%s: lights must be a tensor, got %s' % (who, type(lights)))
        N.require_device(lights)
        if lights.ndim != 3 or lights.shape[0] not in (1, B) or not 1 <= lights.shape[1] <= N.SHAPERENDER_MAX_LIGHTS or lights.shape[2] != 6:
            raise RuntimeError('%s: expected lights of shape [1 or %d, 1..%d, 6], got %s' % (who, B, N.SHAPERENDER_MAX_LIGHTS, tuple(lights.shape)))
        lights = N.f32c(lights.detach())
    if detail:
        from .detail import UvLayout
        if not isinstance(layout, UvLayout):
            raise RuntimeError('%s: layout must be a detail.UvLayout, got %s' % (who, type(layout)))
        if layout.n_faces != topo.n_faces or layout.n_vertices != topo.n_vertices:
            raise RuntimeError('%s: the layout is for a mesh of %d vertices and %d faces, topo has %d and %d'
                               % (who, layout.n_vertices, layout.n_faces, topo.n_vertices, topo.n_faces))
        if not torch.is_tensor(detail_normals):
            raise RuntimeError('%s: detail_normals must be a tensor, got %s' % (who, type(detail_normals)))
        N.require_device(detail_normals)
        Su = layout.uv_size
        if tuple(detail_normals.shape) != (B, 3, Su, Su):
            raise RuntimeError('%s: expected detail_normals of shape [%d,3,%d,%d], got %s' % (who, B, Su, Su, tuple(detail_normals.shape)))
        detail_normals = N.f32c(detail_normals.detach())
    if any(t is not None and t.device != dev for t in (cam, projected, images, lights, detail_normals)):
        raise RuntimeError('%s: all tensors must live on the vertices\' device %s' % (who, dev))
    faces, offsets, entries = topo.tables(dev)
    out = {'shape': torch.empty((B, 3, size, size), dtype=torch.float32, device=dev)}
    for name, shape, dtype in (('alpha', (B, 1, size, size), torch.float32), ('pix_to_face', (B, size, size), torch.int32),
                               ('zbuf', (B, size, size), torch.float32), ('bary', (B, size, size, 3), torch.float32)):
        if name in want:
            out[name] = torch.empty(shape, dtype=dtype, device=dev)
    ws, nbytes = _workspace(B, topo, dev)
    if detail:
        for name, shape in (('shape_detail', (B, 3, size, size)), ('grid', (B, size, size, 2)), ('detail_normal_images', (B, 3, size, size))):
            if name in want:
                out[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        face_uv = layout.tables(dev)[5]
        N.call('sgdfr_shaperender_detail_f32', N.ptr(v), N.ptr(projected), N.ptr(cam), Z_OFFSET, B, topo.n_vertices, N.ptr(faces), topo.n_faces,
               N.ptr(offsets), N.ptr(entries), size, N.ptr(lights), lights.shape[0], lights.shape[1], N.ptr(images), int(bool(gan_range)),
               N.ptr(face_uv), N.ptr(detail_normals), layout.uv_size, N.ptr(out['shape']), N.ptr(out.get('shape_detail')), N.ptr(out.get('grid')),
               N.ptr(out.get('detail_normal_images')), N.ptr(out.get('alpha')), N.ptr(out.get('pix_to_face')), N.ptr(out.get('zbuf')),
               N.ptr(out.get('bary')), N.ptr(ws), nbytes, N.stream())
        return out
    N.call('sgdfr_shaperender_forward_f32', N.ptr(v), N.ptr(projected), N.ptr(cam), Z_OFFSET, B, topo.n_vertices, N.ptr(faces), topo.n_faces,
           N.ptr(offsets), N.ptr(entries), size, N.ptr(lights), lights.shape[0], lights.shape[1], N.ptr(images), int(bool(gan_range)),
           N.ptr(out['shape']), N.ptr(out.get('alpha')), N.ptr(out.get('pix_to_face')), N.ptr(out.get('zbuf')), N.ptr(out.get('bary')),
           N.ptr(ws), nbytes, N.stream())
    return out


def _forward_only(who, *tensors):
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise RuntimeError('%s: forward only (no gradient reaches its inputs); call it under torch.no_grad() or on detached tensors' % who)


def _check_map(who, name, t, shape):
    if not torch.is_tensor(t):
        raise RuntimeError('%s: %s must be a tensor, got %s' % (who, name, type(t)))
    N.require_device(t)
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError('%s: expected %s of shape [%s], got %s' % (who, name, ','.join(map(str, shape)), tuple(t.shape)))
    return N.f32c(t.detach())


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
    if (cam is None) == (projected is None):
        raise RuntimeError('%s: exactly one of cam and projected must be given' % who)
    from .detail import UvLayout
    if not isinstance(layout, UvLayout):
        raise RuntimeError('%s: layout must be a detail.UvLayout, got %s' % (who, type(layout)))
    if layout.n_faces != topo.n_faces or layout.n_vertices != topo.n_vertices:
        raise RuntimeError('%s: the layout is for a mesh of %d vertices and %d faces, topo has %d and %d'
                           % (who, layout.n_vertices, layout.n_faces, topo.n_vertices, topo.n_faces))
    _forward_only(who, vertices, albedo, lights, cam, projected)
    v = _check_vertices(who, 'vertices', vertices, topo)
    _check_size(who, size)
    B, dev, Su = v.shape[0], v.device, layout.uv_size
    if cam is not None:
        cam = _check_map(who, 'cam', cam, (B, 3))
    else:
        projected = _check_vertices(who, 'projected', projected, topo, B)
    if albedo is None:
        if 'images' in want or 'albedo_images' in want:
            raise RuntimeError("%s: 'images' and 'albedo_images' need an albedo" % who)
    else:
        albedo = _check_map(who, 'albedo', albedo, (B, 3, Su, Su))
    if lights is not None:
        if torch.is_tensor(lights) and lights.ndim == 3 and lights.shape[2] == 6:
            raise RuntimeError('%s: point and directional lights [B,L,6] have no HIP kernel here; pass spherical-harmonic lights [B,9,3]' % who)
        lights = _check_map(who, 'lights', lights, (B, 9, 3))
    if any(t is not None and t.device != dev for t in (cam, projected, albedo, lights)):
        raise RuntimeError('%s: all tensors must live on the vertices\' device %s' % (who, dev))
    faces, offsets, entries = topo.tables(dev)
    V, S = topo.n_vertices, size
    shapes = {'images': (B, 3, S, S), 'albedo_images': (B, 3, S, S), 'alpha_images': (B, 1, S, S), 'pos_mask': (B, 1, S, S),
              'shading_images': (B, 3, S, S), 'grid': (B, S, S, 2), 'normal_images': (B, 3, S, S), 'normals': (B, V, 3),
              'transformed_normals': (B, V, 3), 'pix_to_face': (B, S, S), 'zbuf': (B, S, S), 'bary': (B, S, S, 3)}
    out = {k: torch.empty(shapes[k], dtype=torch.int32 if k == 'pix_to_face' else torch.float32, device=dev) for k in _WANT_TEXTURE if k in want}
    ws, nbytes = _workspace(B, topo, dev)
    face_uv = layout.tables(dev)[5]
    N.call('sgdfr_shaperender_texture_f32', N.ptr(v), N.ptr(projected), N.ptr(cam), Z_OFFSET, B, V, N.ptr(faces), topo.n_faces, N.ptr(offsets),
           N.ptr(entries), S, N.ptr(lights), sh_constants(), N.ptr(face_uv), N.ptr(albedo), Su, *[N.ptr(out.get(k)) for k in _WANT_TEXTURE],
           N.ptr(ws), nbytes, N.stream())
    return out


def _render_attr(who, projected, values, topo, size, z_offset):
    _check_topology(who, topo)
    _forward_only(who, projected, values)
    p = _check_vertices(who, 'projected', projected, topo)
    _check_size(who, size)
    if not torch.is_tensor(values):
        raise RuntimeError('%s: the per-vertex values must be a tensor, got %s' % (who, type(values)))
    N.require_device(values)
    B, V = p.shape[0], topo.n_vertices
    if values.ndim != 3 or tuple(values.shape[:2]) != (B, V) or not 1 <= values.shape[2] <= 3:
        raise RuntimeError('%s: expected per-vertex values of shape [%d,%d,1..3], got %s' % (who, B, V, tuple(values.shape)))
    if values.device != p.device:
        raise RuntimeError('%s: all tensors must live on one device' % who)
    a = N.f32c(values.detach())
    D = a.shape[2]
    faces, _, _ = topo.tables(p.device)
    out = torch.empty((B, D, size, size), dtype=torch.float32, device=p.device)
    ws, nbytes = _workspace(B, topo, p.device)
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
    _check_topology(who, topo)
    _forward_only(who, projected)
    p = _check_vertices(who, 'projected', projected, topo)
    z = p[:, :, 2:] - p[:, :, 2].min()
    d = -z
    d = d - d.min()
    d = d / d.max()
    return _render_attr(who, torch.cat([p[:, :, :2], z], 2), d, topo, size, Z_OFFSET)

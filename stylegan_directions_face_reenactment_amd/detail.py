"""DECA's detail path on the HIP kernels of csrc/detail.hip and csrc/shaperender.hip: the counterpart of decalib/models/decoders.py
Generator (D_detail), of DECA.displacement2normal / displacement2vertex (deca.py:114-141) with SRenderY.world2uv
(utils/renderer.py:331-340) and util.generate_triangles, and of the detail half of DECA.decode_deca (deca.py:160-227).

    ckpt = torch.load('deca_model.tar')
    E = deca.ResnetEncoder(236); E.load_state_dict(ckpt['E_flame'])
    E_detail = deca.ResnetEncoder(128); E_detail.load_state_dict(ckpt['E_detail'])
    D = DetailDecoder(); D.load_state_dict(ckpt['D_detail'])             # all three .cuda().eval()
    layout = UvLayout.from_obj('head_template.obj', 256, face_eye_mask, fixed_dis)
    code = deca.encode(E, images, M, E_detail=E_detail)
    out = decode_detail(F, D, layout, code)          # 'uv_z', 'displacement_map', 'uv_detail_normals', 'shape_images',
                                                     # 'shape_detail_images', 'detail_normal_images'

`DetailDecoder` has the module layout and state-dict keys of the reference's Generator and holds the weights only, frozen at
construction; the HIP kernels run it in eval mode.  Its six BatchNorms are folded on the host in fp64 -- the first (eps 1e-5) into
the Linear, the other five are nn.BatchNorm2d(C, 0.8), whose second argument is eps = 0.8 -- and each upsample + conv layer is one
launch whose gather computes the bilinear value on the fly (no upsampled tensor exists).  `UvLayout` holds the UV side of a mesh and,
per device, the UV table (pix_to_face, bary) that shape_render.rasterize gives for the UV vertices.  Forward only, no host
synchronisation: everything runs on the current stream and captures into a graph.  The texture side (albedo sampling, add_SHlight,
uv_texture, uv_texture_gt), visofp, render_depth / render_normal and decode_deca as a whole are texture.py; any backward is out of scope.
"""
import numpy as np
import torch
from torch import nn

from . import _native as N
from .packs import PackedWeights, views
from .shape_render import MeshTopology, _check_device, _check_map, _check_vertices, render_shape, vertex_normals, rasterize

LATENT, UV_SIZE = N.DETAIL_LATENT, N.DETAIL_UV_SIZE
_CHANNELS = ((128, 128), (128, 64), (64, 64), (64, 32), (32, 16))       # the five up + conv layers
_CONVS = (2, 6, 10, 14, 18, 21)                                         # conv_blocks indices of the convs; BatchNorms at + 1
TAP_SHAPES = ((128, 8, 8),) + tuple((co, 16 << i, 16 << i) for i, (_, co) in enumerate(_CHANNELS))


class DetailDecoder(PackedWeights, nn.Module):
    """decoders.Generator(latent_dim=181, out_channels=1, out_scale=0.01, sample_mode='bilinear'): weights only.
    forward(latent [B,181]) -> uv_z [B,1,256,256] on the HIP kernels."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_detail_prepack_f32', 'sgdfr_detail_pack_elems', N.DETAIL_PARAMS
    TRAIN_ERROR = 'DetailDecoder: the HIP kernels run the decoder in eval mode only (running BatchNorm statistics); call .eval()'
    GRAD_ERROR = 'DetailDecoder: the HIP kernels give no gradient for the decoder weights; keep every parameter at requires_grad=False'

    def __init__(self, latent_dim=LATENT, out_channels=1, out_scale=0.01, sample_mode='bilinear'):
        if latent_dim != LATENT or out_channels != 1 or sample_mode != 'bilinear':
            raise NotImplementedError("DetailDecoder: only latent_dim=181, out_channels=1, sample_mode='bilinear' have HIP kernels "
                                      '(got %r, %r, %r)' % (latent_dim, out_channels, sample_mode))
        super().__init__()
        self.out_scale = float(out_scale)
        self.init_size = 8
        self.l1 = nn.Sequential(nn.Linear(latent_dim, 128 * self.init_size ** 2))
        blocks = [nn.BatchNorm2d(128)]
        for cin, cout in _CHANNELS:
            blocks += [nn.Upsample(scale_factor=2, mode=sample_mode), nn.Conv2d(cin, cout, 3, stride=1, padding=1),
                       nn.BatchNorm2d(cout, 0.8), nn.LeakyReLU(0.2, inplace=True)]       # BatchNorm2d(C, 0.8): eps = 0.8
        blocks += [nn.Conv2d(16, out_channels, 3, stride=1, padding=1), nn.Tanh()]
        self.conv_blocks = nn.Sequential(*blocks)
        for p in self.parameters():
            p.requires_grad = False

    def folded(self, dtype=torch.float32):
        """The 14 tensors sgdfr_detail_prepack_f32 takes, every BatchNorm folded in fp64 on the parameters' device, in `dtype`."""
        def scale_shift(bn):
            s = bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + bn.eps)
            return s, bn.bias.detach().double() - bn.running_mean.detach().double() * s

        lin, cb = self.l1[0], self.conv_blocks
        per = self.init_size ** 2
        s, h = scale_shift(cb[0])
        s, h = s.repeat_interleave(per), h.repeat_interleave(per)      # channel of Linear row r: r // 64
        out = [lin.weight.detach().double() * s[:, None], lin.bias.detach().double() * s + h]
        for i in _CONVS[:-1]:
            s, h = scale_shift(cb[i + 1])
            out += [cb[i].weight.detach().double() * s.view(-1, 1, 1, 1), cb[i].bias.detach().double() * s + h]
        out += [cb[_CONVS[-1]].weight.detach().double(), cb[_CONVS[-1]].bias.detach().double()]
        return [v.to(dtype).contiguous() for v in out]

    def forward(self, latent):
        return decode_uv(self, latent)


def tap_views(taps, rows):
    """The taps buffer of decode_uv as views [rows, C, h, h]: the Linear's output, then the five layers' outputs."""
    take = views(taps, rows)
    out = [take(shape) for shape in TAP_SHAPES]
    take.done()
    return out


def _check_latent(latent):
    z = _check_map('DetailDecoder', 'latent', latent, (None, LATENT), 'a latent of shape [B,%d] = cat(pose[:, 3:], exp, detail)' % LATENT)
    if torch.is_grad_enabled() and latent.requires_grad:
        raise RuntimeError('DetailDecoder: the detail path is forward only; call it under torch.no_grad() or on a detached latent')
    return z


def decode_uv(D, latent, taps=False):
    """uv_z [B,1,256,256] of D_detail for latent [B,181]; taps=True: (uv_z, the six stage outputs as tap_views gives them)."""
    D.check()
    z = _check_latent(latent)
    B, dev = z.shape[0], z.device
    ws, nbytes = N.workspace('sgdfr_detail_workspace_bytes', dev, B, error='DetailDecoder: unsupported batch of %d rows' % B)
    uv_z = torch.empty((B, 1, UV_SIZE, UV_SIZE), dtype=torch.float32, device=dev)
    buf = torch.empty(B * sum(c * h * w for c, h, w in TAP_SHAPES), dtype=torch.float32, device=dev) if taps else None
    N.call('sgdfr_detail_decode_f32', N.ptr(z), B, N.ptr(D.packed()), D.out_scale, N.ptr(uv_z), N.ptr(buf), N.ptr(ws), nbytes, N.stream())
    return (uv_z, tap_views(buf, B)) if taps else uv_z


def upconv(x, weight, bias, slope=0.2, up=True):
    """The layer kernel alone: lrelu(conv3x3(upsample2x(x) if up else x, weight, pad 1) + bias, slope); slope=1: no activation.
    x [B,Cin,h,w], weight [Cout,Cin,3,3], bias [Cout]; Cin, Cout <= 1024, h, w <= 256."""
    N.require_device(x, weight, bias)
    if x.ndim != 4 or weight.ndim != 4 or tuple(weight.shape[1:]) != (x.shape[1], 3, 3) or tuple(bias.shape) != (weight.shape[0],):
        raise RuntimeError('upconv: expected x [B,Cin,h,w], weight [Cout,Cin,3,3], bias [Cout], got %s, %s, %s'
                           % (tuple(x.shape), tuple(weight.shape), tuple(bias.shape)))
    B, cin, h, w = x.shape
    cout, f = weight.shape[0], 2 if up else 1
    ws, nbytes = N.workspace('sgdfr_detail_upconv_workspace_bytes', x.device, cin, cout,
                             error='upconv: unsupported channel counts %d -> %d (1..1024)' % (cin, cout))
    y = torch.empty((B, cout, f * h, f * w), dtype=torch.float32, device=x.device)
    N.call('sgdfr_detail_upconv_f32', N.ptr(N.f32c(x.detach())), N.ptr(N.f32c(weight.detach())), N.ptr(N.f32c(bias.detach())), B, cin, cout,
           h, w, float(slope), int(bool(up)), N.ptr(y), N.ptr(ws), nbytes, N.stream())
    return y


# ---------------------------------------------------------------------------------------------------------------- UV space
def dense_triangles(h, w, margin_x=2, margin_y=5):
    """util.generate_triangles(h, w): per quad (y, x), x in [margin_x, w-1-margin_x) outermost, y in [margin_y, h-1-margin_y), the
    two triangles (a, c, b), (b, c, d) of a = y w + x, b = a + 1, c = a + w, d = c + 1 -> int64 [n,3]."""
    x = np.arange(margin_x, w - 1 - margin_x, dtype=np.int64)
    y = np.arange(margin_y, h - 1 - margin_y, dtype=np.int64)
    a = (y[None, :] * w + x[:, None]).reshape(-1)
    b, c, d = a + 1, a + w, a + w + 1
    return np.stack([np.stack([a, c, b], 1), np.stack([b, c, d], 1)], 1).reshape(-1, 3)


class UvLayout:
    """The UV side of a mesh, as SRenderY holds it (renderer.py:95-112): faces [F,3] into the V mesh vertices, uvcoords [Vt,2] in
    [0,1], uvfaces [F,3] into them, the UV map side S = uv_size (13..1024), and the two [S,S] maps of the detail path:
    face_eye_mask and fixed_dis.  Built on the host: the reference's `uvcoords` buffer (2u - 1, -(2v - 1), 1) as uv_vertices [Vt,3],
    face_uv [F,3,2] (the first two components of face_uvcoords) and dense_faces = util.generate_triangles(S, S).  Per device, on
    first use: the UV table pix_to_face [S,S] and bary [S,S,3] of shape_render.rasterize on uv_vertices over uvfaces (that call has
    the reference rasteriser's x, y flip folded in, so the buffer goes in unchanged)."""

    def __init__(self, faces, uvcoords, uvfaces, uv_size, face_eye_mask, fixed_dis, n_vertices=None):
        S = uv_size
        if isinstance(S, bool) or not isinstance(S, int) or not N.DETAIL_UV_MIN <= S <= N.DETAIL_UV_MAX:
            raise RuntimeError('UvLayout: uv_size must be an int in %d..%d, got %r' % (N.DETAIL_UV_MIN, N.DETAIL_UV_MAX, S))
        faces, uvfaces = torch.as_tensor(faces).detach().cpu(), torch.as_tensor(uvfaces).detach().cpu()
        uv = torch.as_tensor(uvcoords).detach().cpu().to(torch.float64)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or tuple(uvfaces.shape) != tuple(faces.shape):
            raise RuntimeError('UvLayout: expected faces and uvfaces of one shape [F,3], got %s and %s' % (tuple(faces.shape), tuple(uvfaces.shape)))
        if uv.ndim != 2 or uv.shape[1] != 2 or uv.shape[0] < 1:
            raise RuntimeError('UvLayout: expected uvcoords of shape [Vt,2], got %s' % (tuple(uv.shape),))
        faces, uvfaces = faces.to(torch.int64), uvfaces.to(torch.int64)
        V = int(faces.max()) + 1 if n_vertices is None else int(n_vertices)
        if int(faces.min()) < 0 or int(faces.max()) >= V or int(uvfaces.min()) < 0 or int(uvfaces.max()) >= uv.shape[0]:
            raise RuntimeError('UvLayout: faces or uvfaces hold indices outside their vertex lists')
        maps = []
        for name, m in (('face_eye_mask', face_eye_mask), ('fixed_dis', fixed_dis)):
            m = torch.as_tensor(m).detach().cpu().to(torch.float32)
            if tuple(m.shape) != (S, S):
                raise RuntimeError('UvLayout: expected %s of shape [%d,%d] (already at uv_size), got %s' % (name, S, S, tuple(m.shape)))
            maps.append(m.contiguous())
        self.uv_size, self.n_vertices, self.n_faces = S, V, int(faces.shape[0])
        self.faces = faces.to(torch.int32).contiguous()
        self.uv_vertices = torch.stack([2 * uv[:, 0] - 1, -(2 * uv[:, 1] - 1), torch.ones_like(uv[:, 0])], 1).to(torch.float32)
        self.uv_topology = MeshTopology(uvfaces, int(uv.shape[0]))
        self.face_uv = self.uv_vertices[uvfaces][:, :, :2].contiguous()
        self.face_eye_mask, self.fixed_dis = maps
        self.dense_faces = torch.from_numpy(dense_triangles(S, S))
        self._device = {}

    @classmethod
    def from_obj(cls, path, uv_size, face_eye_mask, fixed_dis):
        """From a Wavefront file: its `v`, `vt` and triangle `f a/b[/c]` lines (what util.load_obj gives the reference for
        head_template.obj); anything else in the file is skipped."""
        n_v, vt, f, ft = 0, [], [], []
        with open(path) as fh:
            for line in fh:
                tok = line.split()
                if not tok:
                    continue
                if tok[0] == 'v':
                    n_v += 1
                elif tok[0] == 'vt':
                    vt.append((float(tok[1]), float(tok[2])))
                elif tok[0] == 'f':
                    if len(tok) != 4:
                        raise RuntimeError('UvLayout.from_obj: %s holds a face that is no triangle: %r' % (path, line.strip()))
                    corners = [t.split('/') for t in tok[1:]]
                    if any(len(c) < 2 or not c[1] for c in corners):
                        raise RuntimeError('UvLayout.from_obj: %s holds a face without texture indices: %r' % (path, line.strip()))
                    f.append([int(c[0]) - 1 for c in corners])
                    ft.append([int(c[1]) - 1 for c in corners])
        if not f or not vt or not n_v:
            raise RuntimeError('UvLayout.from_obj: %s holds no v / vt / f lines' % path)
        return cls(torch.tensor(f), torch.tensor(vt, dtype=torch.float64), torch.tensor(ft), uv_size, face_eye_mask, fixed_dis, n_vertices=n_v)

    def dense_topology(self):
        """MeshTopology of the dense faces over the S*S texels (displacement2vertex's detail_faces)."""
        if '_dense' not in self.__dict__:
            self._dense = MeshTopology(self.dense_faces, self.uv_size * self.uv_size)
        return self._dense

    def tables(self, device):
        """(faces int32 [F,3], pix_to_face int32 [S,S], bary [S,S,3], face_eye_mask [S,S], fixed_dis [S,S], face_uv [F,3,2]) on
        `device`; the UV table is rasterised there on first use."""
        key = str(device)
        if key not in self._device:
            pix, _, bary = rasterize(self.uv_vertices.to(device).unsqueeze(0), self.uv_topology, self.uv_size)
            self._device[key] = (self.faces.to(device), pix[0].contiguous(), bary[0].contiguous(), self.face_eye_mask.to(device),
                                 self.fixed_dis.to(device), self.face_uv.to(device))
        return self._device[key]

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_device'] = {}
        state.pop('_dense', None)
        return state


def _check_layout(who, layout):
    if not isinstance(layout, UvLayout):
        raise RuntimeError('%s: layout must be a UvLayout, got %s' % (who, type(layout)))


def world2uv(layout, values):
    """SRenderY.world2uv: per-vertex values [B,V,3] -> [B,3,S,S]; per texel sum_k bary_k values[faces[f][k]], 0 where no face covers."""
    _check_layout('world2uv', layout)
    v = _check_vertices('world2uv', 'values', values, layout.n_vertices)
    faces, pix, bary, _, _, _ = layout.tables(v.device)
    S = layout.uv_size
    out = torch.empty((v.shape[0], 3, S, S), dtype=torch.float32, device=v.device)
    N.call('sgdfr_detail_world2uv_f32', N.ptr(v), v.shape[0], layout.n_vertices, N.ptr(faces), layout.n_faces, N.ptr(pix), N.ptr(bary), S,
           N.ptr(out), N.stream())
    return out


def detail_normals(layout, uv_z, verts, normals, dense_vertices=False):
    """DECA.displacement2normal: uv_z [B,1,S,S], coarse vertices and their normals [B,V,3] -> uv_detail_normals [B,3,S,S] in one
    launch; dense_vertices=True: (uv_detail_normals, dense vertices [B,S*S,3]) -- displacement2vertex's, over layout.dense_faces."""
    who = 'detail_normals'
    _check_layout(who, layout)
    v = _check_vertices(who, 'verts', verts, layout.n_vertices)
    n = _check_vertices(who, 'normals', normals, layout.n_vertices, v.shape[0])
    S, B = layout.uv_size, v.shape[0]
    z = _check_map(who, 'uv_z', uv_z, (B, 1, S, S))
    _check_device(who, v.device, z, n)
    faces, pix, bary, mask, fixed, _ = layout.tables(v.device)
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=v.device)
    dense = torch.empty((B, S * S, 3), dtype=torch.float32, device=v.device) if dense_vertices else None
    N.call('sgdfr_detail_uvnormals_f32', N.ptr(z), N.ptr(v), N.ptr(n), B, layout.n_vertices, N.ptr(faces), layout.n_faces, N.ptr(pix), N.ptr(bary),
           N.ptr(mask), N.ptr(fixed), S, N.ptr(out), N.ptr(dense), N.stream())
    return (out, dense) if dense_vertices else out


# ---------------------------------------------------------------------------------------------------------------- composition
def decode_detail(flame, D_detail, layout, codedict, size=224, images=None, gan_range=False):
    """The detail half of DECA.decode_deca (deca.py:160-227) for codedict['shape' | 'exp' | 'pose' | 'cam' | 'detail'] ('alpha_shp' /
    'alpha_exp' are taken too): {'uv_z' [B,1,256,256], 'displacement_map' = uv_z + fixed_dis, 'uv_detail_normals' [B,3,256,256],
    'shape_images', 'shape_detail_images', 'detail_normal_images' [B,3,size,size]}.  One rasterisation serves both panels.  Forward
    only, no host synchronisation; every argument is checked before the first launch."""
    from . import flame as FL
    from .shape_render import _check_size
    who = 'decode_detail'
    _check_layout(who, layout)
    _check_size(who, size)
    if not isinstance(D_detail, DetailDecoder):
        raise RuntimeError('%s: D_detail must be a DetailDecoder, got %s' % (who, type(D_detail)))
    D_detail.check()
    if layout.uv_size != UV_SIZE:
        raise RuntimeError('%s: D_detail writes %d x %d maps, the layout has uv_size=%d' % (who, UV_SIZE, UV_SIZE, layout.uv_size))
    pick = lambda a, b: codedict[a] if a in codedict else codedict[b]
    with torch.no_grad():
        shape, exp, pose, cam = FL._check_coeffs(pick('alpha_shp', 'shape'), pick('alpha_exp', 'exp'), codedict['pose'], codedict['cam'])
        detail, B = codedict['detail'], pose.shape[0]
        if not torch.is_tensor(detail) or tuple(detail.shape) != (B, LATENT - 3 - exp.shape[1]):
            raise RuntimeError('%s: expected a detail code of shape [%d,%d], got %s'
                               % (who, B, LATENT - 3 - exp.shape[1], tuple(detail.shape) if torch.is_tensor(detail) else type(detail)))
        N.require_device(detail)
        topo = FL.topology(flame)
        if topo.n_vertices != layout.n_vertices or topo.n_faces != layout.n_faces:
            raise RuntimeError('%s: the layout is for a mesh of %d vertices and %d faces, FLAME has %d and %d'
                               % (who, layout.n_vertices, layout.n_faces, topo.n_vertices, topo.n_faces))
        if images is not None and (not torch.is_tensor(images) or not images.is_cuda or tuple(images.shape) != (B, 3, size, size)):
            raise RuntimeError('%s: expected images as a GPU tensor of shape [%d,3,%d,%d]' % (who, B, size, size))
        if any(t.device != pose.device for t in (detail, cam) + (() if images is None else (images,))):
            raise RuntimeError('%s: all tensors must live on one device' % who)
        latent = _check_latent(torch.cat([pose[:, 3:], exp, detail.detach()], 1))       # deca.py:167
        uv_z = decode_uv(D_detail, latent)
        verts, _, _ = flame(shape, exp, pose)
        normals = vertex_normals(verts, topo)
        uv_n = detail_normals(layout, uv_z, verts, normals)
        out = render_shape(verts, topo, cam=cam, size=size, images=images, gan_range=gan_range, layout=layout, detail_normals=uv_n,
                           want=('shape', 'shape_detail', 'detail_normal_images'))
        fixed = layout.tables(uv_z.device)[4]
        return {'uv_z': uv_z, 'displacement_map': uv_z + fixed[None, None], 'uv_detail_normals': uv_n, 'shape_images': out['shape'],
                'shape_detail_images': out['shape_detail'], 'detail_normal_images': out['detail_normal_images']}

"""DECA's texture side on the HIP kernels of csrc/texture.hip, csrc/shaperender.hip and csrc/flame.hip: the counterpart of
decalib/models/FLAME.py:216-262 FLAMETex, of the UV texture lines of DECA.decode_deca (deca.py:180-181, 193-199) and of decode_deca as
a whole (deca.py:160-227), with no pytorch3d.

    T = FlameTex(n_tex=50); T.load_state_dict({'texture_mean': ..., 'texture_basis': ...}); T.cuda()      # or FlameTex.from_file(path)
    albedo = T(code['tex'])                                              # [B,3,256,256], the reference's BGR -> RGB flip included
    maps = uv_textures(layout, albedo, uv_detail_normals, code['light'], trans_verts, code['images'])
    opdict, visdict = decode_deca(F, D_detail, layout, code, flametex=T)  # flametex=None: cfg.model.use_tex False

Forward only, no host synchronisation: everything runs on the current stream and captures into a graph (build the weight packs and
the layout's table with one eager call first).  Nothing the caller passes is modified.  The reference adds 10 to the z of trans_verts
in place on each of its three render calls, so the `transformed_vertices` it returns carry z + 30; here they are the projected
vertices themselves.  Kept as the reference has them: `shading_images` is not masked by the coverage, and a texel of `uv_texture_gt`
that no face covers samples the centre of the input image.
"""
import numpy as np
import torch
from torch import nn

from . import _native as N
from .packs import PackedWeights
from .shape_render import _check_map, _check_size, _check_vertices, _forward_only, render_texture, sh_constants

_WANT_UV = ('uv_shading', 'uv_texture', 'uv_texture_gt', 'uv_pverts', 'uv_gt')


def nearest_index(source, size):
    """The source index F.interpolate(mode='nearest') keeps for each of `size` outputs over `source` inputs:
    min(floor(dst * (source / size)), source - 1) with the scale and the product in float32, as torch evaluates them."""
    scale = np.float32(source) / np.float32(size)
    idx = np.floor(np.arange(size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, source - 1)


class FlameTex(PackedWeights, nn.Module):
    """models/FLAME.py FLAMETex: buffers texture_mean [1,1,Hs*Ws*3] and texture_basis [1,Hs*Ws*3,n_tex] under the reference's names, so
    its state dict loads.  forward(texcode [B,n_tex]) -> albedo [B,3,uv_size,uv_size] = the whole source texture mean + basis . code,
    F.interpolate(., [uv_size, uv_size]) (nearest) and channels [2,1,0] -- from a pack that holds the kept texels only."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_flametex_prepack_f32', 'sgdfr_flametex_pack_elems', N.FLAMETEX_PARAMS
    PACK_DTYPE = None               # the folded list holds the two int32 index tables beside the float32 buffers
    WRAP_STATE_DICT = False

    def __init__(self, n_tex=50, source_size=512, uv_size=256):
        for name, v, hi in (('n_tex', n_tex, N.FLAMETEX_MAX_TEX), ('source_size', source_size, N.FLAMETEX_MAX_SOURCE),
                            ('uv_size', uv_size, N.FLAMETEX_MAX_UV)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
                raise RuntimeError('FlameTex: %s must be an int in 1..%d, got %r' % (name, hi, v))
        super().__init__()
        self.n_tex, self.source_size, self.uv_size = n_tex, source_size, uv_size
        n = source_size * source_size * 3
        self.register_buffer('texture_mean', torch.zeros(1, 1, n))
        self.register_buffer('texture_basis', torch.zeros(1, n, n_tex))

    @classmethod
    def from_file(cls, path, n_tex=50, tex_type='BFM', uv_size=256):
        """Reads the texture space the way the reference's constructor does: 'BFM' (FLAME_albedo_from_BFM.npz: MU, PC, 199
        components) or 'FLAME' (mean, tex_dir, 200 components, both / 255)."""
        space = np.load(path)
        if tex_type == 'BFM':
            mean, basis = space['MU'].reshape(1, -1), space['PC'].reshape(-1, 199)
        elif tex_type == 'FLAME':
            mean, basis = space['mean'].reshape(1, -1) / 255.0, space['tex_dir'].reshape(-1, 200) / 255.0
        else:
            raise NotImplementedError('FlameTex: texture type %r does not exist' % (tex_type,))
        side = int(round((mean.shape[1] / 3) ** 0.5))
        self = cls(n_tex, side, uv_size)
        self.load_state_dict({'texture_mean': torch.from_numpy(mean).float()[None],
                              'texture_basis': torch.from_numpy(np.ascontiguousarray(basis[:, :n_tex])).float()[None]})
        return self

    def folded(self):
        """The 4 tensors sgdfr_flametex_prepack_f32 takes: mean, basis, and the source row / column of every output row / column."""
        N.require_device(self.texture_mean, self.texture_basis)
        idx = torch.from_numpy(nearest_index(self.source_size, self.uv_size).astype(np.int32)).to(self.texture_mean.device)
        return [self.texture_mean.detach().reshape(-1).contiguous(), self.texture_basis.detach().reshape(-1, self.n_tex).contiguous(), idx, idx]

    def _prepack_plan(self, ps):
        return self.PARAMS, (self.uv_size, self.n_tex), (self.source_size, self.source_size, self.uv_size, self.n_tex)

    def host_pack(self):
        """The pack's layout written out with torch indexing, on the buffers' device (any device; tests and diagnostics): mean
        [3][uv][uv], then basis [n_tex][3][uv][uv], element (c, y, x) taken from source texel (index[y], index[x]), channel 2 - c."""
        i = torch.from_numpy(nearest_index(self.source_size, self.uv_size)).to(self.texture_mean.device)
        rows = ((i[:, None] * self.source_size + i[None, :]) * 3)[None] + torch.tensor([2, 1, 0], device=i.device)[:, None, None]
        basis = self.texture_basis.detach().reshape(-1, self.n_tex)[rows].permute(3, 0, 1, 2)
        return torch.cat([self.texture_mean.detach().reshape(-1)[rows].reshape(-1), basis.reshape(-1)])

    def unpack(self, pack):
        """(mean [3,uv,uv], basis [n_tex,3,uv,uv]) as views of a pack."""
        P, uv = 3 * self.uv_size * self.uv_size, self.uv_size
        return pack[:P].view(3, uv, uv), pack[P:].view(self.n_tex, 3, uv, uv)

    def forward(self, texcode):
        code = _check_map('FlameTex', 'texcode', texcode, (None, self.n_tex), 'texcode of shape [B,%d]' % self.n_tex)
        if code.shape[0] > 4096:
            raise RuntimeError('FlameTex: unsupported batch of %d rows (1..4096)' % code.shape[0])
        _forward_only('FlameTex', texcode)
        if code.device != self.texture_mean.device:
            raise RuntimeError('FlameTex: texcode lives on %s, the texture space on %s' % (code.device, self.texture_mean.device))
        out = torch.empty((code.shape[0], 3, self.uv_size, self.uv_size), dtype=torch.float32, device=code.device)
        N.call('sgdfr_flametex_forward_f32', N.ptr(code), code.shape[0], N.ptr(self.packed()), self.uv_size, self.n_tex, N.ptr(out), N.stream())
        return out


def _check_uv_args(who, layout, albedo, uv_detail_normals, light, trans_verts, images):
    from .detail import _check_layout
    _check_layout(who, layout)
    _forward_only(who, albedo, uv_detail_normals, light, trans_verts, images)
    tv = _check_vertices(who, 'trans_verts', trans_verts, layout.n_vertices)
    B, S = tv.shape[0], layout.uv_size
    n = _check_map(who, 'uv_detail_normals', uv_detail_normals, (B, 3, S, S))
    a = None if albedo is None else _check_map(who, 'albedo', albedo, (B, 3, S, S))
    l = _check_map(who, 'light', light, (B, 9, 3))
    im = _check_map(who, 'images', images, (B, 3, range(1, 4097), range(1, 4097)), 'images of shape [%d,3,H,W] with sides 1..4096' % B)
    if any(t is not None and t.device != tv.device for t in (n, a, l, im)):
        raise RuntimeError('%s: all tensors must live on one device' % who)
    return tv, n, a, l, im


def uv_textures(layout, albedo, uv_detail_normals, light, trans_verts, images, want=('uv_shading', 'uv_texture', 'uv_texture_gt')):
    """The UV texture pass of DECA.decode_deca (deca.py:180-181, 193-199) in one launch over the UV map.  layout: the detail.UvLayout;
    albedo [B,3,S,S] (None: cfg.model.use_tex False); uv_detail_normals [B,3,S,S]; light [B,9,3]; trans_verts [B,V,3], the projected
    vertices; images [B,3,H,W] -> a dict of what `want` names:

      'uv_shading' = add_SHlight(uv_detail_normals, light);  'uv_texture' = albedo * uv_shading (left out without an albedo);
      'uv_texture_gt' = uv_gt * mask + uv_texture * (1 - mask) * 0.7 with mask = layout.face_eye_mask and, without an albedo, 1 in
        place of uv_texture;  'uv_pverts' = world2uv(trans_verts) [B,3,S,S] and 'uv_gt' = grid_sample(images, uv_pverts.xy), the maps
        in between, written only when named.

    As in the reference, a texel no face covers has uv_pverts (0, 0) and samples the centre of the image."""
    who = 'uv_textures'
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _WANT_UV for w in want):
        raise RuntimeError('%s: want must name at least one of %s, got %r' % (who, _WANT_UV, want))
    tv, n, a, l, im = _check_uv_args(who, layout, albedo, uv_detail_normals, light, trans_verts, images)
    B, S, dev = tv.shape[0], layout.uv_size, tv.device
    faces, pix, bary, mask, _, _ = layout.tables(dev)
    out = {k: torch.empty((B, 3, S, S), dtype=torch.float32, device=dev) for k in _WANT_UV if k in want and (k != 'uv_texture' or a is not None)}
    if not out:
        raise RuntimeError("%s: 'uv_texture' alone needs an albedo" % who)
    N.call('sgdfr_texture_uv_f32', N.ptr(a), N.ptr(n), N.ptr(l), sh_constants(), N.ptr(tv), N.ptr(im), B, layout.n_vertices, im.shape[2], im.shape[3],
           N.ptr(faces), layout.n_faces, N.ptr(pix), N.ptr(bary), N.ptr(mask), S, *[N.ptr(out.get(k)) for k in _WANT_UV], N.stream())
    return out


def orth_proj(points, cam):
    """util.batch_orth_proj with DECA's flip: [B,n,3], cam [B,3] = (s, tx, ty) -> (s (x + tx), -s (y + ty), -s z)."""
    s, tx, ty = cam[:, None, 0:1], cam[:, None, 1:2], cam[:, None, 2:3]
    return torch.cat([s * (points[:, :, 0:1] + tx), -(s * (points[:, :, 1:2] + ty)), -(s * points[:, :, 2:3])], 2)


def decode_deca(flame, D_detail, layout, codedict, flametex=None, size=224):
    """DECA.decode_deca (deca.py:160-227) -> (opdict, visdict) with the reference's keys: for codedict['shape' | 'exp' | 'pose' | 'cam' |
    'detail' | 'light' | 'images'] ('alpha_shp' / 'alpha_exp' are taken too) and, with a FlameTex (cfg.model.use_tex True),
    codedict['tex'].

      opdict:  vertices, normals, transformed_vertices, landmarks2d [B,68,2], landmarks3d [B,68,4] (the visibility of visofp last),
               uv_detail_normals, uv_texture_gt, displacement_map; with flametex also albedo, uv_texture
      visdict: inputs, landmarks2d, landmarks3d, shape_images, shape_detail_images; with flametex also rendered_images

    The reference draws visdict['landmarks2d' / 'landmarks3d'] onto the input images with OpenCV on the host; here they are the
    landmark tensors of opdict, for the caller to draw.  transformed_vertices are the projected vertices (the reference's carry
    z + 30 from its three in-place additions).  Composed of detail.decode_detail (whose two panels are returned bit for bit),
    shape_render.render_texture, flame.visofp and uv_textures; every argument is checked before the first launch."""
    from . import flame as FL
    from .detail import DetailDecoder, _check_layout, decode_detail
    who = 'decode_deca'
    _check_layout(who, layout)
    _check_size(who, size)
    if not isinstance(D_detail, DetailDecoder):
        raise RuntimeError('%s: D_detail must be a DetailDecoder, got %s' % (who, type(D_detail)))
    if flametex is not None and not isinstance(flametex, FlameTex):
        raise RuntimeError('%s: flametex must be a FlameTex or None, got %s' % (who, type(flametex)))
    for k in ('pose', 'cam', 'detail', 'light', 'images') + (('tex',) if flametex is not None else ()):
        if k not in codedict:
            raise RuntimeError('%s: codedict has no %r' % (who, k))
    pick = lambda a, b: codedict[a] if a in codedict else codedict[b]
    _forward_only(who, *[v for v in codedict.values() if torch.is_tensor(v)])
    with torch.no_grad():
        shape, exp, pose, cam = FL._check_coeffs(pick('alpha_shp', 'shape'), pick('alpha_exp', 'exp'), codedict['pose'], codedict['cam'])
        B, dev, Su = pose.shape[0], pose.device, layout.uv_size
        light = _check_map(who, 'light', codedict['light'], (B, 9, 3))
        images = codedict['images']
        if not torch.is_tensor(images) or not images.is_cuda or images.dtype != torch.float32 or images.ndim != 4 or tuple(images.shape[:2]) != (B, 3):
            raise RuntimeError('%s: expected images as a float32 GPU tensor of shape [%d,3,H,W]' % (who, B))
        tex = None
        if flametex is not None:
            tex = _check_map(who, 'tex', codedict['tex'], (B, flametex.n_tex))
            if flametex.uv_size != Su:
                raise RuntimeError('%s: the FlameTex writes %d x %d maps, the layout has uv_size=%d' % (who, flametex.uv_size, flametex.uv_size, Su))
        if any(t is not None and t.device != dev for t in (light, images, tex)):
            raise RuntimeError('%s: all tensors must live on one device' % who)
        det = decode_detail(flame, D_detail, layout, codedict, size=size)           # its own checks come before its first launch
        albedo = None if flametex is None else flametex(tex)
        verts, lm2d, lm3d = flame(shape, exp, pose)
        topo = FL.topology(flame)
        half = size / 2
        landmarks2d = orth_proj(lm2d, cam)[:, :, :2] * half + half
        landmarks3d = orth_proj(lm3d, cam) * half + half
        trans_verts = orth_proj(verts, cam)
        want = ('normals', 'transformed_normals') + (('images',) if flametex is not None else ())
        ops = render_texture(verts, topo, layout, albedo, lights=light, cam=cam, size=size, want=want)
        maps = uv_textures(layout, albedo, det['uv_detail_normals'], light, trans_verts, images,
                           want=('uv_texture_gt',) + (('uv_texture',) if flametex is not None else ()))
        landmarks3d = torch.cat([landmarks3d, FL.visofp(flame, ops['transformed_normals'])], 2)
        opdict = {'vertices': verts, 'normals': ops['normals'], 'transformed_vertices': trans_verts, 'landmarks2d': landmarks2d,
                  'landmarks3d': landmarks3d, 'uv_detail_normals': det['uv_detail_normals'], 'uv_texture_gt': maps['uv_texture_gt'],
                  'displacement_map': det['displacement_map']}
        visdict = {'inputs': images, 'landmarks2d': landmarks2d, 'landmarks3d': landmarks3d, 'shape_images': det['shape_images'],
                   'shape_detail_images': det['shape_detail_images']}
        if flametex is not None:
            opdict['albedo'], opdict['uv_texture'] = albedo, maps['uv_texture']
            visdict['rendered_images'] = ops['images']
        return opdict, visdict

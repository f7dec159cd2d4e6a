"""FLAME decode and the shape / mouth / eye losses on the HIP kernels of csrc/flame.hip: the counterpart of DECA.decode
(libs/DECA/decalib/deca.py:229-239 = models/FLAME.py + models/lbs.py + utils/util.batch_orth_proj) and of the shape-loss block of
libs/utilities/utils_train.py:383-419 with libs/criteria/losses.py.

    F = FLAME.from_files('generic_model.pkl', 'landmark_embedding.npy').cuda()      # or FLAME() + F.load_state_dict(reference_sd)
    vertices, landmarks2d, landmarks3d = F(shape, exp, pose)                        # FLAME.forward
    landmarks2d, landmarks3d, trans_verts = decode(F, codedict)                     # DECA.decode: 224-pixel coordinates
    loss, terms = ShapeLoss(F)(coeff_gt, coeff_reen, lambda_shape, lambda_mouth, lambda_eye)

Everything from the coefficients to the loss and back runs in seven launches (pose, vertices, landmarks, loss, sum; vertex backward,
pose backward) without a host synchronisation, so it captures into a graph; results are bit-identical from call to call.  The
coefficient encoder (DECA's ResNet-50) is deca.py: deca.encode's dict feeds decode / ShapeLoss directly.  The joint regressor is folded into the blend-shape basis on the host in
fp64 (J = J_regressor v_template + (J_regressor shapedirs) betas), once per buffer version; the device pack is rebuilt whenever a
buffer's storage or version changes.
"""
import ctypes
import pickle

import numpy as np
import torch
from torch import nn

from . import _native as N
from .packs import PackedWeights

V, FACES, N_SHAPE, N_EXP, N_POSE_FEATURE, JOINTS, LANDMARKS, DYN_ROWS, DYN_LMK, STATIC_LMK = 5023, 9976, 100, 50, 36, 5, 68, 79, 17, 51
N_CSR = (STATIC_LMK + LANDMARKS + DYN_ROWS * DYN_LMK) * 3
_SMALL, _S_DYN = 256, 201                              # csrc/flame.hip: per-row saved block
_SROW = _SMALL + 2 * 3 * V
PARENTS = (-1, 0, 1, 1, 1)

_BUFFERS = (('faces_tensor', (FACES, 3), torch.long), ('v_template', (V, 3), torch.float32),
            ('shapedirs', (V, 3, N_SHAPE + N_EXP), torch.float32), ('posedirs', (N_POSE_FEATURE, 3 * V), torch.float32),
            ('J_regressor', (JOINTS, V), torch.float32), ('parents', (JOINTS,), torch.long), ('lbs_weights', (V, JOINTS), torch.float32),
            ('lmk_faces_idx', (STATIC_LMK,), torch.long), ('lmk_bary_coords', (STATIC_LMK, 3), torch.float32),
            ('dynamic_lmk_faces_idx', (DYN_ROWS, DYN_LMK), torch.long), ('dynamic_lmk_bary_coords', (DYN_ROWS, DYN_LMK, 3), torch.float32),
            ('full_lmk_faces_idx', (1, LANDMARKS), torch.long), ('full_lmk_bary_coords', (1, LANDMARKS, 3), torch.float32),
            ('neck_kin_chain', (2,), torch.long))


def _to_np(a, dtype):
    if 'scipy.sparse' in str(type(a)):
        a = a.todense()
    return np.array(a, dtype=dtype)


class FLAME(PackedWeights, nn.Module):
    """models/FLAME.py's module at DECA's sizes (n_shape = 100, n_exp = 50): buffers under the reference's names, so its state dict
    loads; forward(shape_params, expression_params, pose_params) -> (vertices [B,5023,3], landmarks2d [B,68,3], landmarks3d [B,68,3])."""
    PREPACK, PACK_ELEMS, PARAMS = 'sgdfr_flame_prepack_f32', 'sgdfr_flame_pack_elems', N.FLAME_PARAMS
    PACK_DTYPE = None               # the folded list mixes int32 index tables with float32: only the device is checked
    WRAP_STATE_DICT = False         # the dict is passed on as it comes (buffers only: no BatchNorm whose loading the wrap changes)
    # no TRAIN_ERROR, no GRAD_ERROR: nothing calls check(); the tables are buffers and the two pose parameters must be zero (folded())

    def __init__(self, n_shape=N_SHAPE, n_exp=N_EXP, n_vertices=V, n_faces=FACES):
        if (n_shape, n_exp, n_vertices, n_faces) != (N_SHAPE, N_EXP, V, FACES):
            raise NotImplementedError('FLAME: the HIP kernels are built for n_shape=%d, n_exp=%d, %d vertices, %d faces (got %r, %r, %r, %r)'
                                      % (N_SHAPE, N_EXP, V, FACES, n_shape, n_exp, n_vertices, n_faces))
        super().__init__()
        for name, shape, dtype in _BUFFERS:
            self.register_buffer(name, torch.zeros(shape, dtype=dtype))
        self.parents.copy_(torch.tensor(PARENTS))
        self.neck_kin_chain.copy_(torch.tensor([1, 0]))
        self.register_parameter('eye_pose', nn.Parameter(torch.zeros(1, 6), requires_grad=False))
        self.register_parameter('neck_pose', nn.Parameter(torch.zeros(1, 3), requires_grad=False))

    @classmethod
    def from_files(cls, flame_model_path, flame_lmk_embedding_path, n_shape=N_SHAPE, n_exp=N_EXP):
        """Reads DECA's generic_model.pkl and landmark_embedding.npy the way the reference's constructor does."""
        with open(flame_model_path, 'rb') as f:
            m = pickle.load(f, encoding='latin1')
        emb = np.load(flame_lmk_embedding_path, allow_pickle=True, encoding='latin1')[()]
        sd = _to_np(m['shapedirs'], np.float32)
        posedirs = _to_np(m['posedirs'], np.float32)
        faces = _to_np(m['f'], np.int64)
        if sd.shape[0] != V or faces.shape[0] != FACES or sd.shape[2] < 300 + n_exp:
            raise NotImplementedError('FLAME: the HIP kernels are built for %d vertices and %d faces (file: shapedirs %s, faces %s)'
                                      % (V, FACES, sd.shape, faces.shape))
        self = cls(n_shape, n_exp, sd.shape[0], faces.shape[0])
        parents = torch.from_numpy(_to_np(m['kintree_table'][0], np.float32)).long()
        parents[0] = -1
        state = {
            'faces_tensor': torch.from_numpy(faces),
            'v_template': torch.from_numpy(_to_np(m['v_template'], np.float32)),
            'shapedirs': torch.from_numpy(np.concatenate([sd[:, :, :n_shape], sd[:, :, 300:300 + n_exp]], 2)),
            'posedirs': torch.from_numpy(np.ascontiguousarray(posedirs.reshape(-1, posedirs.shape[-1]).T)),
            'J_regressor': torch.from_numpy(_to_np(m['J_regressor'], np.float32)),
            'parents': parents,
            'lbs_weights': torch.from_numpy(_to_np(m['weights'], np.float32)),
            'lmk_faces_idx': torch.as_tensor(emb['static_lmk_faces_idx']).long(),
            'lmk_bary_coords': torch.as_tensor(emb['static_lmk_bary_coords']).float(),
            'dynamic_lmk_faces_idx': torch.as_tensor(emb['dynamic_lmk_faces_idx']).long(),
            'dynamic_lmk_bary_coords': torch.as_tensor(emb['dynamic_lmk_bary_coords']).float(),
            'full_lmk_faces_idx': torch.as_tensor(emb['full_lmk_faces_idx']).long(),
            'full_lmk_bary_coords': torch.as_tensor(emb['full_lmk_bary_coords']).float(),
        }
        for k, v in state.items():
            if tuple(v.shape) != tuple(getattr(self, k).shape):
                raise NotImplementedError('FLAME: %s has shape %s in the files, the HIP kernels are built for %s'
                                          % (k, tuple(v.shape), tuple(getattr(self, k).shape)))
        self.load_state_dict(state, strict=False)
        return self

    # ---- tables
    def folded(self):
        """The 15 tensors sgdfr_flame_prepack_f32 takes, on the buffers' device: the joint regressor folded in fp64, landmark faces
        resolved to corner vertices, and the inverse landmark index (per vertex, the landmark corners that reference it)."""
        if float(self.eye_pose.detach().abs().max()) != 0.0 or float(self.neck_pose.detach().abs().max()) != 0.0:
            raise ValueError('FLAME: the HIP kernels assume eye_pose = neck_pose = 0 (the reference freezes both at zero)')
        if tuple(self.parents.tolist()) != PARENTS or tuple(self.neck_kin_chain.tolist()) != (1, 0):
            raise NotImplementedError('FLAME: the HIP kernels are built for parents %r (got %r)' % (PARENTS, tuple(self.parents.tolist())))
        dev = self.v_template.device
        faces = self.faces_tensor.cpu()
        if int(faces.min()) < 0 or int(faces.max()) >= V:
            raise ValueError('FLAME: faces_tensor holds vertex indices outside 0..%d' % (V - 1))
        corner, bary = [], []
        for idx, b in ((self.lmk_faces_idx, self.lmk_bary_coords), (self.full_lmk_faces_idx, self.full_lmk_bary_coords),
                       (self.dynamic_lmk_faces_idx, self.dynamic_lmk_bary_coords)):
            idx = idx.cpu().reshape(-1)
            if int(idx.min()) < 0 or int(idx.max()) >= FACES:
                raise ValueError('FLAME: a landmark table holds face indices outside 0..%d' % (FACES - 1))
            corner.append(faces[idx].to(torch.int32).contiguous())
            bary.append(b.detach().cpu().float().reshape(-1, 3).contiguous())
        # slots: 0..50 static, 51..118 full, 119 + 17 * row + j dynamic; three corners each, grouped by vertex in slot order
        verts = torch.cat(corner).reshape(-1).numpy().astype(np.int64)
        weights = torch.cat(bary).reshape(-1).numpy()
        order = np.argsort(verts, kind='stable')
        offsets = np.zeros(V + 1, dtype=np.int32)
        np.cumsum(np.bincount(verts, minlength=V), out=offsets[1:])
        slots = (order // 3).astype(np.int32)
        sd = self.shapedirs.detach().double().reshape(3 * V, N_SHAPE + N_EXP)
        Jr = self.J_regressor.detach().double()
        jt = (Jr @ self.v_template.detach().double()).reshape(-1)
        jd = torch.einsum('jv,vkl->jkl', Jr, sd.view(V, 3, -1)).reshape(3 * JOINTS, -1)

        def f(t):
            return t.to(device=dev, dtype=torch.float32).contiguous()

        def i32(t):
            return torch.as_tensor(t, dtype=torch.int32).to(dev).contiguous()

        return [f(self.v_template.detach().reshape(-1)), f(sd), f(self.posedirs.detach()), f(self.lbs_weights.detach()), f(jt), f(jd),
                i32(corner[0]), f(bary[0]), i32(corner[1]), f(bary[1]), i32(corner[2]), f(bary[2]),
                i32(offsets), i32(slots), f(torch.from_numpy(weights[order]))]

    def _prepack_plan(self, ps):
        return self.PARAMS, (), (V, N_SHAPE + N_EXP, N_POSE_FEATURE, JOINTS, DYN_ROWS, int(ps[13].numel()))

    def forward(self, shape_params=None, expression_params=None, pose_params=None, eye_pose_params=None):
        if eye_pose_params is not None:
            raise NotImplementedError('FLAME: eye_pose_params has no HIP kernel (the reference never passes it)')
        shape, exp, pose = _check_coeffs(shape_params, expression_params, pose_params)
        lm2d, lm3d, verts = _DecodeFn.apply(shape, exp, pose, None, self.packed(), False, _needs_grad(shape, exp, pose))
        return verts, lm2d, lm3d


def _check_coeffs(shape, exp, pose, cam=None):
    N.require_device(shape, exp, pose, cam)
    rows = shape.shape[0]
    for t, n, what in ((shape, N_SHAPE, 'shape'), (exp, N_EXP, 'exp'), (pose, 6, 'pose'), (cam, 3, 'cam')):
        if t is not None and (t.dim() != 2 or tuple(t.shape) != (rows, n)):
            raise ValueError('FLAME: expected %s of shape [%d,%d], got %s' % (what, rows, n, tuple(t.shape)))
    if rows < 1:
        raise ValueError('FLAME: empty batch')
    out = [N.f32c(shape), N.f32c(exp), N.f32c(pose)]
    return out + [N.f32c(cam)] if cam is not None else out


def _workspace(rows, device):
    return N.workspace('sgdfr_flame_workspace_bytes', device, rows, error='FLAME: unsupported batch of %d rows' % rows)


def _saved(rows, device):
    n = N.size('sgdfr_flame_saved_elems', rows, error='FLAME: unsupported batch of %d rows' % rows)
    return torch.empty(n, dtype=torch.float32, device=device)


def _needs_grad(*tensors):
    """Whether a backward can follow: nothing is kept for a forward under torch.no_grad() or without an input that needs a gradient."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _g(t):
    return None if t is None else t.to(torch.float32).contiguous()


class _DecodeFn(torch.autograd.Function):
    """(landmarks2d, landmarks3d, trans_verts or vertices) on the HIP kernels; backward: dL/dshape, dL/dexp, dL/dpose, dL/dcam."""

    @staticmethod
    def forward(ctx, shape, exp, pose, cam, pack, project, save):
        rows, dev = shape.shape[0], shape.device
        saved = _saved(rows, dev)
        lm2d = torch.empty((rows, LANDMARKS, 2 if project else 3), dtype=torch.float32, device=dev)
        lm3d = torch.empty((rows, LANDMARKS, 3), dtype=torch.float32, device=dev)
        tv = torch.empty((rows, V, 3), dtype=torch.float32, device=dev) if project else None
        N.call('sgdfr_flame_decode_f32', N.ptr(shape), N.ptr(exp), N.ptr(pose), rows, None, None, None, 0, N.ptr(cam), N.ptr(pack),
               int(project), N.ptr(lm2d), N.ptr(lm3d), N.ptr(tv), N.ptr(saved), N.stream())
        if not project:
            tv = saved.view(rows, _SROW)[:, _SMALL + 3 * V:].reshape(rows, V, 3)
        if save:
            ctx.save_for_backward(saved, pack)
        ctx.meta = (rows, bool(project), cam is not None and cam.requires_grad)
        ctx.set_materialize_grads(False)
        return lm2d, lm3d, tv

    @staticmethod
    def backward(ctx, g2, g3, gv):
        saved, pack = ctx.saved_tensors
        rows, project, want_cam = ctx.meta
        dev = saved.device
        g2, g3, gv = _g(g2), _g(g3), _g(gv)
        dshape = torch.empty((rows, N_SHAPE), dtype=torch.float32, device=dev)
        dexp = torch.empty((rows, N_EXP), dtype=torch.float32, device=dev)
        dpose = torch.empty((rows, 6), dtype=torch.float32, device=dev)
        dcam = torch.empty((rows, 3), dtype=torch.float32, device=dev) if want_cam else None
        ws, nbytes = _workspace(rows, dev)
        N.call('sgdfr_flame_decode_backward_f32', N.ptr(g2), N.ptr(g3), N.ptr(gv), None, rows, N.ptr(pack), int(project), N.ptr(saved),
               N.ptr(dshape), N.ptr(dexp), N.ptr(dpose), N.ptr(dcam), N.ptr(ws), nbytes, N.stream())
        return dshape, dexp, dpose, dcam, None, None, None


def dynamic_rows(flame, pose_params):
    """The dynamic contour row (0..78) the decode picks for each pose, as an int32 tensor [B] (diagnostics and tests)."""
    rows = pose_params.shape[0]
    z = torch.zeros((rows, N_SHAPE), dtype=torch.float32, device=pose_params.device)
    shape, exp, pose = _check_coeffs(z, z[:, :N_EXP], pose_params)
    saved = _saved(rows, pose.device)
    lm = torch.empty((2, rows, LANDMARKS, 3), dtype=torch.float32, device=pose.device)
    N.call('sgdfr_flame_decode_f32', N.ptr(shape), N.ptr(exp), N.ptr(pose), rows, None, None, None, 0, None, N.ptr(flame.packed()), 0,
           N.ptr(lm[0]), N.ptr(lm[1]), None, N.ptr(saved), N.stream())
    return saved.view(rows, _SROW)[:, _S_DYN].contiguous().view(torch.int32)


def decode(flame, codedict, image_size=224):
    """DECA.decode / DECA_model.calculate_shape: codedict['shape' | 'exp' | 'pose' | 'cam'] -> (landmarks2d [B,68,2], landmarks3d
    [B,68,3], trans_verts [B,5023,3]) in pixels, differentiable to the four coefficient tensors."""
    if image_size != 224:
        raise NotImplementedError('decode: the HIP kernels project to DECA\'s 224-pixel image (got image_size=%r)' % (image_size,))
    shape, exp, pose, cam = _check_coeffs(codedict['shape'], codedict['exp'], codedict['pose'], codedict['cam'])
    return _DecodeFn.apply(shape, exp, pose, cam, flame.packed(), True, _needs_grad(shape, exp, pose, cam))


def topology(flame):
    """The shape_render.MeshTopology of the module's faces_tensor, built on first use and again when the buffer changes."""
    from .shape_render import MeshTopology
    ft = flame.faces_tensor
    key = (ft.data_ptr(), ft._version, str(ft.device))
    cached = flame.__dict__.get('_topology')
    if cached is None or cached[0] != key:
        cached = flame.__dict__['_topology'] = (key, MeshTopology.from_flame(flame))
    return cached[1]


class LandmarkTable:
    """Landmarks embedded in a triangle mesh, as FLAME's full_lmk_faces_idx / full_lmk_bary_coords are: faces [F,3], per landmark the
    face it lies in [n] and its barycentric weights [n,3].  Resolved on the host to corner vertices; the device copies are made on
    first use.  visofp takes one in place of a FLAME module, for any mesh."""

    def __init__(self, faces, lmk_faces_idx, lmk_bary_coords, n_vertices):
        faces = torch.as_tensor(faces).detach().cpu().long()
        idx = torch.as_tensor(lmk_faces_idx).detach().cpu().long().reshape(-1)
        bary = torch.as_tensor(lmk_bary_coords).detach().cpu().float().reshape(-1, 3)
        if faces.ndim != 2 or faces.shape[1] != 3 or idx.numel() < 1 or bary.shape[0] != idx.numel():
            raise RuntimeError('LandmarkTable: expected faces [F,3], face indices [n] and weights [n,3], got %s, %s, %s'
                               % (tuple(faces.shape), tuple(idx.shape), tuple(bary.shape)))
        if int(idx.min()) < 0 or int(idx.max()) >= faces.shape[0] or int(faces.min()) < 0 or int(faces.max()) >= n_vertices:
            raise RuntimeError('LandmarkTable: a face or vertex index lies outside the mesh')
        self.n, self.n_vertices = int(idx.numel()), int(n_vertices)
        self.corners, self.bary = faces[idx].to(torch.int32).contiguous(), bary.contiguous()
        self._device = {}

    def tables(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = (self.corners.to(device), self.bary.to(device))
        return self._device[key]

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_device'] = {}
        return state


def landmark_table(flame):
    """The LandmarkTable of a FLAME module's 68 full landmarks (seletec_3d68), rebuilt when one of its three buffers changes."""
    ts = (flame.faces_tensor, flame.full_lmk_faces_idx, flame.full_lmk_bary_coords)
    key = tuple((t.data_ptr(), t._version, str(t.device)) for t in ts)
    cached = flame.__dict__.get('_lmk_table')
    if cached is None or cached[0] != key:
        cached = flame.__dict__['_lmk_table'] = (key, LandmarkTable(ts[0], ts[1], ts[2], int(flame.v_template.shape[0])))
    return cached[1]


VISOFP_Z = 0.1                                         # deca.py:147


def visofp(flame, transformed_normals):
    """DECA.visofp (deca.py:143-148): the normals of the projected vertices [B,V,3] gathered at the 68 landmarks of seletec_3d68,
    1 where their z is below 0.1 -> [B,68,1].  flame: a FLAME module, or a LandmarkTable for another mesh.  Forward only."""
    table = flame if isinstance(flame, LandmarkTable) else landmark_table(flame) if isinstance(flame, FLAME) else None
    if table is None:
        raise RuntimeError('visofp: expected a FLAME module or a LandmarkTable, got %s' % type(flame))
    t = transformed_normals
    if not torch.is_tensor(t):
        raise RuntimeError('visofp: transformed_normals must be a tensor, got %s' % type(t))
    N.require_device(t)
    if t.ndim != 3 or t.shape[0] < 1 or tuple(t.shape[1:]) != (table.n_vertices, 3):
        raise RuntimeError('visofp: expected transformed_normals of shape [B,%d,3], got %s' % (table.n_vertices, tuple(t.shape)))
    if torch.is_grad_enabled() and t.requires_grad:
        raise RuntimeError('visofp: forward only (the result is a 0 / 1 mask); call it under torch.no_grad() or on a detached tensor')
    t = N.f32c(t.detach())
    corners, bary = table.tables(t.device)
    vis = torch.empty((t.shape[0], table.n, 1), dtype=torch.float32, device=t.device)
    N.call('sgdfr_flame_visofp_f32', N.ptr(t), t.shape[0], table.n_vertices, N.ptr(corners), N.ptr(bary), table.n, VISOFP_Z, N.ptr(vis), None,
           N.stream())
    return vis


def shape_images(flame, codedict, size=224, images=None, gan_range=False):
    """The `shape_images` of DECA.decode_deca (deca.py:175-187): FLAME forward, the camera projection and SRenderY.render_shape ->
    [B,3,size,size], the grey lit mesh over `images` (None: black).  codedict is what deca.encode / train_step.shape_params return
    ('alpha_shp', 'alpha_exp', 'pose', 'cam') or DECA's own keys ('shape', 'exp', 'pose', 'cam').  Forward only: nothing is kept
    for a backward.  gan_range=True: clamp(., 0, 1) * 2 - 1, a float panel for reenact.video_frames_px."""
    from .shape_render import render_shape
    pick = lambda a, b: codedict[a] if a in codedict else codedict[b]
    with torch.no_grad():
        shape, exp, pose, cam = _check_coeffs(pick('alpha_shp', 'shape'), pick('alpha_exp', 'exp'), codedict['pose'], codedict['cam'])
        verts, _, _ = flame(shape, exp, pose)
        return render_shape(verts, topology(flame), cam=cam, size=size, images=images, gan_range=gan_range)['shape']


def shape_detail_images(flame, D_detail, layout, codedict, size=224, images=None, gan_range=False):
    """The `shape_detail_images` of DECA.decode_deca (deca.py:189): shape_images with the shading normal sampled from the detail normal
    map that D_detail (detail.DetailDecoder) and the layout (detail.UvLayout) give for codedict['detail'] -> [B,3,size,size].
    detail.decode_detail returns both panels and the maps from one pass."""
    from .detail import decode_detail
    return decode_detail(flame, D_detail, layout, codedict, size=size, images=images, gan_range=gan_range)['shape_detail_images']


class _ShapeLossFn(torch.autograd.Function):
    """Both decodes as one batch, the three terms and their cotangents in five launches; backward: two more, for the reenacted set."""

    @staticmethod
    def forward(ctx, shape, exp, pose, shape_gt, exp_gt, pose_gt, cam, pack, lambdas, save):
        rows, dev = shape.shape[0], shape.device
        saved = _saved(2 * rows, dev)
        lm2d = torch.empty((2 * rows, LANDMARKS, 2), dtype=torch.float32, device=dev)
        lm3d = torch.empty((2 * rows, LANDMARKS, 3), dtype=torch.float32, device=dev)
        tv = torch.empty((2 * rows, V, 3), dtype=torch.float32, device=dev)
        N.call('sgdfr_flame_decode_f32', N.ptr(shape_gt), N.ptr(exp_gt), N.ptr(pose_gt), rows, N.ptr(shape), N.ptr(exp), N.ptr(pose), rows,
               N.ptr(cam), N.ptr(pack), 1, N.ptr(lm2d), N.ptr(lm3d), N.ptr(tv), N.ptr(saved), N.stream())
        loss = torch.empty((), dtype=torch.float32, device=dev)
        terms = torch.empty(8, dtype=torch.float32, device=dev)
        g2 = torch.empty((rows, LANDMARKS, 2), dtype=torch.float32, device=dev)
        gv = torch.empty((rows, V, 3), dtype=torch.float32, device=dev)
        ws, nbytes = _workspace(rows, dev)
        N.call('sgdfr_shape_loss_f32', N.ptr(lm2d), N.ptr(tv), rows, lambdas[0], lambdas[1], lambdas[2], N.ptr(loss), N.ptr(terms),
               N.ptr(g2), N.ptr(gv), N.ptr(ws), nbytes, N.stream())
        if save:
            ctx.save_for_backward(saved, pack, g2, gv, ws)
        ctx.rows = rows
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss, terms

    @staticmethod
    def backward(ctx, gloss, _gterms):
        saved, pack, g2, gv, ws = ctx.saved_tensors
        rows, dev = ctx.rows, saved.device
        gloss = gloss.to(torch.float32).contiguous()
        dshape = torch.empty((rows, N_SHAPE), dtype=torch.float32, device=dev)
        dexp = torch.empty((rows, N_EXP), dtype=torch.float32, device=dev)
        dpose = torch.empty((rows, 6), dtype=torch.float32, device=dev)
        N.call('sgdfr_flame_decode_backward_f32', N.ptr(g2), None, N.ptr(gv), N.ptr(gloss), rows, N.ptr(pack), 1,
               ctypes.c_void_p(saved.data_ptr() + 4 * rows * _SROW), N.ptr(dshape), N.ptr(dexp), N.ptr(dpose), None, N.ptr(ws),
               ws.numel() * 4, N.stream())
        return dshape, dexp, dpose, None, None, None, None, None, None, None


class ShapeLoss(nn.Module):
    """The shape-loss block of libs/utilities/utils_train.py:383-419: forward(coeff_gt, coeff_reen, lambda_shape, lambda_mouth,
    lambda_eye) -> (loss, {'loss_shape', 'loss_mouth', 'loss_eye'}), the lambda-weighted terms as 0-d device tensors.  Both sets are
    decoded with cam = (8, 0, 0), as the reference forces it, without touching the callers' `cam`; the ground-truth set is treated as
    detached and gradients reach coeff_reen['shape' | 'exp' | 'pose'] only."""

    def __init__(self, flame):
        super().__init__()
        self.flame = flame
        self._cam = None

    def _fixed_cam(self, rows, device):
        if self._cam is None or self._cam.shape[0] != 2 * rows or self._cam.device != device:
            self._cam = torch.tensor([8.0, 0.0, 0.0], dtype=torch.float32).repeat(2 * rows, 1).to(device)
        return self._cam

    def __getstate__(self):         # ShapeLoss holds no pack (the FLAME module does): this drops its cached camera rows only
        state = self.__dict__.copy()
        state['_cam'] = None
        return state

    def forward(self, coeff_gt, coeff_reen, lambda_shape=1.0, lambda_mouth=1.0, lambda_eye=1.0):
        shape, exp, pose = _check_coeffs(coeff_reen['shape'], coeff_reen['exp'], coeff_reen['pose'])
        sg, eg, pg = _check_coeffs(coeff_gt['shape'].detach(), coeff_gt['exp'].detach(), coeff_gt['pose'].detach())
        if sg.shape[0] != shape.shape[0]:
            raise ValueError('ShapeLoss: %d ground-truth rows against %d reenacted rows' % (sg.shape[0], shape.shape[0]))
        loss, terms = _ShapeLossFn.apply(shape, exp, pose, sg, eg, pg, self._fixed_cam(shape.shape[0], shape.device), self.flame.packed(),
                                         (float(lambda_shape), float(lambda_mouth), float(lambda_eye)), _needs_grad(shape, exp, pose))
        return loss, {'loss_shape': terms[0], 'loss_mouth': terms[1], 'loss_eye': terms[2]}

"""fp64 restatement of DECA.decode (libs/DECA/decalib/deca.py:229-239: models/FLAME.py:175-214, models/lbs.py, utils/util.py:227-237)
and of the shape / mouth / eye terms (libs/criteria/losses.py:20-62) for the FLAME tests: plain torch ops written from the formulas,
in the dtype of the tables it is given, optionally with the decisions forced (the dynamic contour row, the signs of the L1 terms) so
that a gradient check does not depend on an fp32-vs-fp64 flip."""
import math

import torch

MOUTH_PAIRS = [(48, 54), (49, 59), (50, 58), (51, 57), (52, 56), (53, 55), (60, 64), (61, 67), (62, 66), (63, 65)]
EYE_PAIRS = [(36, 39), (37, 41), (38, 40), (42, 45), (43, 47), (44, 46)]


def tables(sd, dtype=torch.float64, device='cpu'):
    return {k: (v.detach().to(device=device, dtype=dtype) if v.is_floating_point() else v.detach().to(device)) for k, v in sd.items()}


def rodrigues(r):
    """lbs.batch_rodrigues as written: the angle is |r + 1e-8|, the direction r / angle."""
    angle = torch.sqrt(((r + 1e-8) ** 2).sum(1, keepdim=True))
    d = r / angle
    z = torch.zeros_like(d[:, 0])
    K = torch.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=r.dtype, device=r.device)
    return eye + torch.sin(angle)[:, :, None] * K + (1 - torch.cos(angle))[:, :, None] * (K @ K)


def dynamic_row(R0):
    """FLAME._find_dynamic_lmk_idx_and_bcoords for a zero neck pose: (row index, y angle in degrees before rounding)."""
    sy = torch.sqrt(R0[:, 0, 0] ** 2 + R0[:, 1, 0] ** 2)
    deg = torch.atan2(-R0[:, 2, 0], sy) * 180.0 / math.pi
    y = torch.round(torch.clamp(deg, max=39)).long()
    y = torch.where(y < 0, torch.where(y < -39, torch.full_like(y, 78), 39 - y), y)
    return y, deg


def _landmarks(verts, corners, bary):
    """verts [B,V,3], corners [B,L,3] vertex indices, bary [B,L,3] -> [B,L,3]."""
    B = verts.shape[0]
    pts = verts[torch.arange(B, device=verts.device)[:, None, None], corners]          # [B,L,3 corners,3]
    return (pts * bary[..., None]).sum(2)


def flame_forward(T, shape, exp, pose, dyn=None):
    """-> dict: vertices, landmarks2d, landmarks3d (un-projected), dyn (row index), deg, v_posed, A."""
    B = shape.shape[0]
    betas = torch.cat([shape, exp], 1)
    zero = torch.zeros(B, 3, dtype=pose.dtype, device=pose.device)
    full_pose = torch.cat([pose[:, :3], zero, pose[:, 3:], zero, zero], 1)
    R = rodrigues(full_pose.reshape(-1, 3)).view(B, 5, 3, 3)
    v_shaped = T['v_template'][None] + torch.einsum('bl,vkl->bvk', betas, T['shapedirs'])
    J = torch.einsum('jv,bvk->bjk', T['J_regressor'], v_shaped)
    eye = torch.eye(3, dtype=pose.dtype, device=pose.device)
    feature = (R[:, 1:] - eye).reshape(B, -1)
    v_posed = v_shaped + (feature @ T['posedirs']).view(B, -1, 3)
    parents = [int(p) for p in T['parents']]
    GR, Gt = [R[:, 0]], [J[:, 0]]
    for j in range(1, 5):
        p = parents[j]
        GR.append(GR[p] @ R[:, j])
        Gt.append((GR[p] @ (J[:, j] - J[:, p])[:, :, None])[:, :, 0] + Gt[p])
    A = torch.stack([torch.cat([GR[j], (Gt[j] - (GR[j] @ J[:, j, :, None])[:, :, 0])[:, :, None]], 2) for j in range(5)], 1)   # [B,5,3,4]
    Tv = torch.einsum('vj,bjkc->bvkc', T['lbs_weights'], A)
    verts = (Tv[..., :3] @ v_posed[..., None])[..., 0] + Tv[..., 3]
    row, deg = dynamic_row(R[:, 0])
    if dyn is not None:
        row = torch.as_tensor(dyn, device=row.device).long()
    faces = T['faces_tensor']
    c2 = torch.cat([faces[T['dynamic_lmk_faces_idx'][row]], faces[T['lmk_faces_idx']][None].expand(B, -1, -1)], 1)
    b2 = torch.cat([T['dynamic_lmk_bary_coords'][row], T['lmk_bary_coords'][None].expand(B, -1, -1)], 1)
    c3 = faces[T['full_lmk_faces_idx'].reshape(-1)][None].expand(B, -1, -1)
    b3 = T['full_lmk_bary_coords'].reshape(-1, 3)[None].expand(B, -1, -1)
    return {'vertices': verts, 'landmarks2d': _landmarks(verts, c2, b2), 'landmarks3d': _landmarks(verts, c3, b3), 'dyn': row, 'deg': deg,
            'v_posed': v_posed, 'A': A}


def project(X, cam, image_size=224):
    """batch_orth_proj, y and z negated, scaled to pixels."""
    cam = cam.view(-1, 1, 3)
    Xt = torch.cat([X[:, :, :2] + cam[:, :, 1:], X[:, :, 2:]], 2) * cam[:, :, 0:1]
    Xt = torch.cat([Xt[:, :, :1], -Xt[:, :, 1:]], 2)
    return Xt * image_size / 2 + image_size / 2


def decode(T, codedict, dyn=None):
    """DECA.decode -> (landmarks2d [B,68,2], landmarks3d [B,68,3], trans_verts [B,V,3], forward dict)."""
    out = flame_forward(T, codedict['shape'], codedict['exp'], codedict['pose'], dyn)
    cam = codedict['cam']
    return project(out['landmarks2d'], cam)[:, :, :2], project(out['landmarks3d'], cam), project(out['vertices'], cam), out


def _l1(a, b, sign=None):
    return (a - b).abs().mean() if sign is None else (sign * (a - b)).mean()


def shape_term(tv_gt, tv_re, sign=None):
    return _l1(tv_gt, tv_re, sign)


def pair_term(l_gt, l_re, pairs, signs=None):
    """Mean over the pairs of the mean L1 between |l[a] - l[b]| of the two sets; signs: per pair (sign of d_gt - d_re, sign of the
    reenacted difference), forcing both decisions."""
    loss = 0
    for i, (a, b) in enumerate(pairs):
        d_gt = (l_gt[:, a] - l_gt[:, b]).abs()
        if signs is None:
            loss = loss + _l1(d_gt, (l_re[:, a] - l_re[:, b]).abs())
        else:
            loss = loss + _l1(d_gt, signs[i][1] * (l_re[:, a] - l_re[:, b]), signs[i][0])
    return loss / len(pairs)


def losses(l2_gt, tv_gt, l2_re, tv_re):
    return shape_term(tv_gt, tv_re), pair_term(l2_gt, l2_re, MOUTH_PAIRS), pair_term(l2_gt, l2_re, EYE_PAIRS)


def fixed_cam(c):
    """The coefficient set with cam = (8, 0, 0), as utils_train.py:392-394, 404-406 force it."""
    cam = torch.zeros_like(c['cam'] if 'cam' in c else c['pose'][:, :3])
    cam[:, 0] = 8
    return {'shape': c['shape'], 'exp': c['exp'], 'pose': c['pose'], 'cam': cam}

"""Stock-PyTorch FLAME decode and shape / mouth / eye terms (plain torch ops, fp32, the tables of flame.FLAME): the comparison leg of
scripts/shape_loss_time.py.  Written from the formulas of DECA.decode (models/FLAME.py:175-214, models/lbs.py, utils/util.py:227-237)
and libs/criteria/losses.py:20-62; not part of the product path."""
import math

import torch
from torch import nn

MOUTH = ((48, 54), (49, 59), (50, 58), (51, 57), (52, 56), (53, 55), (60, 64), (61, 67), (62, 66), (63, 65))
EYES = ((36, 39), (37, 41), (38, 40), (42, 45), (43, 47), (44, 46))


class StockShapeLoss(nn.Module):
    def __init__(self, state):
        super().__init__()
        for k, v in state.items():
            self.register_buffer(k, v.clone())
        self.register_buffer('eye3', torch.eye(3))
        self.register_buffer('sign', torch.tensor([1.0, -1.0, -1.0]))
        for name, pairs in (('mouth', MOUTH), ('eyes', EYES)):
            self.register_buffer(name + '_a', torch.tensor([p[0] for p in pairs]))
            self.register_buffer(name + '_b', torch.tensor([p[1] for p in pairs]))

    def rodrigues(self, r):
        angle = torch.norm(r + 1e-8, dim=1, keepdim=True)
        d = r / angle
        z = torch.zeros_like(d[:, 0])
        K = torch.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).view(-1, 3, 3)
        return self.eye3 + torch.sin(angle)[:, :, None] * K + (1 - torch.cos(angle))[:, :, None] * torch.bmm(K, K)

    def landmarks(self, verts, corners, bary):
        B = verts.shape[0]
        pts = verts[torch.arange(B, device=verts.device)[:, None, None], corners]
        return (pts * bary[..., None]).sum(2)

    def decode(self, shape, exp, pose):
        B = shape.shape[0]
        betas = torch.cat([shape, exp], 1)
        zero = torch.zeros(B, 3, dtype=pose.dtype, device=pose.device)
        R = self.rodrigues(torch.cat([pose[:, :3], zero, pose[:, 3:], zero, zero], 1).reshape(-1, 3)).view(B, 5, 3, 3)
        v_shaped = self.v_template[None] + torch.einsum('bl,vkl->bvk', betas, self.shapedirs)
        J = torch.einsum('jv,bvk->bjk', self.J_regressor, v_shaped)
        v_posed = v_shaped + ((R[:, 1:] - self.eye3).reshape(B, -1) @ self.posedirs).view(B, -1, 3)
        GR, Gt = [R[:, 0]], [J[:, 0]]
        for j, p in ((1, 0), (2, 1), (3, 1), (4, 1)):
            GR.append(GR[p] @ R[:, j])
            Gt.append((GR[p] @ (J[:, j] - J[:, p])[:, :, None])[:, :, 0] + Gt[p])
        A = torch.stack([torch.cat([GR[j], (Gt[j] - (GR[j] @ J[:, j, :, None])[:, :, 0])[:, :, None]], 2) for j in range(5)], 1)
        T = torch.einsum('vj,bjkc->bvkc', self.lbs_weights, A)
        verts = (T[..., :3] @ v_posed[..., None])[..., 0] + T[..., 3]
        R0 = R[:, 0]
        deg = torch.atan2(-R0[:, 2, 0], torch.sqrt(R0[:, 0, 0] ** 2 + R0[:, 1, 0] ** 2)) * 180.0 / math.pi
        y = torch.round(torch.clamp(deg, max=39)).long()
        y = torch.where(y < 0, torch.where(y < -39, torch.full_like(y, 78), 39 - y), y)
        c2 = torch.cat([self.faces_tensor[self.dynamic_lmk_faces_idx[y]], self.faces_tensor[self.lmk_faces_idx][None].expand(B, -1, -1)], 1)
        b2 = torch.cat([self.dynamic_lmk_bary_coords[y], self.lmk_bary_coords[None].expand(B, -1, -1)], 1)
        lm = self.landmarks(verts, c2, b2)
        # cam = (8, 0, 0), y and z negated, 224-pixel image
        return (lm[:, :, :2] * 8.0 * self.sign[:2]) * 112.0 + 112.0, (verts * 8.0 * self.sign) * 112.0 + 112.0

    def pairs(self, lg, lr, a, b):
        return ((lg[:, a] - lg[:, b]).abs() - (lr[:, a] - lr[:, b]).abs()).abs().mean((0, 2)).mean()

    def forward(self, gt, reen, lambda_shape=1.0, lambda_mouth=1.0, lambda_eye=1.0):
        with torch.no_grad():
            lg, tg = self.decode(gt['shape'], gt['exp'], gt['pose'])
        lr, tr = self.decode(reen['shape'], reen['exp'], reen['pose'])
        return (lambda_mouth * self.pairs(lg, lr, self.mouth_a, self.mouth_b) + lambda_shape * (tg - tr).abs().mean()
                + lambda_eye * self.pairs(lg, lr, self.eyes_a, self.eyes_b))

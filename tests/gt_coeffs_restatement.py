"""A torch restatement, on the CPU, of the ground-truth coefficients of the `disentanglement_50` step: what
shift.ShiftVectors.get_params_gt_reenacted computes on the device (csrc/shift.hip gt_reenacted_kernel), written from the direction
table of a ShiftVectors object (host attributes only, no GPU).  Every operation is one torch operation on 0-d tensors of the
inputs' dtype, in the order include/sgdfr.h gives for sgdfr_gt_reenacted_f32, so in float32 the copied, jaw and expression
entries equal the reference's bit for bit and the rotated ones differ from it by the rounding of sin / cos / atan2 only."""
import math

import torch


def euler_deg_to_axis(ang):
    """[3] angles in degrees -> [3] axis-angle: radians, half angles, the Euler quaternion (x, y, z order), then the quaternion's
    axis-angle with both selects (w < 0: atan2 of the negated pair; |v|^2 > 0, else the factor 2)."""
    r = ang * torch.tensor(math.pi, dtype=torch.float32).to(ang.dtype) / 180.0
    x, y, z = r[0] / 2.0, r[1] / 2.0, r[2] / 2.0
    cx, cy, cz, sx, sy, sz = torch.cos(x), torch.cos(y), torch.cos(z), torch.sin(x), torch.sin(y), torch.sin(z)
    q0 = cx * cy * cz - sx * sy * sz
    q1 = cx * sy * sz + cy * cz * sx
    q2 = cx * cz * sy - sx * cy * sz
    q3 = cx * cy * sz + sx * cz * sy
    sin2 = q1 * q1 + q2 * q2 + q3 * q3
    sin_t = torch.sqrt(sin2)
    two_t = 2.0 * (torch.atan2(-sin_t, -q0) if bool(q0 < 0) else torch.atan2(sin_t, q0))
    k = two_t / sin_t if bool(sin2 > 0) else torch.tensor(2.0, dtype=ang.dtype)
    return torch.stack([q1 * k, q2 * k, q3 * k])


def directions(sv):
    """{direction index: (kind, column, a, b)} of the training table, from the attributes ShiftVectors shares with the reference's
    Utilities_train; later entries overwrite earlier ones as in shift._table."""
    table = {}
    for c, d in enumerate((sv.yaw_direction, sv.pitch_direction, sv.roll_direction)):
        if d != -1:
            table[d] = ('angle', c, sv.shift_scale, sv.angle_scales[c])
    table[sv.count_pose - 1] = ('jaw', 3, sv.a_jaw, sv.b_jaw)
    for e in sv.directions_exp:
        table[e['A_direction']] = ('exp', e['exp_component'], e['a'], e['b'])
    return {k: v for k, v in table.items() if 0 <= k < sv.learned_directions}


def gt_reenacted(sv, param_source, param_target, shift_vector, target_indices, angles_source):
    """{'pose', 'exp'} for CPU tensors of one dtype (float32 or float64); the inputs are not modified."""
    pose, exp = param_source['pose'].clone(), param_source['alpha_exp'].clone()
    B = pose.shape[0]
    h = B // 2
    pose[:h], exp[:h] = param_target['pose'][:h], param_target['alpha_exp'][:h]
    table = directions(sv)
    for i in range(h):
        row, ind = h + i, int(target_indices[i])
        if ind not in table:
            continue
        kind, col, a, b = table[ind]
        a, b = float(a), float(b)                      # Python scalars against 0-d tensors: the tensors' dtype is kept
        shift = shift_vector[row, ind]
        if kind == 'angle':
            start = angles_source[row, col] * a / b
            ang = angles_source[row].clone()
            ang[col] = (start + shift) * b / a
            aa = euler_deg_to_axis(ang)
            pose[row, 0], pose[row, 1], pose[row, 2] = aa[1], -aa[0], aa[2]
        else:
            x = param_source['pose'][row, col] if kind == 'jaw' else param_source['alpha_exp'][row, col]
            moved = ((a * x + b + shift) - b) / a
            if kind == 'jaw':
                pose[row, col] = moved
            else:
                exp[row, col] = moved
    return {'pose': pose, 'exp': exp}

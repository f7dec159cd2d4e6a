"""Restatements for the direction sweeps (csrc/sweep.hip, sweep.py), independent of the package's own code:

  plan_ladder / plan_rows   get_direction_info + the two np.arange loops + one_hot (config_directions.py:42-85, visualization.py:46-60)
                            in NumPy / torch on the dtypes the reference's expressions produce; np.arange itself is called
  pool64 / border64 / frame_u8   the f x f mean, add_border and tensor_to_image(...).astype(uint8) of the frames kernel in float64 /
                            in the float32 operation order of image_utils.py:97-110
"""
import numpy as np
import torch

ANGLE, JAW, EXP = 1, 2, 3          # SGDFR_DIR_*
BORDER = 3                          # image_utils.py:130


def plan_ladder(kind, x, a, b, shift_scale, shifts_count):
    """(start, min_shift, max_shift, step, lo values, hi values) of one source value x along one direction.
    kind ANGLE: a = shift_scale, b = angle_scales[col]; JAW / EXP: the line a * x + b."""
    if kind == ANGLE:
        start = np.asarray(np.float32(x)) * shift_scale / np.float64(b)     # 0-d float32 array * Python number, / float64 element
    else:
        start = (float(a) * torch.tensor(x, dtype=torch.float32) + float(b)).numpy()      # float32 0-d array
    min_shift = (-shift_scale - start)
    max_shift = (shift_scale - start) + 1e-5
    step = shift_scale / shifts_count
    return start, min_shift, max_shift, step, np.arange(min_shift, start, step), np.arange(start, max_shift, step)


def table_of(shifts):
    """[(kind, col, a, b)] per direction index from a shift.ShiftVectors' public attributes, the way get_direction_info reads them."""
    D, out = shifts.learned_directions, {}
    for c, d in enumerate((shifts.yaw_direction, shifts.pitch_direction, shifts.roll_direction)):
        if d != -1:
            out[int(d)] = (ANGLE, c, shifts.shift_scale, float(shifts.angle_scales[c]))
    for k in range(D):
        if k in out:
            continue
        if k == shifts.count_pose - 1:
            out[k] = (JAW, 3, shifts.a_jaw, shifts.b_jaw)
        else:
            e = next(e for e in shifts.directions_exp if e['A_direction'] == k)
            out[k] = (EXP, e['exp_component'], e['a'], e['b'])
    return [out[k] for k in range(D)]


def plan_rows(table, ang, pose, exp, shift_scale, shifts_count):
    """Records and one-hot rows for every (source row, direction), in the fixture's layout and order."""
    N, D = ang.shape[0], len(table)
    rec = {f: np.zeros((N, D), dtype=np.float64) for f in ('start', 'min', 'max')}
    n_lo, n_hi = np.zeros((N, D), dtype=np.int32), np.zeros((N, D), dtype=np.int32)
    rows, row_k, is_start = [], [], []
    for n in range(N):
        for k, (kind, col, a, b) in enumerate(table):
            x = ang[n, col] if kind == ANGLE else (pose[n, col] if kind == JAW else exp[n, col])
            start, mn, mx, step, lo, hi = plan_ladder(kind, x, a, b, shift_scale, shifts_count)
            rec['start'][n, k], rec['min'][n, k], rec['max'][n, k] = float(start), float(mn), float(mx)
            n_lo[n, k], n_hi[n, k] = len(lo), len(hi)
            for j, v in enumerate(list(lo) + list(hi)):
                vec = torch.zeros(D)
                vec[k] = v                                              # one_hot: the value is stored into a float32 tensor
                rows.append(vec.numpy())
                row_k.append(k)
                is_start.append(1 if j == len(lo) else 0)
    rows = np.stack(rows) if rows else np.zeros((0, D), dtype=np.float32)
    return rec, step, n_lo, n_hi, rows, np.array(row_k, dtype=np.int32), np.array(is_start, dtype=np.int32)


def pool64(x, f):
    """[R,3,P*f,P*f] -> the f x f mean in float64 (AdaptiveAvgPool2d((P,P)) for an integer factor)."""
    x = np.asarray(x, dtype=np.float64)
    R, C, H, W = x.shape
    return x.reshape(R, C, H // f, f, W // f, f).mean(axis=(3, 5))


def border64(pooled, is_start):
    """add_border (image_utils.py:129-137) on the flagged rows: 3 pixels, R = 1, G = B = -1."""
    out = np.array(pooled, copy=True)
    for r in np.nonzero(np.asarray(is_start))[0]:
        for ch in range(3):
            color = 1.0 if ch == 0 else -1.0
            out[r, ch, :BORDER, :] = color
            out[r, ch, -BORDER:, :] = color
            out[r, ch, :, :BORDER] = color
            out[r, ch, :, -BORDER:] = color
    return out


def border_mask(P):
    m = np.zeros((P, P), dtype=bool)
    m[:BORDER], m[-BORDER:], m[:, :BORDER], m[:, -BORDER:] = True, True, True, True
    return m


def frame_u8(images):
    """tensor_to_image(...).astype(uint8) (image_utils.py:97-110) for a float32 batch [R,3,H,W] -> [R,H,W,3] uint8."""
    t = torch.as_tensor(np.asarray(images, dtype=np.float32)).clone()
    t.clamp_(min=-1, max=1)
    t.add_(1).div_(1 - (-1) + 1e-5)
    t = t.mul(255.0).add(0.0)
    return np.transpose(t.numpy(), (0, 2, 3, 1)).astype(np.uint8)


def frames_u8(pooled, src=None):
    """The gif frames [R,P,Kp*P,3]: the source in the left panel when given (run_facial_editing.py:198-203)."""
    right = frame_u8(pooled)
    if src is None:
        return right
    left = frame_u8(src)
    if left.shape[0] == 1:
        left = np.repeat(left, right.shape[0], axis=0)
    return np.concatenate([left, right], axis=2)

"""Direction sweeps on the GPU: facial editing ladders and interpolation charts.

Counterparts, same names and argument order where the reference has a function:
  * ``DirectionSweep.plan``            libs/configs/config_directions.py:42-85   get_direction_info, all directions in one launch
  * ``DirectionSweep.run``             run_facial_editing.py:144-207            get_shifted_image + interpolate
  * ``edit_image``                     run_facial_editing.py:246-250            the per-file loop body of run_editing after inversion
  * ``make_interpolation_chart``       libs/utilities/visualization.py:13-73    (Utilities_train.log_interpolation calls it)
  * ``extract_statistics``             extract_statistics.py:81-109             the statistics behind ranges_*.npy

The reference walks a direction as a chain of B=1 generator calls, each behind a host-built ``one_hot`` vector and an upload, with the
direction's start pulled to the host by ``.detach().cpu().numpy()``: 21+ frames per direction, up to 15 directions, ~300 blocking
B=1 forwards per source.  Every frame depends only on the fixed source code and its own one-hot shift, so the frames are rows of one
batch (the argument reenact.py makes for run_inference.py:170-181).  A run here is: one launch for all ladders' records
(``sgdfr_sweep_plan_f32``), ONE device->host copy of those [K] records -- the run's only synchronisation: the row count sizes the
batch, and the names and printed numbers need them --, one launch for the [R, D] one-hot rows (``sgdfr_sweep_rows_f32``), the rows
rendered in chunks through ``ReenactmentSession`` (verified no-grad forwards, as generate_image gives), and one
``sgdfr_sweep_frames_f32`` launch per chunk for the 1024 -> 256 pooling, the red border of the start frame and the uint8 gif frames.

The ladder arithmetic (the two np.arange loops included) reproduces the reference's mixed NumPy / torch dtypes operation by operation
and equals fixtures captured from the real functions bit for bit, lengths and values (csrc/sweep.hip, tests/golden/kat20_sweeps.npz;
NumPy >= 2 scalar rules).  Writing PNG / GIF files stays with the caller.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from . import generic
from . import shift as SH
from .reenact import ReenactmentSession

FAILED_ANGLE = -180.0                           # estimate_DECA.py:48-51: the angles of a row the detector failed on
RECORD = np.dtype([('start', '<f8'), ('min_shift', '<f8'), ('max_shift', '<f8'), ('step', '<f8'), ('n_lo', '<i4'), ('n_hi', '<i4')])
MAX_LADDER = 1 << 20                            # csrc/sweep.hip kSweepMaxLen
ANGLE_NAMES = ('yaw', 'pitch', 'roll')
assert RECORD.itemsize == ctypes.sizeof(N.SweepRecord) == 40


def direction_table(learned_directions, shift_scale, angle_scales, angle_directions, count_pose, a_jaw, b_jaw, directions_exp):
    """The by-value direction table from the pieces get_direction_info takes, with its precedence: an angle's row first, then the
    jaw at count_pose - 1, then the expressions."""
    exps = [(e['A_direction'], N.DIR_EXP, e['exp_component'], e['a'], e['b']) for e in directions_exp]
    pose = [(int(d), N.DIR_ANGLE, c, shift_scale, angle_scales[c]) for c, d in reversed(list(enumerate(angle_directions))) if d != -1]
    return SH._table(exps + [(count_pose - 1, N.DIR_JAW, 3, a_jaw, b_jaw)] + pose, int(learned_directions))


def direction_types(table, D):
    """'yaw' / 'pitch' / 'roll' / 'jaw' / 'exp_%02d' per direction index (None where nothing drives it)."""
    out = []
    for k in range(D):
        e = table[k]
        out.append(ANGLE_NAMES[e.col] if e.kind == N.DIR_ANGLE else 'jaw' if e.kind == N.DIR_JAW else
                   'exp_{:02d}'.format(e.col) if e.kind == N.DIR_EXP else None)
    return out


class _Tables:
    """What DirectionSweep reads of a shift.ShiftVectors, built from get_direction_info's own arguments."""

    def __init__(self, learned_directions, shift_scale, angle_scales, angle_directions, count_pose, a_jaw, b_jaw, directions_exp):
        self.learned_directions, self.shift_scale = int(learned_directions), shift_scale
        self._table_train = direction_table(learned_directions, shift_scale, angle_scales, angle_directions, count_pose, a_jaw, b_jaw,
                                            directions_exp)


def _dirs(directions, D):
    ks = [int(k) for k in (directions.tolist() if hasattr(directions, 'tolist') else directions)]
    if not 1 <= len(ks) <= N.MAX_DIRECTIONS:
        raise RuntimeError('sweep: 1..%d directions per call, got %d' % (N.MAX_DIRECTIONS, len(ks)))
    return ks, (ctypes.c_int * len(ks))(*ks)


def pool_frames(x, P=None, is_start=None, source_img=None, want=('images',), out=None):
    """One ``sgdfr_sweep_frames_f32`` pass over rendered rows x [R,3,S,S] (S = P*f, f in 1, 2, 4; P defaults to 256, or S below that):
    {'images': f x f mean [R,3,P,P] float32, 'bordered': the same with add_border on the rows flagged in is_start (int32 [R]),
    'frames': [R,P,P or 2P,3] uint8, the source in the left panel when source_img [1 or R,3,P,P] is given} for the names in `want`.
    `out`: a dict of preallocated tensors to write into (row slices of a run's outputs)."""
    N.require_device(x)
    x = N.f32c(x)
    if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise RuntimeError('pool_frames: expected square RGB images [R,3,S,S], got %s' % (tuple(x.shape),))
    R, S = x.shape[0], x.shape[2]
    if P is None:
        P = min(S, 256)
    f = S // P if P > 0 and S % P == 0 else 0
    unknown = set(want) - {'images', 'bordered', 'frames'}
    if unknown:
        raise RuntimeError('pool_frames: unknown outputs %s' % sorted(unknown))
    src, stride, panels = None, 0, 1
    if source_img is not None and 'frames' in want:
        N.require_device(source_img)
        src = N.f32c(source_img if source_img.ndim == 4 else source_img.unsqueeze(0))
        if tuple(src.shape[1:]) != (3, P, P) or src.shape[0] not in (1, R):
            raise RuntimeError('pool_frames: the source panel must be [1 or %d,3,%d,%d], got %s' % (R, P, P, tuple(src.shape)))
        stride, panels = (0 if (src.shape[0] == 1 and R != 1) else 3 * P * P), 2
    flags = None
    if 'bordered' in want:
        if is_start is None:
            raise RuntimeError('pool_frames: the bordered output needs the is_start flags')
        N.require_device(is_start, dtype=torch.int32)
        flags = N.f32c(is_start)
        if flags.numel() != R:
            raise RuntimeError('pool_frames: %d is_start flags for %d rows' % (flags.numel(), R))
    shapes = {'images': ((R, 3, P, P), torch.float32), 'bordered': ((R, 3, P, P), torch.float32),
              'frames': ((R, P, panels * P, 3), torch.uint8)}
    res = {}
    for name in want:
        shape, dtype = shapes[name]
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, device=x.device, dtype=dtype)
        elif tuple(t.shape) != shape or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError('pool_frames: out[%r] must be a contiguous %s device tensor of shape %s' % (name, dtype, shape))
        res[name] = t
    N.call('sgdfr_sweep_frames_f32', N.ptr(x), R, P, f, N.ptr(flags), N.ptr(src), stride, N.ptr(res.get('images')),
           N.ptr(res.get('bordered')), N.ptr(res.get('frames')), panels, N.stream())
    return res


class SweepResult:
    """What a run leaves: per requested direction j its name `types[j]`, its rows `slices[j]` (a slice into the row dimension of every
    tensor here, empty for an empty ladder), `start[j]` / `min_shift[j]` / `max_shift[j]` / `step` as get_direction_info returns them,
    `n_lo[j]` / `n_hi[j]` (the lengths of the two loops); `rows` [R,D] the one-hot shift vectors, `row_k` [R] (position in
    `directions`), `is_start` [R]; `images` [R,3,P,P] float32 (pooled), `bordered` (red box on each direction's start frame, what
    save_images writes), `frames` [R,P,P or 2P,3] uint8 (the gif frames, never bordered) -- those that were asked for."""

    def __init__(self, **kw):
        self.images = self.bordered = self.frames = None
        self.__dict__.update(kw)

    def __len__(self):
        return len(self.types)


class DirectionSweep:
    def __init__(self, G, A, shifts, truncation=0.7, trunc=None, w_plus=True, num_layers_shift=8, batch=32):
        """shifts: a shift.ShiftVectors (the direction tables of the dataset).  truncation / trunc / w_plus / num_layers_shift are
        what get_shifted_image hands to generate_image; batch: rows per generator call."""
        if truncation < 1 and trunc is None:
            raise RuntimeError('truncation < 1 needs the truncation latent')
        if bool(w_plus) != bool(A.w_plus) or (not w_plus and A.num_layers != num_layers_shift):
            raise RuntimeError('DirectionSweep: w_plus=%s / num_layers_shift=%d do not describe this DirectionMatrix (w_plus=%s, %d layers)'
                               % (w_plus, num_layers_shift, A.w_plus, A.num_layers))
        if A.input_dim != shifts.learned_directions:
            raise RuntimeError('DirectionSweep: the DirectionMatrix takes %d directions, the tables hold %d'
                               % (A.input_dim, shifts.learned_directions))
        self.G, self.A, self.shifts = G, A, shifts
        self.truncation, self.trunc, self.w_plus, self.num_layers_shift, self.batch = truncation, trunc, w_plus, num_layers_shift, int(batch)
        self.types_all = direction_types(shifts._table_train, shifts.learned_directions)

    # ------------------------------------------------------------------ launches
    def plan(self, params_source, angles_source, directions, shifts_count=10):
        """Device records of every (source row, direction): a float64 tensor [N, K, 5] whose bytes are struct sgdfr_sweep_record
        (start, min_shift, max_shift, step, then n_lo and n_hi as two int32 in the fifth word); `records_to_host` decodes it."""
        ang = SH._dev(angles_source)
        pose, exp = SH._dev(params_source['pose'], ang), SH._dev(params_source['alpha_exp'], ang)
        n = ang.shape[0]
        if ang.ndim != 2 or ang.shape[1] != 3 or pose.ndim != 2 or exp.ndim != 2 or pose.shape[0] != n or exp.shape[0] != n:
            raise RuntimeError('sweep plan: angles %s / pose %s / alpha_exp %s do not describe %d sources'
                               % (tuple(ang.shape), tuple(pose.shape), tuple(exp.shape), n))
        D = self.shifts.learned_directions
        ks, arr = _dirs(directions, D)
        rec = torch.empty(n, len(ks), 5, device=ang.device, dtype=torch.float64)
        N.call('sgdfr_sweep_plan_f32', N.ptr(ang), N.ptr(pose), N.ptr(exp), pose.shape[1], exp.shape[1], self.shifts._table_train, D,
               arr, len(ks), float(self.shifts.shift_scale), int(shifts_count), N.ptr(rec), n, N.stream())
        return rec

    @staticmethod
    def records_to_host(records):
        """The one device->host copy: a NumPy record array [N, K] with fields start, min_shift, max_shift, step, n_lo, n_hi."""
        host = records.cpu().numpy()
        return host.view(RECORD).reshape(host.shape[:2])

    def rows(self, records, directions, total):
        """(rows [R,D] float32, row_k [R] int32, is_start [R] int32) for device records [N,K,5]; total = R, the sum of all lengths."""
        n, K = records.shape[0], records.shape[1]
        D = self.shifts.learned_directions
        ks, arr = _dirs(directions, D)
        if K != len(ks):
            raise RuntimeError('sweep rows: %d directions for records of %d' % (len(ks), K))
        dev = records.device
        lens = records.view(torch.int32).view(n * K, 10)[:, 8:10].sum(1, dtype=torch.int32)
        offset = (torch.cumsum(lens, 0, dtype=torch.int32) - lens).contiguous()
        rows = torch.empty(total, D, device=dev, dtype=torch.float32)
        row_k = torch.empty(total, device=dev, dtype=torch.int32)
        is_start = torch.empty(total, device=dev, dtype=torch.int32)
        N.call('sgdfr_sweep_rows_f32', N.ptr(records), N.ptr(offset), self.shifts._table_train, D, arr, K, n, N.ptr(rows), N.ptr(row_k),
               N.ptr(is_start), int(total), N.stream())
        return rows, row_k, is_start

    def _source_latent(self, G, source_code, input_is_latent):
        N.require_device(source_code)
        w = source_code if input_is_latent else G.get_latent(source_code if source_code.ndim == 2 else source_code.reshape(-1, source_code.shape[-1]))
        if w.ndim == 2 and w.shape[0] == G.n_latent and input_is_latent and G.n_latent != 1:
            w = w.unsqueeze(0)                                            # one W+ code without its batch dimension
        if w.ndim == 2:
            if w.shape[0] != 1:
                raise RuntimeError('sweep: one source per run, got %d codes' % w.shape[0])
            w = w.unsqueeze(1).expand(1, G.n_latent, w.shape[-1])         # W -> W+, as get_shifted_latent_code broadcasts it
        if w.ndim != 3 or w.shape[0] != 1 or w.shape[1] != G.n_latent:
            raise RuntimeError('sweep: the source must be one z / W code [1,512] or one W+ code [1,%d,512], got %s'
                               % (G.n_latent, tuple(source_code.shape)))
        return w.contiguous()

    @torch.no_grad()
    def run(self, source_code, directions, params_source, angles_source, input_is_latent=True, shifts_count=10, source_img=None,
            want=('images', 'frames'), G=None, pool_to=None):
        """Every requested direction's ladder of the one source, rendered: see the module docstring for the steps and SweepResult for
        what comes back.  params_source / angles_source: the source's 3DMM parameters (row 0 is used, as the reference reads it).
        source_img [1,3,P,P]: shown in the left panel of the gif frames (draw_original).  G: another generator for this run (the
        PTI-tuned G_copy of run_editing).  pool_to: the side P of the outputs (default 256, or the generator's size below that)."""
        G = self.G if G is None else G
        first = lambda v: v[0:1]
        rec = self.plan({'pose': first(params_source['pose']), 'alpha_exp': first(params_source['alpha_exp'])}, first(angles_source),
                        directions, shifts_count)
        host = self.records_to_host(rec)[0]                              # the run's one synchronisation
        ks, _ = _dirs(directions, self.shifts.learned_directions)
        lens = host['n_lo'].astype(np.int64) + host['n_hi']
        if (host['n_lo'] > MAX_LADDER).any() or (host['n_hi'] > MAX_LADDER).any():
            raise RuntimeError('sweep: a ladder of more than %d rows (non-finite parameters?)' % MAX_LADDER)
        ends = np.cumsum(lens)
        total = int(ends[-1])
        slices = [slice(int(e - n), int(e)) for e, n in zip(ends, lens)]
        rows, row_k, is_start = self.rows(rec, directions, total)
        P = pool_to if pool_to is not None else min(G.size, 256)
        res = SweepResult(directions=ks, types=[self.types_all[k] for k in ks], slices=slices, start=host['start'].copy(),
                          min_shift=host['min_shift'].copy(), max_shift=host['max_shift'].copy(), step=float(host['step'][0]),
                          n_lo=host['n_lo'].copy(), n_hi=host['n_hi'].copy(), rows=rows, row_k=row_k, is_start=is_start, records=rec)
        want = tuple(want)
        names = {'images': 'images', 'bordered': 'bordered', 'frames': 'frames'}
        if set(want) - set(names):
            raise RuntimeError('sweep: unknown outputs %s' % sorted(set(want) - set(names)))
        panels = 2 if source_img is not None else 1
        dev = rows.device
        outs = {}
        for name in want:
            outs[name] = (torch.empty(total, P, panels * P, 3, device=dev, dtype=torch.uint8) if name == 'frames'
                          else torch.empty(total, 3, P, P, device=dev, dtype=torch.float32))
        if total and want:
            sess = ReenactmentSession(G, self.A, self._source_latent(G, source_code, input_is_latent), self.truncation, self.trunc,
                                      batch=self.batch)
            lo = 0
            for img in sess.frames(rows):
                b = img.shape[0]
                pool_frames(img, P, is_start[lo:lo + b], source_img, want, out={k: v[lo:lo + b] for k, v in outs.items()})
                lo += b
        for name in want:
            setattr(res, name, outs[name])
        return res


def _torch_range_1_to_255(image):
    """libs/utilities/image_utils.py:87-94."""
    return image.clamp(-1, 1).add(1).div(1 - (-1) + 1e-5).mul(255.0)


def shape_model_fn(shape_model):
    """images -> (params, angles) from either a callable that already is one (e.g. a closure over train_step.shape_params) or an object
    with extract_DECA_params, used as generic.calculate_shapemodel (libs/utilities/generic.py:22-34) uses it."""
    if hasattr(shape_model, 'extract_DECA_params'):
        def fn(images):
            p, shp, exp, angles, cam = shape_model.extract_DECA_params(_torch_range_1_to_255(images))
            return {'pose': p, 'alpha_exp': exp, 'alpha_shp': shp, 'cam': cam}, angles.to(images.device)
        return fn
    if not callable(shape_model):
        raise RuntimeError('shape_model must be a callable images -> (params, angles) or have extract_DECA_params')
    return shape_model


@torch.no_grad()
def make_interpolation_chart(G, A_matrix, shape_model, z, directions_exp, angle_scales, angle_directions, info, max_directions=None):
    """libs/utilities/visualization.py:13-73 with its signature and return value: (grids, types), grids[i] the list of uint8 HWC numpy
    frames of direction i, types[i] its name.  One sweep for all directions, one host copy for all frames."""
    learned_dims = info['learned_dims']
    truncation = 0.7
    trunc = G.mean_latent(4096).detach().clone()
    tables = _Tables(learned_dims, info['shift_scale'], angle_scales, angle_directions, info['count_pose'], info['a_jaw'], info['b_jaw'],
                     directions_exp)
    if max_directions is not None and learned_dims > max_directions:
        learned_dims = max_directions
    original_img = generic.generate_image(G, z, truncation, trunc, info['w_plus'], input_is_latent=info['input_is_latent'],
                                          num_layers_shift=info['num_layers_shift'], return_latents=False)
    params_original, angles_original = shape_model_fn(shape_model)(original_img)
    if learned_dims < 1:
        return [], []
    sweep = DirectionSweep(G, A_matrix, tables, truncation, trunc, info['w_plus'], info['num_layers_shift'])
    res = sweep.run(z, range(learned_dims), params_original, angles_original, input_is_latent=info['input_is_latent'],
                    shifts_count=info['shifts_count'], want=('frames',))
    frames = res.frames.cpu().numpy()
    return [[frames[r] for r in range(s.start, s.stop)] for s in res.slices], list(res.types)


def edit_image(sweep, source_code, source_img, directions, params_source=None, angles_source=None, shape_model=None, G_copy=None,
               input_is_latent=True, shifts_count=10, draw_red_box=True, draw_original=True, verbose=True):
    """The body of run_editing's per-file loop after inversion / PTI (run_facial_editing.py:246-250): the shape model of the source
    image (unless its params / angles are given), then every direction's interpolate.  Returns the SweepResult: `bordered` (or
    `images` with draw_red_box=False) are the tensors save_image writes as '<type>_<count:03d>.png', `frames[slices[j]]` the frames of
    'gif_<type>_<i:02d>.gif' (fps 15).  G_copy: the generator to render with (the PTI-tuned copy); default the sweep's own."""
    if params_source is None or angles_source is None:
        if shape_model is None:
            raise RuntimeError('edit_image needs the source parameters or a shape model')
        with torch.no_grad():
            params_source, angles_source = shape_model_fn(shape_model)(source_img)
    want = ('bordered' if draw_red_box else 'images', 'frames')
    res = sweep.run(source_code, directions, params_source, angles_source, input_is_latent=input_is_latent, shifts_count=shifts_count,
                    source_img=source_img if draw_original else None, want=want, G=G_copy)
    if verbose:
        for j, k in enumerate(res.directions):                          # run_facial_editing.py:169
            print('Direction {}/{}: Start {:.3f} Min shift {:.3f} Max shift {:.3f} {}'.format(
                res.types[j], k, res.start[j], res.min_shift[j], res.max_shift[j], res.step))
    return res


@torch.no_grad()
def extract_statistics(G, shape_fn, num_images, batch=32, truncation=0.7, trunc=None, z=None):
    """extract_statistics.py:81-109 in batches: (statistics [N,54] float64, ranges [54,2] float64, used [N] bool) as NumPy arrays;
    columns yaw, pitch, roll, jaw = pose[:,3], alpha_exp[0:50]; ranges[i] = (min, max) of column i, the layout
    shift.get_direction_ranges loads (np.save it as ranges_<dataset>.npy).  shape_fn: images [b,3,256,256] -> (params, angles)
    (see shape_model_fn).  z [N,512]: the latents to use (default: drawn on the device).

    One deliberate change: a row the detector failed on (angles of -180 and zero coefficients, estimate_DECA.py:48-51) is left out of
    the minima and maxima and reported in `used`; the reference lets such rows set yaw / pitch / roll minima of -180 and pull every
    other minimum to 0.  `statistics` still holds every row."""
    shape_fn = shape_model_fn(shape_fn)
    dev = G.input.input.device
    if z is None:
        z = torch.randn(num_images, G.style_dim, device=dev)
    N.require_device(z)
    if z.ndim != 2 or z.shape[0] != num_images:
        raise RuntimeError('extract_statistics: z must be [%d,%d], got %s' % (num_images, G.style_dim, tuple(z.shape)))
    if truncation < 1 and trunc is None:
        trunc = G.mean_latent(4096).detach().clone()
    stats = []
    for lo in range(0, num_images, batch):
        img = generic_forward(G, z[lo:lo + batch], truncation, trunc)
        if img.shape[2] > 256:
            img = pool_frames(img, 256)['images']
        params, angles = shape_fn(img)
        stats.append(torch.cat([angles[:, :3], params['pose'][:, 3:4], params['alpha_exp'][:, :50]], 1).double())
    stats = torch.cat(stats, 0) if stats else torch.zeros(0, 54, dtype=torch.float64, device=dev)
    used = ~(stats[:, :3] == FAILED_ANGLE).all(1)
    if not bool(used.any()):
        raise RuntimeError('extract_statistics: the shape model found a face in none of the %d images' % num_images)
    inf = torch.full((), float('inf'), dtype=torch.float64, device=dev)
    keep = used.view(-1, 1)
    ranges = torch.stack([torch.where(keep, stats, inf).amin(0), torch.where(keep, stats, -inf).amax(0)], 1)
    return stats.cpu().numpy(), ranges.cpu().numpy(), used.cpu().numpy()


def generic_forward(G, z, truncation, trunc):
    """G([z], truncation=..., truncation_latent=trunc, input_is_latent=False)[0] as extract_statistics.py:85 calls it, verified like
    generic.generate_image's forwards, at the generator's own resolution."""
    extra = {'verify_range': bool(generic.VERIFY_RANGE)} if hasattr(G, 'range_ok') else {}
    return G([z], return_latents=False, truncation=truncation, truncation_latent=trunc, input_is_latent=False, **extra)[0]

"""Batched reenactment driver: the MI355X counterpart of the per-frame loop of the reference's
``run_inference.py:170-181``.

The reference re-renders ONE target frame per generator call:
    shift = A(shift_vector [1,15]) ; generate_image(G, source_code, 0.7, trunc, w_plus, 8, shift_code=shift,
                                                     input_is_latent=True)
Every frame depends only on the fixed source code and its own shift vector, so N frames are exactly N rows of one
batch.  `ReenactmentSession.frames` chunks the shift vectors, broadcasts the source W+ code inside
``sgdfr_latent_prepare_f32`` (shift add + truncation in the same launch) and yields [b,3,H,W] images, optionally
converted on the GPU to the uint8 HWC layout the reference writes (libs/utilities/image_utils.py:97-110).

`Reenactor` is the caller above it: Inference.run_reenactment whole (run_inference.py:157-199), target frames in, video frames out
-- the source side once (`set_source`: crop, e4e, PTI on a copy of G, the source's 3DMM parameters), then per batch of target frames
S3FD, FAN, the alignment crop, DECA, the shift vectors, a stated policy for frames that fail, and the session.
"""
import ctypes
import os

import numpy as np
import torch

from . import _native as N
from . import functional as F_


def images_to_uint8(images):
    """[B,3,H,W] fp32 in [-1,1] -> [B,H,W,3] uint8 with the reference's scaling (image_utils.py:87-110)."""
    N.require_device(images)
    x = N.f32c(images)
    B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError('expected RGB images, got %d channels' % C)
    y = torch.empty(B, H, W, 3, device=x.device, dtype=torch.uint8)
    N.call('sgdfr_image_to_u8_f32', N.ptr(x), N.ptr(y), B, H, W, N.stream())
    return y


def _left_panel(p, B, tail, indexed, bad_shape, bad_rows):
    """One left panel of a frames launch, on the device already: None stays None (skipped: `out` keeps it), [*tail] becomes
    [1,*tail]; the shape behind the rows must be `tail`, the rows 1 (shown in every frame) or B unless the panel is `indexed`.
    bad_shape / bad_rows are the caller's error texts with one %s for the shape found.  -> the contiguous panel."""
    if p is None:
        return None
    p = p if p.ndim == 4 else p.unsqueeze(0)
    if p.ndim != 4 or tuple(p.shape[1:]) != tuple(tail) or p.shape[0] < 1:
        raise RuntimeError(bad_shape % (tuple(p.shape),))
    if not indexed and p.shape[0] not in (1, B):
        raise RuntimeError(bad_rows % (tuple(p.shape),))
    return p.contiguous()


def _float_panel_args(xs, B):
    """The pointer and batch-stride arrays the float entries take for panels checked by _left_panel (NULL = skipped, stride 0 = one
    row shown in every frame)."""
    n = max(len(xs), 1)
    ptrs = (ctypes.c_void_p * n)(*[None if p is None else p.data_ptr() for p in xs])
    strides = (ctypes.c_int64 * n)(*[0 if (p is None or (p.shape[0] == 1 and B > 1)) else p.numel() // p.shape[0] for p in xs])
    return ptrs, strides


def _frames_out(who, out, shape, device, skipped):
    """The uint8 frames tensor [B,H,K*W,3] of a frames launch: `out` checked, or a new one -- which `skipped` panels rule out."""
    if out is None:
        if skipped:
            raise RuntimeError('%s: a skipped panel needs the `out` tensor that already holds it' % who)
        return torch.empty(shape, device=device, dtype=torch.uint8)
    if not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise RuntimeError('%s: out must be a contiguous uint8 [%d,%d,%d,3] device tensor' % ((who,) + tuple(shape[:3])))
    return out


def _square_rgb(who, x, P, default_P=True):
    """x [B,3,S,S] float32 on the device -> (x contiguous, B, P, f): P defaults to 256, or S below that; f = S / P (_pool_factor)."""
    N.require_device(x)
    x = N.f32c(x)
    if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise RuntimeError('%s: expected square RGB images [B,3,S,S], got %s' % (who, tuple(x.shape)))
    if P is None and default_P:
        P = min(x.shape[2], 256)
    return x, x.shape[0], P, _pool_factor(x.shape[2], P)


def grid_frames_uint8(panels, swap_rb=False, out=None):
    """Side-by-side video frames for a batch: panels = list of [B,3,H,W] or [1,3,H,W] (shown in every frame) fp32
    images in [-1,1] -> [B,H,K*W,3] uint8.  One launch for what the reference does per frame with
    generate_grid_image + tensor_to_image + np.uint8 (utils_inference.py:11-33, run_inference.py:188-194);
    swap_rb applies that path's cvtColor channel swap.  A panel given as None is left untouched in `out` (the generator
    already wrote it there: Generator.forward(image_out=U8Target(out, panel)))."""
    if not 1 <= len(panels) <= 4:
        raise RuntimeError('grid_frames_uint8 takes 1..4 panels, got %d' % len(panels))
    given = [x for x in panels if x is not None]
    if not given:
        if out is None:
            raise RuntimeError('grid_frames_uint8: nothing to write')
        return out
    N.require_device(*given)
    H, W = given[0].shape[-2:]
    B = out.shape[0] if out is not None else max(x.shape[0] if x.ndim == 4 else 1 for x in given)
    bad = 'grid panels must be [B or 1,3,%d,%d], got %%s' % (H, W)
    xs = [_left_panel(x, B, (3, H, W), False, bad, bad) for x in panels]
    K = len(xs)
    out = _frames_out('grid_frames_uint8', out, (B, H, K * W, 3), given[0].device, len(given) < K)
    ptrs, strides = _float_panel_args(xs, B)
    N.call('sgdfr_grid_to_u8_f32', ptrs, strides, K, N.ptr(out), B, H, W, int(bool(swap_rb)), N.stream())
    return out


def _pool_factor(size, pool_to):
    """f = size / pool_to for the pooled outputs (1, 2 or 4: what the frames kernels take)."""
    f = size // pool_to if isinstance(pool_to, int) and not isinstance(pool_to, bool) and pool_to > 0 and size % pool_to == 0 else 0
    if f not in (1, 2, 4):
        raise RuntimeError('pool_to must be None or a divisor of the generator size %d that leaves a factor of 1, 2 or 4, got %r'
                           % (size, pool_to))
    return f


def pool_images(x, P, as_uint8=False):
    """x [B,3,P*f,P*f] float32 -> the f x f mean [B,3,P,P] float32, or with as_uint8 its [B,P,P,3] uint8 frames: one
    ``sgdfr_sweep_frames_f32`` launch (AdaptiveAvgPool2d((P,P)) for f = 1, 2, 4, as generic.generate_image pools above 256)."""
    x, B, P, f = _square_rgb('pool_images', x, P, default_P=False)
    y = torch.empty((B, P, P, 3) if as_uint8 else (B, 3, P, P), device=x.device, dtype=torch.uint8 if as_uint8 else torch.float32)
    N.call('sgdfr_sweep_frames_f32', N.ptr(x), B, P, f, None, None, 0, None if as_uint8 else N.ptr(y), None,
           N.ptr(y) if as_uint8 else None, 1, N.stream())
    return y


def video_frames_uint8(x, panels=(), P=None, swap_rb=False, out=None):
    """Rendered rows to grid frames in ONE launch (``sgdfr_video_frames_f32``): x [B,3,P*f,P*f] float32 (f = 1, 2 or 4; P defaults to
    256, or the side of x below that) is pooled f x f and placed to the right of up to three left `panels` ([B or 1,3,P,P] float32;
    None = leave that panel of `out` as it is) -> [B,P,K*P,3] uint8, K = len(panels) + 1.  The bytes are those of
    pool_images(x, P) -> grid_frames_uint8(panels + [pooled]) without the float intermediate."""
    who = 'video_frames_uint8'
    x, B, P, f = _square_rgb(who, x, P)
    if len(panels) > 3:
        raise RuntimeError('%s takes up to 3 left panels, got %d' % (who, len(panels)))
    N.require_device(*panels)
    bad = '%s: left panels must be [1 or %d,3,%d,%d], got %%s' % (who, B, P, P)
    xs = [_left_panel(p, B, (3, P, P), False, bad, bad) for p in panels]
    out = _frames_out(who, out, (B, P, (len(xs) + 1) * P, 3), x.device, any(p is None for p in xs))
    ptrs, strides = _float_panel_args(xs, B)
    N.call('sgdfr_video_frames_f32', N.ptr(x), B, P, f, ptrs, strides, len(xs), N.ptr(out), int(bool(swap_rb)), N.stream())
    return out


def uint8_panel_map():
    """The byte a uint8 panel byte u becomes in a frame, for u = 0..255, as a [256] uint8 CPU tensor: the alignment crop's float
    fl32(u / 255) * 2 - 1 (face_crop.crop_using_landmarks(as_tensor=True)) through images_to_uint8's trunc((v + 1) / (2 + 1e-5) * 255),
    every operation in float32.  Not the identity: the 1e-5 in the divisor pulls u * (1 - 5e-6) below u and truncation then gives
    u - 1 for every u >= 1 (0 stays 0).  ``sgdfr_video_frames_px`` evaluates the two expressions per byte; this table restates them
    for the tests and for callers that want the target panel's bytes without a launch."""
    u = torch.arange(256, dtype=torch.float32)
    v = ((u / 255.0) * 2.0 - 1.0).clamp(-1.0, 1.0)
    den = torch.tensor(2.0, dtype=torch.float32) + torch.tensor(1e-5, dtype=torch.float32)
    return ((v + 1.0) / den * 255.0).to(torch.uint8)


# the byte of the float 0.0 that the alignment crop writes into every pixel of an INVALID row's x: trunc(1 / (2 + 1e-5) * 255)
BLANK_BYTE = 127


def video_frames_px(x, panels, P=None, swap_rb=False, out=None, index=None):
    """video_frames_uint8 with typed, indexed left panels and an optional x, in ONE launch (``sgdfr_video_frames_px``).

    x: [B,3,P*f,P*f] float32 as video_frames_uint8 takes it, or None = leave the last panel of `out` as it is (the generator's last
    ToRGB launch has written it: functional.U8Target).  panels: up to three of None (skipped: `out` keeps it), a float32 table
    [rows,3,P,P] in [-1,1], or a uint8 table [rows,P,P,3] RGB (the crops preprocess_frames returns).  index: None, one int32 device
    tensor [B] for every given panel, or one entry (None or such a tensor) per panel; frame b shows row index[b] of the panel's table,
    clamped into it by the kernel.  Without an index a table has B rows or 1 (shown in every frame).  -> [B,P,K*P,3] uint8,
    K = len(panels) + 1.  A float32 panel gives video_frames_uint8's bytes; a uint8 panel gives the bytes its float crop
    u / 255 * 2 - 1 gives there (uint8_panel_map), which is not the identity."""
    who = 'video_frames_px'
    panels = list(panels)
    if len(panels) > 3:
        raise RuntimeError('%s takes up to 3 left panels, got %d' % (who, len(panels)))
    K = len(panels) + 1
    if x is not None:
        if not torch.is_tensor(x) or x.dtype != torch.float32:
            raise RuntimeError('%s: x must be a float32 device tensor or None, got %s' % (who, x.dtype if torch.is_tensor(x) else type(x)))
        x, B, P, f = _square_rgb(who, x, P)
        device = x.device
    else:
        if out is None or not torch.is_tensor(out) or out.ndim != 4:
            raise RuntimeError('%s: a skipped panel needs the `out` tensor that already holds it (x=None skips the last one)' % who)
        B, f, device = out.shape[0], 1, out.device
        if P is None:
            P = out.shape[1]
    if index is None or torch.is_tensor(index):
        index = [index] * len(panels)
    else:
        index = list(index)
        if len(index) != len(panels):
            raise RuntimeError('%s: %d index entries for %d panels' % (who, len(index), len(panels)))
    descs = (N.VideoPanel * max(len(panels), 1))()
    keep = []                                                               # the tensors behind the descriptors' pointers
    for k, (p, ix) in enumerate(zip(panels, index)):
        if p is None:
            continue
        if not torch.is_tensor(p):
            raise RuntimeError('%s: panel %d must be a tensor or None, got %s' % (who, k, type(p)))
        if p.dtype == torch.uint8:
            kind, tail = N.PANEL_U8, (P, P, 3)
        elif p.dtype == torch.float32:
            kind, tail = N.PANEL_F32, (3, P, P)
        else:
            raise RuntimeError('%s: panel %d must be float32 [rows,3,P,P] or uint8 [rows,P,P,3], got %s' % (who, k, p.dtype))
        if ix is not None and (not torch.is_tensor(ix) or ix.dtype != torch.int32):
            raise RuntimeError('%s: the index of panel %d must be an int32 device tensor [%d], got %s'
                               % (who, k, B, ix.dtype if torch.is_tensor(ix) else type(ix)))
        for t in (p, ix):
            if t is not None and not t.is_cuda:
                raise RuntimeError('expected a GPU (HIP) tensor, got device %s: this package has no CPU path' % t.device)
        p = _left_panel(p, B, tail, ix is not None,
                        '%s: left panels must be [rows,%d,%d,%d] (%s), got %%s' % ((who,) + tail + (str(p.dtype).replace('torch.', ''),)),
                        '%s: left panels without an index must have 1 or %d rows, got %%s' % (who, B))
        if ix is not None:
            if tuple(ix.shape) != (B,) or not ix.is_contiguous():
                raise RuntimeError('%s: the index of panel %d must be a contiguous [%d] tensor, got %s' % (who, k, B, tuple(ix.shape)))
            keep.append(ix)
        keep.append(p)
        descs[k].data, descs[k].index = p.data_ptr(), (None if ix is None else ix.data_ptr())
        descs[k].kind, descs[k].rows = kind, p.shape[0]
    out = _frames_out(who, out, (B, P, K * P, 3), device, any(p is None for p in panels))
    N.call('sgdfr_video_frames_px', N.ptr(x), B, P, f, descs, len(panels), N.ptr(out), int(bool(swap_rb)), N.stream())
    return out


def shape_panels(flame, params, ok=None, size=256, batch=32):
    """The fitted mesh of every analysed frame as a float panel: params = a `TargetAnalysis.params`-shaped dict ('alpha_shp',
    'alpha_exp', 'pose', 'cam', [N,.] each), rendered `batch` rows at a time by flame.shape_images -> [N,3,size,size] float32 in
    [-1,1] (clamp(shape_images, 0, 1) * 2 - 1).  Rows whose `ok` [N] (bool) is False are 0.0 everywhere, which is what the alignment
    crop writes for an invalid row.  Whether DECA tracked the target is answered by looking at the mesh beside the frame:

        a = R.analyse(frames)                                                  # Reenactor
        mesh = shape_panels(flame, a.params, a.ok)                             # [N,3,256,256]
        _, ok, sv = R.reenact_analysed(a, output='images')                     # the shift vectors under the on_fail policy
        x = R.session.render(sv)                                               # the reenacted frames, float32 [N,3,256,256]
        video = video_frames_px(x, [R.source_x, a.crops, mesh])                # source | target | target's mesh | reenacted
    """
    from . import flame as FL
    keys = ('alpha_shp', 'alpha_exp', 'pose', 'cam')
    if not isinstance(params, dict) or any(k not in params or not torch.is_tensor(params[k]) or params[k].ndim != 2 for k in keys):
        raise RuntimeError('shape_panels: params must be a dict with [N,.] tensors under %s' % (keys,))
    n = params['pose'].shape[0]
    if n < 1 or any(params[k].shape[0] != n for k in keys):
        raise RuntimeError('shape_panels: the params describe %s rows' % [params[k].shape[0] for k in keys])
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise RuntimeError('shape_panels: batch must be a positive int, got %r' % (batch,))
    N.require_device(*(params[k] for k in keys))
    if ok is not None:
        if not torch.is_tensor(ok) or ok.dtype != torch.bool or tuple(ok.shape) != (n,) or ok.device != params['pose'].device:
            raise RuntimeError('shape_panels: ok must be a bool tensor [%d] on the params\' device' % n)
    out = torch.empty((n, 3, size, size), dtype=torch.float32, device=params['pose'].device)
    for lo in range(0, n, batch):
        out[lo:lo + batch] = FL.shape_images(flame, {k: params[k][lo:lo + batch] for k in keys}, size=size, gan_range=True)
    if ok is not None:
        out = torch.where(ok.view(n, 1, 1, 1), out, torch.zeros((), dtype=out.dtype, device=out.device))
    return out


def hold_failed_rows_many(sv, ok):
    """hold_failed_rows for S sources at once, each starting from an empty carry: sv [S,N,D], ok [N] (the targets' alone, so the
    row every failed row takes is found once) -> [S,N,D].  Equal to S hold_failed_rows(sv[s], ok, zeros, False) calls bit for bit;
    nothing is carried out.  Plain torch on the tensors' device (CPU tensors too), no host read."""
    n = sv.shape[1]
    if n == 0:
        return sv
    ok = ok.to(torch.bool)
    idx = torch.arange(n, device=sv.device)
    last = torch.cummax(torch.where(ok, idx, torch.full_like(idx, -1)), 0).values
    held = torch.where((last >= 0).view(1, n, 1), sv.index_select(1, last.clamp(min=0)), torch.zeros((), dtype=sv.dtype, device=sv.device))
    return torch.where(ok.view(1, n, 1), sv, held)


def hold_failed_rows(sv, ok, carry, carry_valid):
    """The 'hold' policy for target frames that failed: every row of sv [N,D] whose `ok` [N] (bool) is False takes the vector of the
    nearest earlier ok row; before the first ok row it takes `carry` [D] when `carry_valid` (0-d bool tensor) is set -- the last good
    vector of the calls before this one -- and zeros otherwise (a zero shift vector renders the inverted source).  Rows that are ok
    pass through bit for bit, whatever the failed rows hold (NaNs included).  Returns (sv, carry, carry_valid) with the carry for
    the next call.  Plain torch on the tensors' device (CPU tensors too), no host read."""
    n = sv.shape[0]
    if n == 0:
        return sv, carry, carry_valid
    ok = ok.to(torch.bool)
    idx = torch.arange(n, device=sv.device)
    last = torch.cummax(torch.where(ok, idx, torch.full_like(idx, -1)), 0).values        # nearest ok row at or before each row, or -1
    before = torch.where(carry_valid, carry, torch.zeros_like(carry)).to(sv.dtype)
    held = torch.where((last >= 0).unsqueeze(1), sv.index_select(0, last.clamp(min=0)), before.unsqueeze(0))
    out = torch.where(ok.unsqueeze(1), sv, held)
    return out, out[-1].clone(), carry_valid | ok.any()


def save_latent_codes(directory, names, latents):
    """The reference's W+ latent store: one `<name>.npy` holding a [n_latent,512] fp32 array per frame
    (invert_images.py:119-125).  `latents` [B,n_latent,512] comes back to the host in ONE copy."""
    lat = latents.detach().to('cpu', torch.float32).numpy()
    if lat.ndim != 3 or len(names) != lat.shape[0]:
        raise RuntimeError('save_latent_codes: %d names for latents of shape %s' % (len(names), tuple(lat.shape)))
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name, code in zip(names, lat):
        path = os.path.join(directory, os.path.splitext(name)[0] + '.npy')
        np.save(path, code)
        paths.append(path)
    return paths


@torch.no_grad()
def invert_images(enc, G, images, truncation=1.0, trunc=None, as_uint8=False):
    """The body of the reference's inversion loop (invert_images.py:101-125) as one call: images [B,3,R,R] in [-1,1] -> e4e W+
    codes on the HIP encoder (encoder.encode) -> G([w], input_is_latent=True, truncation=..., truncation_latent=trunc).
    Returns (latent_codes [B,n_latent,512], inverted frames [B,3,H,W] float32, or [B,H,W,3] uint8 with the reference's scaling
    when as_uint8).  Encoder and generator share the caller's stream with no host synchronisation between them; the codes pair
    with `save_latent_codes`."""
    from .encoder import encode
    if truncation < 1 and trunc is None:
        raise RuntimeError('truncation < 1 needs the truncation latent')
    w = encode(enc, images)
    if w.shape[1] != G.n_latent:
        raise RuntimeError('invert_images: the encoder gives %d latents, the generator takes %d' % (w.shape[1], G.n_latent))
    frames, _ = G([w], input_is_latent=True, truncation=truncation, truncation_latent=trunc)
    return w, (images_to_uint8(frames) if as_uint8 else frames)


@torch.no_grad()
def preprocess_frames(det, fan, frames, out_size=256):
    """The body of the reference's preprocess_image (libs/utilities/utils_inference.py:61-82) for a batch, without its
    image_resize(width=1000): frames [B,H,W,3] uint8 on the device -> face_detector.detect_landmarks(rule='last_above_0.99',
    input_range='255') on the float CHW view, as LandmarksEstimation.detect_landmarks is called there -> the alignment crop
    (face_crop.crop_using_landmarks).  Returns (crops [B,S,S,3] uint8, x [B,3,S,S] float32 in [-1,1], ok [B] bool) with
    ok = has_face & valid; x feeds `invert_images` directly.  One stream, no host synchronisation; rows with ok False hold nothing
    of use."""
    crops, x, has_face, valid = _preprocess(det, fan, frames, out_size)
    return crops, x, has_face & valid


def _preprocess(det, fan, frames, out_size=256):
    """preprocess_frames with its two flags apart: (crops, x, has_face [B] bool, valid [B] bool, the crop's own flag)."""
    from . import face_crop
    from .face_detector import detect_landmarks
    face_crop._check_frames(frames)
    images = frames.permute(0, 3, 1, 2).float()
    pts, _, has_face = detect_landmarks(det, fan, images, rule='last_above_0.99', input_range='255')
    (crops, x), valid = face_crop.crop_using_landmarks(frames, pts.contiguous(), out_size=out_size, as_tensor=True)
    return crops, x, has_face, valid != 0


def load_latent_codes(paths, device=None):
    """Read per-frame `.npy` codes back into one [B,n_latent,512] tensor (pinned staging, one H2D copy)."""
    codes = [np.load(p) for p in paths]
    for p, c in zip(paths, codes):
        if c.ndim != 2 or c.shape != codes[0].shape or c.dtype != np.float32:
            raise RuntimeError('latent store %s: expected fp32 %s, got %s %s' % (p, codes[0].shape, c.dtype, c.shape))
    host = torch.from_numpy(np.stack(codes, 0))
    if device is None or torch.device(device).type == 'cpu':
        return host
    return host.pin_memory().to(device, non_blocking=True)


class ReenactmentSession:
    """One source identity, many target poses/expressions."""

    def __init__(self, G, A, source_code, truncation=0.7, trunc=None, batch=32, graph=False, shifts=None, streams=2, pool_to=None):
        """shifts: a `shift.ShiftVectors` (direction tables of the dataset) -- then `render_targets` / `frames_for_targets`
        take the 3DMM parameters of source and targets and build the shift vectors on the device too.
        graph=True captures one `batch`-sized step (DirectionMatrix -> shift -> generator) in a hipGraph the first time a
        full batch is rendered and replays it afterwards: the ~65 launches of a step become one submission, which is what a
        small batch is bound by (B=1: 1.10 -> 0.72 ms per frame).  Weights must not be replaced while the graph is alive
        (call `reset_graph()` after loading new ones); partial last batches run eagerly.
        streams: consecutive chunks alternate between this many HIP streams (functional.StreamPipeline: the latency-bound head
        of chunk i+1 runs beside the big layers of chunk i; 1 = everything on the caller's stream).  Replayed graphs share
        their static buffers and stay on the caller's stream.
        pool_to: the side P of what the session hands back for a generator above it (256 for the 512 and 1024 generators): `frames`,
        `render` and `streaming` give images pooled f x f as generic.generate_image pools them (generic.py:51-52; here the frames
        kernel's mean, pool_images), `video_frames` writes the pooled reenacted panel (video_frames_uint8).  The last ToRGB
        launch's direct uint8 write (functional.U8Target) is bypassed on this path: it has full-size pixels to offer.  None (the
        default): images of the generator's own size, as before."""
        self.pool_to, self.pool_f = None, 1
        if pool_to is not None:
            self.pool_f = _pool_factor(G.size, pool_to)
            self.pool_to = int(pool_to) if self.pool_f > 1 else None
        if source_code.ndim == 2:
            source_code = source_code.unsqueeze(0)
        if source_code.shape[0] != 1 or source_code.shape[1] != G.n_latent:
            raise RuntimeError('source_code must be one W+ code [1,%d,512]' % G.n_latent)
        if truncation < 1 and trunc is None:
            raise RuntimeError('truncation < 1 needs the truncation latent')
        self.G, self.A = G, A
        self.source = source_code.contiguous()
        self.truncation, self.trunc, self.batch = truncation, trunc, batch
        self.use_graph = bool(graph)
        self.shifts = shifts
        self._graph = None          # (hipGraph, static shift-vector input, static image output)
        self.n_streams = max(1, int(streams))
        self.pipeline_min_work = G.GRAPH_MAX_WORK      # batch * (size/256)^2 above which chunks alternate between the streams
        self._pipe = None

    def reset_graph(self):
        self._graph = None

    def _step(self, sv, image_out=None, no_graph=False, prefer_graph=False, verify=False):
        shift = self.A(sv)                                              # [b, L, 512] (w_plus) or [b, 512]
        b = sv.shape[0]
        w = self.source.expand(b, -1, -1).contiguous()
        layers = shift.shape[1] if shift.ndim == 3 else self.A.num_layers
        latent = F_.latent_prepare(w, self.G.n_latent, shift=shift, shift_layers=layers)
        # (a session with graph=True captures the whole step itself -- DirectionMatrix and latent shift included -- so the
        # generator's own per-forward graphs stay out of it)
        # (verify_range=False: the session checks every chunk's RangeToken itself, one chunk behind the launches; verify: the
        #  second rendering of a chunk that clamped -- the generator measures it, widens its range plan or falls back to bf16x3)
        img, _ = self.G([latent], input_is_latent=True, truncation=self.truncation, truncation_latent=self.trunc,
                        image_out=image_out, graph=False if (self.use_graph or no_graph or verify) else (True if prefer_graph else None),
                        verify_range=bool(verify))
        return img

    def _graphed_step(self, sv):
        mode = self.G.range_mode()
        if self._graph is not None and self._graph[3] != mode:          # the generator changed arithmetic (fallback / new weights)
            self._graph = None
        if self._graph is None:
            static_sv = sv.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                                   # warm-up off the capture: packs, caches, allocator
                for _ in range(2):
                    self._step(static_sv)
            torch.cuda.current_stream().wait_stream(side)
            mode = self.G.range_mode()                                      # (the warm-up may have calibrated / fallen back)
            g = torch.cuda.CUDAGraph()
            with F_.capture_graph(g):
                static_out = self._step(static_sv)
            self._graph = (g, static_sv, static_out, mode)
        g, static_sv, static_out, mode = self._graph
        static_sv.copy_(sv)
        g.replay()
        # the captured launches add to the generator's saturation word like eager ones: snapshot it behind the replay
        tok = self.G._snapshot() if mode == 'fp16x3' else None
        return static_out.clone(), tok

    def _chunks(self, pipelined, device):
        """launch(lo, sv, u8) -> item / settle(item) -> (lo, sv, u8, images, graphed) for one chunk each; see _pipeline."""
        sess = self
        pipe = None
        # (chunks small enough for the generator's own hipGraph replay are host-bound and share the graph's static buffers: one stream)
        if pipelined and self.n_streams > 1 and not self.use_graph and \
                self.batch * (self.G.size / 256.0) ** 2 > self.pipeline_min_work:
            if self._pipe is None or self._pipe.streams[0].device != device:
                self._pipe = F_.StreamPipeline(self.n_streams, device)
            pipe = self._pipe

        class Chunks:
            def launch(self, lo, sv, u8):
                if sess.use_graph and sv.shape[0] == sess.batch:
                    img, tok = sess._graphed_step(sv)
                    return [lo, sv, u8, img, tok, True, None, 'graph']
                mode = sess.G.range_mode()
                if pipe is None:
                    # (one stream: the chunk's token is awaited right behind its launches, which exposes the ~0.5 ms of host enqueue
                    # time of an eager forward -- the generator replays its hipGraph for these, as a verified forward does)
                    img = sess._step(sv, u8, prefer_graph=True)
                    return [lo, sv, u8, img, sess.G.take_range_token(), False, None, mode]
                with pipe.next():
                    img = sess._step(sv, u8, no_graph=True)
                    tok = sess.G.take_range_token()
                return [lo, sv, u8, img, tok, False, pipe.last, mode]

            def settle(self, item):
                lo, sv, u8, img, tok, graphed, stream, mode = item
                # False for a chunk that clamped operands AND for one that was in flight beside it on the other stream (the shared
                # saturation word cannot tell the two apart: RangeToken.suspect)
                ok = sess.G.range_ok(tok)
                if stream is not None:
                    pipe.join(img, stream=stream)                           # the caller's stream may now read this chunk
                if not ok:
                    sess._graph = None                                      # this chunk again, eagerly and VERIFIED: the generator measures
                    img, graphed = sess._step(sv, u8, verify=True), False   # it and widens its range plan (or renders in bf16x3)
                return lo, sv, u8, img, graphed

        return Chunks()

    def _pipeline(self, shift_vectors, target_for=None):
        """(lo, image batch) for every chunk of `shift_vectors`, each VERIFIED against the generator's fp16 range plan before
        it is yielded: chunk i+1 is queued first (on the other HIP stream when the session pipelines), then chunk i's RangeToken
        is awaited (the GPU never idles for the check), and a chunk that clamped operands is rendered again in the generator's
        fallback arithmetic.  target_for(lo, b) -> functional.U8Target or None (eager chunks: the last ToRGB launch writes uint8
        frames)."""
        n = shift_vectors.shape[0]
        chunks = self._chunks(n > self.batch, shift_vectors.device)
        pending = None
        for lo in range(0, n, self.batch):
            sv = shift_vectors[lo:lo + self.batch]
            cur = chunks.launch(lo, sv, target_for(lo, sv.shape[0]) if target_for is not None else None)
            if pending is not None:
                yield chunks.settle(pending)
            pending = cur
        if pending is not None:
            yield chunks.settle(pending)

    def streaming(self, as_uint8=False):
        """For frames that arrive chunk by chunk (a live video, bench.py's inference config): `push(shift_vectors [b, dim])`
        queues that chunk and returns the images of the PREVIOUS one (None for the first), `flush()` returns the last -- the same
        one-chunk look-ahead, stream alternation and range verification as `frames`, kept alive between calls."""
        sess = self

        class Streaming:
            def __init__(self):
                self.chunks, self.pending, self.count = None, None, 0

            def _out(self, item):
                lo, sv, u8, img, graphed = self.chunks.settle(item)
                if sess.pool_to is not None:
                    return pool_images(img, sess.pool_to, as_uint8)
                return images_to_uint8(img) if (as_uint8 and graphed) else img

            @torch.no_grad()
            def push(self, shift_vectors):
                if self.chunks is None:
                    self.chunks = sess._chunks(True, shift_vectors.device)
                cur = self.chunks.launch(self.count, shift_vectors, F_.U8Target() if (as_uint8 and sess.pool_to is None) else None)
                self.count += shift_vectors.shape[0]
                prev, self.pending = self.pending, cur
                return self._out(prev) if prev is not None else None

            @torch.no_grad()
            def flush(self):
                prev, self.pending = self.pending, None
                return self._out(prev) if prev is not None else None

        return Streaming()

    @torch.no_grad()
    def frames(self, shift_vectors, as_uint8=False):
        """shift_vectors [N, input_dim] -> generator of image batches (same result as N generate_image calls)."""
        if self.pool_to is not None:
            for lo, sv, u8, img, graphed in self._pipeline(shift_vectors, None):
                yield pool_images(img, self.pool_to, as_uint8)
            return
        for lo, sv, u8, img, graphed in self._pipeline(shift_vectors, (lambda lo, b: F_.U8Target()) if as_uint8 else None):
            # eager uint8 frames come straight out of the last ToRGB launch (no fp32 image is stored); a replayed graph
            # produced fp32 images
            yield images_to_uint8(img) if (as_uint8 and graphed) else img

    def render(self, shift_vectors, as_uint8=False):
        return torch.cat(list(self.frames(shift_vectors, as_uint8=as_uint8)), 0)

    def shift_vectors_for(self, angles_source, params_source, angles_target, params_target):
        """[N, learned_directions] for N target frames against the one source identity, in one launch and without a
        host round trip (the reference: run_inference.py:178 `make_shift`, once per frame, ~10 `.cpu()` syncs each)."""
        if self.shifts is None:
            raise RuntimeError('this session was built without direction tables (pass shifts=ShiftVectors(...))')
        return self.shifts.make_shift(angles_source, angles_target, params_source, params_target)

    def frames_for_targets(self, angles_source, params_source, angles_target, params_target, as_uint8=False):
        """run_inference.py:170-181 for all target frames: 3DMM parameters in, image batches out."""
        return self.frames(self.shift_vectors_for(angles_source, params_source, angles_target, params_target), as_uint8=as_uint8)

    def render_targets(self, angles_source, params_source, angles_target, params_target, as_uint8=False):
        return torch.cat(list(self.frames_for_targets(angles_source, params_source, angles_target, params_target,
                                                      as_uint8=as_uint8)), 0)

    @torch.no_grad()
    def video_frames(self, source_image, target_images, shift_vectors, swap_rb=True, out=None):
        """source | target | reenacted frames [N,H,3W,3] uint8 (the --save_video output of run_inference.py:186-198).
        target_images: [N,3,H,W] float32 in [-1,1], or the uint8 crops [N,H,W,3] themselves (preprocess_frames' first result): the
        grid launch then reads a quarter of the bytes and no float crop has to exist (video_frames_px; the bytes are those of the
        float crop u / 255 * 2 - 1).  A float input takes the launches it always took.  out: a contiguous uint8 [N,H,3W,3] device
        tensor to write into (a slice of a larger result)."""
        n = shift_vectors.shape[0]
        H, W = source_image.shape[-2], source_image.shape[-1]
        as_bytes = target_images.dtype == torch.uint8
        if as_bytes and (H != W or tuple(target_images.shape) != (n, H, W, 3)):
            raise RuntimeError('video_frames: uint8 target crops must be [%d,%d,%d,3] next to a square source panel, got %s'
                               % (n, H, W, tuple(target_images.shape)))
        video = _frames_out('video_frames', out, (n, H, 3 * W, 3), shift_vectors.device, False)
        if self.pool_to is not None:
            if (H, W) != (self.pool_to, self.pool_to):
                raise RuntimeError('video_frames: this session pools to %d, the source panel is %d x %d' % (self.pool_to, H, W))
            fused = video_frames_px if as_bytes else video_frames_uint8
            for lo, sv, u8, img, graphed in self._pipeline(shift_vectors, None):
                b = sv.shape[0]
                fused(img, [source_image, target_images[lo:lo + b]], self.pool_to, swap_rb=swap_rb, out=video[lo:lo + b])
            return video
        # eager chunks: the reenacted panel is written by the generator's last launch; the other two by one grid launch
        target_for = lambda lo, b: F_.U8Target(video[lo:lo + b], panel=2, swap_rb=swap_rb)
        for lo, sv, u8, img, graphed in self._pipeline(shift_vectors, target_for):
            frames = video[lo:lo + sv.shape[0]]
            if as_bytes:
                video_frames_px(img if graphed else None, [source_image, target_images[lo:lo + sv.shape[0]]], H, swap_rb=swap_rb, out=frames)
            else:
                grid_frames_uint8([source_image, target_images[lo:lo + sv.shape[0]], img if graphed else None], swap_rb=swap_rb, out=frames)
        return video


ON_FAIL = ('hold', 'source', 'raise')
OUTPUTS = ('video', 'images')


def _raise_failed_rows(who, ok):
    """on_fail='raise': ONE host read, then RuntimeError naming the rows that are not ok."""
    bad = (~ok).cpu().nonzero().flatten().tolist()                         # the one host read
    if bad:
        raise RuntimeError('%s: %d of %d target frames failed (no face, an invalid crop, or masked out): rows %s'
                           % (who, len(bad), ok.shape[0], bad))


def _device_frames(frames, who):
    if not torch.is_tensor(frames):
        raise RuntimeError('%s: expected a uint8 tensor of frames, got %s' % (who, type(frames)))
    N.require_device(frames, dtype=torch.uint8)
    return frames


_ANALYSIS_FIELDS = ('crops', 'angles', 'ok', 'valid')


class TargetAnalysis:
    """What the heads find in N target frames, kept small: everything `Reenactor.reenact` needs of them, and nothing of any source.

        crops  [N,256,256,3] uint8   the alignment crops, the bytes preprocess_frames returns (an invalid row is zeros)
        params {key: [N,.]}          train_step.shape_params of the crops, rows concatenated
        angles [N,3]
        ok     [N] bool              has_face on the frame & valid crop & has_face on the crop
        valid  [N] bool              the crop's own flag: the float crop of an invalid row is 0.0 where its bytes would map to -1,
                                     so the target panel needs it to show such a row as `reenact` shows it (BLANK_BYTE)
        batch  int                   the chunking it was made with (the heads' results depend on it in the last bits)

    0.20 MB a frame.  len(a), a[lo:hi] (views), TargetAnalysis.cat([...]), a.to(device), a.as_dict() / TargetAnalysis.from_dict(d):
    plain tensors and ints, so torch.save / torch.load make a cache across processes.  cat of analyses made segment by segment equals
    the analysis of the whole bit for bit when every segment boundary is a multiple of `batch`: the chunks are then the same chunks."""

    def __init__(self, crops, params, angles, ok, valid, batch):
        n = crops.shape[0] if torch.is_tensor(crops) and crops.ndim == 4 else -1
        if n < 0 or crops.dtype != torch.uint8 or crops.shape[3] != 3 or crops.shape[1] != crops.shape[2]:
            raise RuntimeError('TargetAnalysis: crops must be a uint8 tensor [N,S,S,3]')
        if not isinstance(params, dict) or not params or not all(torch.is_tensor(v) and v.ndim == 2 and v.shape[0] == n for v in params.values()):
            raise RuntimeError('TargetAnalysis: params must be a dict of [%d,.] tensors' % n)
        if not torch.is_tensor(angles) or tuple(angles.shape) != (n, 3):
            raise RuntimeError('TargetAnalysis: angles must be [%d,3]' % n)
        for name, t in (('ok', ok), ('valid', valid)):
            if not torch.is_tensor(t) or t.dtype != torch.bool or tuple(t.shape) != (n,):
                raise RuntimeError('TargetAnalysis: %s must be a bool tensor [%d]' % (name, n))
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise RuntimeError('TargetAnalysis: batch must be a positive int, got %r' % (batch,))
        if len({t.device for t in [crops, angles, ok, valid] + list(params.values())}) != 1:
            raise RuntimeError('TargetAnalysis: all tensors must live on one device')
        self.crops, self.params, self.angles, self.ok, self.valid, self.batch = crops, dict(params), angles, ok, valid, batch

    def __len__(self):
        return self.crops.shape[0]

    @property
    def device(self):
        return self.crops.device

    def __getitem__(self, rows):
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise RuntimeError('TargetAnalysis: index with a slice lo:hi (the rows stay in order; views, nothing is copied)')
        return TargetAnalysis(self.crops[rows], {k: v[rows] for k, v in self.params.items()}, self.angles[rows], self.ok[rows],
                              self.valid[rows], self.batch)

    @staticmethod
    def cat(analyses):
        analyses = list(analyses)
        if not analyses or not all(isinstance(a, TargetAnalysis) for a in analyses):
            raise RuntimeError('TargetAnalysis.cat: expected a non-empty list of TargetAnalysis')
        first = analyses[0]
        for a in analyses[1:]:
            if a.batch != first.batch:
                raise RuntimeError('TargetAnalysis.cat: analyses made with different batch sizes (%d and %d)' % (first.batch, a.batch))
            if list(a.params) != list(first.params):
                raise RuntimeError('TargetAnalysis.cat: analyses with different param keys (%s and %s)' % (list(first.params), list(a.params)))
        join = lambda get: torch.cat([get(a) for a in analyses], 0)
        return TargetAnalysis(join(lambda a: a.crops), {k: join(lambda a, k=k: a.params[k]) for k in first.params},
                              join(lambda a: a.angles), join(lambda a: a.ok), join(lambda a: a.valid), first.batch)

    def to(self, device):
        move = lambda t: t.to(device)
        return TargetAnalysis(move(self.crops), {k: move(v) for k, v in self.params.items()}, move(self.angles), move(self.ok),
                              move(self.valid), self.batch)

    def as_dict(self):
        d = {name: getattr(self, name) for name in _ANALYSIS_FIELDS}
        d.update({'params.' + k: v for k, v in self.params.items()})
        d['batch'] = self.batch
        return d

    @staticmethod
    def from_dict(d):
        missing = [k for k in _ANALYSIS_FIELDS + ('batch',) if k not in d]
        if missing:
            raise RuntimeError('TargetAnalysis.from_dict: the dict lacks %s' % missing)
        params = {k[len('params.'):]: v for k, v in d.items() if k.startswith('params.')}
        return TargetAnalysis(d['crops'], params, d['angles'], d['ok'], d['valid'], int(d['batch']))


class Source:
    """One source identity as `Reenactor.make_source` prepares it: code (the e4e W+ code), G_source (the generator that renders it:
    the PTI-tuned copy, or the base generator itself), x [1,3,256,256] and crop [1,256,256,3] (the cropped real image), params /
    angles (its 3DMM parameters), inverted (the e4e inversion before PTI), loss (the last PTI loss, a 0-d device tensor, or None)."""

    def __init__(self, code, G_source, x, crop, params, angles, inverted, loss):
        self.code, self.G_source, self.x, self.crop = code, G_source, x, crop
        self.params, self.angles, self.inverted, self.loss = params, angles, inverted, loss


class Reenactor:
    """Frames in, video frames out: Inference.run_reenactment of the reference (run_inference.py:157-199) on this package's heads.

        r = Reenactor(G, A, enc, det, fan, E, shifts, truncation=0.7, trunc=trunc, lpips=lpips, batch=32)
        info = r.set_source(frame)                        # crop -> e4e -> PTI on a copy of G -> session -> the source's 3DMM parameters
        video, ok, sv = r.reenact(frames)                 # [N,256,768,3] uint8: source crop | target crop | reenacted

    G / A: the generator and its DirectionMatrix; enc: the e4e encoder (encoder.encode); det, fan: S3FD and FAN; E: the DECA encoder;
    shifts: the shift.ShiftVectors of the dataset; trunc: the truncation latent; lpips: the lpips.LPIPS of the PTI loss (needed for
    set_source(optimize=True) only); batch: target frames per launch of every head and of the generator.  A generator above 256^2
    is rendered through a session that pools to 256 (ReenactmentSession(pool_to=256)), as generic.generate_image does in the
    reference's loop.  image_resize(width=1000) of the reference's preprocess_image stays with the caller.

    Cross-reenactment: nearly all of a `reenact` call is the analysis of the target frames, which knows nothing of the
    source.  `analyse` does it once, any number of sources are rendered from the result, and `cross_metrics` scores them:

        a = r.analyse(frames)                             # TargetAnalysis: uint8 crops, 3DMM parameters, ok; needs no source
        torch.save(a.as_dict(), path)                     # ... a = TargetAnalysis.from_dict(torch.load(path)).to('cuda')
        srcs = [r.make_source(f, optimize=False) for f in source_frames]
        videos, ok, sv = r.reenact_many(srcs, a)          # [S,N,256,768,3] uint8; each row what use_source + reenact_analysed gives
        csim, pose, exp_error, ok_r = r.cross_metrics(srcs, a, sv, id_loss)      # [S,N] each

    Four deliberate deviations from the reference:
      * a target frame that fails (no face on the frame, an invalid crop, no face on the crop, or the caller's `valid` mask) is
        rendered by a stated policy (`on_fail`); the reference exits on the first two and renders from angles of -180 and zero
        coefficients on the third (estimate_DECA.py:48-51);
      * PTI uses the `trunc` given here; the reference's optimize_g draws a fresh mean_latent(4096) of its own (optimization.py:26);
      * PTI tunes a deep copy: `G` stays bit-unchanged, so the next set_source starts from the base generator.  The reference's
        optimize_g trains the generator it is handed (optimization.py:28-29 copies it for the regulariser only);
      * PTI on a 512 or 1024 generator compares the output pooled to 256 x 256 with the crop (finetune.PooledPtiLoss): the image
        generic.generate_image hands out, AdaptiveAvgPool2d((256,256)) of the generator's (generic.py:146-148).  The reference's
        optimize_g calls the generator directly and hands its loss the 1024^2 output beside the 256^2 crop (optimization.py:50-58):
        it cannot run there.  `Source.inverted` stays at the generator's own size."""

    def __init__(self, G, A, enc, det, fan, E, shifts, truncation=0.7, trunc=None, lpips=None, batch=32):
        if truncation < 1 and trunc is None:
            raise RuntimeError('truncation < 1 needs the truncation latent')
        if A.input_dim != shifts.learned_directions:
            raise RuntimeError('Reenactor: the DirectionMatrix takes %d directions, the tables hold %d' % (A.input_dim, shifts.learned_directions))
        self.G, self.A, self.enc, self.det, self.fan, self.E, self.shifts = G, A, enc, det, fan, E, shifts
        self.truncation, self.trunc, self.lpips, self.batch = truncation, trunc, lpips, int(batch)
        self.pool_to = 256 if G.size > 256 else None
        self.session = None             # set_source makes these
        self.G_source = self.source_x = self.source_params = self.source_angles = None
        self._carry = self._carry_valid = None

    def make_source(self, frame, optimize=True, opt_steps=200, lr=3e-3):
        """Everything `set_source` does short of selecting the source, for one source frame [H,W,3] or [1,H,W,3] uint8 on the device:
        preprocess_frames at B=1 -> invert_images -> (optimize) finetune.optimize_g with PtiLoss(lpips, x) (a 512 or 1024 generator:
        PooledPtiLoss(lpips, x, 256), the class docstring's fourth deviation) on a deep copy of G,
        optimize_all=False, the Reenactor's trunc (on G itself without optimisation, run_inference.py:121-124) ->
        train_step.shape_params of the crop x (the cropped real image, not the inversion).  Returns a `Source`; the Reenactor's
        current source and hold carry are untouched, so any number can be made and kept side by side (reenact_many).

        ONE host read of its own: the source's `ok` flag -- a source without a usable face raises RuntimeError (the reference exits
        there).  Nothing else in this method's own code synchronises; the heads keep their own behaviour (a verified generator
        forward waits for its range check)."""
        from . import finetune
        from .train_step import shape_params
        if optimize and self.lpips is None:
            raise RuntimeError('set_source(optimize=True) needs the LPIPS head of the PTI loss (Reenactor(..., lpips=...))')
        frame = _device_frames(frame, 'set_source')
        if frame.ndim == 3:
            frame = frame.unsqueeze(0)
        if frame.ndim != 4 or frame.shape[0] != 1:
            raise RuntimeError('set_source: one source frame [H,W,3] or [1,H,W,3], got %s' % (tuple(frame.shape),))
        if optimize and self.G.size not in (256, 512, 1024):
            raise RuntimeError('set_source(optimize=True): PTI compares the generator output, pooled by 1, 2 or 4, with the 256 x 256 '
                               'crop; this generator renders %d x %d' % (self.G.size, self.G.size))
        crop, x, ok = preprocess_frames(self.det, self.fan, frame.contiguous())
        if not bool(ok.item()):                                            # the one host read
            raise RuntimeError('set_source: no usable face in the source frame (no detection, or a crop outside the size limits)')
        with torch.no_grad():
            code, inverted = invert_images(self.enc, self.G, x, self.truncation, self.trunc)
        G_source, loss = self.G, None
        if optimize:
            import copy
            G_source = copy.deepcopy(self.G)                               # (model.Generator.__deepcopy__ leaves graphs and tokens behind)
            G_source.invalidate_packs()                                    # ... and the copied weight packs are keyed on G's storage
            # above 256 the loss sees what generate_image hands out: the output pooled to the crop's side (the fourth deviation)
            loss_fn = finetune.PtiLoss(self.lpips, x) if self.G.size == 256 else finetune.PooledPtiLoss(self.lpips, x, 256)
            G_source, loss = finetune.optimize_g(G_source, code, x, self.trunc, opt_steps=opt_steps, lr=lr, optimize_all=False,
                                                 loss_fn=loss_fn, truncation=self.truncation)
            G_source.eval()
            for p in G_source.parameters():
                p.grad = None
        with torch.no_grad():
            params, angles = shape_params(self.det, self.fan, self.E, x)
        return Source(code, G_source, x, crop, params, angles, inverted, loss)

    def _session_for(self, source):
        """The ReenactmentSession that renders `source` for this Reenactor, made once per Source (its streams and events with it)."""
        kept = getattr(source, '_session', None)
        if kept is None or kept[0] is not self or kept[1].batch != self.batch:
            kept = (self, ReenactmentSession(source.G_source, self.A, source.code, self.truncation, self.trunc, batch=self.batch,
                                             shifts=self.shifts, pool_to=self.pool_to))
            source._session = kept
        return kept[1]

    def use_source(self, source):
        """Select a `Source` made by make_source: a ReenactmentSession on its generator, its 3DMM parameters as the shift vectors'
        source side, and the hold carry of `reenact` / `reenact_analysed` reset.  No launch, no host read."""
        if not isinstance(source, Source):
            raise RuntimeError('use_source: expected a Source made by make_source, got %s' % type(source))
        self.G_source = source.G_source
        self.session = self._session_for(source)
        self.source_params, self.source_angles, self.source_x = source.params, source.angles, source.x
        D = self.shifts.learned_directions
        self._carry = torch.zeros(D, device=source.x.device)
        self._carry_valid = torch.zeros((), dtype=torch.bool, device=source.x.device)

    def set_source(self, frame, optimize=True, opt_steps=200, lr=3e-3):
        """load_source_data + run_inference.py:169 for one source frame [H,W,3] or [1,H,W,3] uint8 on the device: make_source
        (crop -> e4e -> PTI on a deep copy of G -> the source's 3DMM parameters) followed by use_source (the session, the hold carry of
        `reenact` reset).  Returns {'crop' [1,256,256,3] uint8, 'x' [1,3,256,256], 'source_code', 'inverted', 'params', 'angles',
        'loss': the last PTI loss as a 0-d device tensor (None without optimisation)}.

        ONE host read, make_source's: a source without a usable face raises RuntimeError (the reference exits there)."""
        src = self.make_source(frame, optimize=optimize, opt_steps=opt_steps, lr=lr)
        self.use_source(src)
        return {'crop': src.crop, 'x': src.x, 'source_code': src.code, 'inverted': src.inverted, 'params': src.params,
                'angles': src.angles, 'loss': src.loss}

    def _head_chain(self, frames):
        """One chunk of target frames through the heads: _preprocess -> detect_landmarks(input_range='gan') on the crops ->
        shape_params(boxes=, has_face=) -> (crop uint8, x float, params, angles, has_face on the frame, valid crop, has_face on the
        crop).  `analyse` and `target_shift_vectors` chunk by `batch` and call this, so their bits agree."""
        from .face_detector import detect_landmarks
        from .train_step import shape_params
        crop, x, has_frame, valid = _preprocess(self.det, self.fan, frames)
        _, boxes, has = detect_landmarks(self.det, self.fan, x, input_range='gan')
        params, angles = shape_params(self.det, self.fan, self.E, x, boxes=boxes, has_face=has)
        return crop, x, params, angles, has_frame, valid, has

    @staticmethod
    def _check_policy(who, on_fail, output):
        """on_fail and output of the three reenact methods: refused before anything else is looked at."""
        if on_fail not in ON_FAIL:
            raise RuntimeError('%s: on_fail must be one of %s, got %r' % (who, ', '.join(ON_FAIL), on_fail))
        if output not in OUTPUTS:
            raise RuntimeError('%s: output must be one of %s, got %r' % (who, ', '.join(OUTPUTS), output))

    @staticmethod
    def _check_valid(who, valid, n):
        """The caller's `valid` mask of the three reenact methods, once the rows are known to be n: None or a bool tensor [n]."""
        if valid is not None and (not torch.is_tensor(valid) or valid.dtype != torch.bool or tuple(valid.shape) != (n,)):
            raise RuntimeError('%s: valid must be a bool tensor [%d]' % (who, n))

    def _apply_on_fail(self, who, sv, ok, on_fail):
        """The shift vectors a call renders: sv [N,D] (reenact, reenact_analysed: 'hold' uses and updates the Reenactor's carry) or
        [S,N,D] (reenact_many: every source holds from an empty carry) under the policy for the rows whose ok [N] is False."""
        if on_fail == 'raise':
            _raise_failed_rows(who, ok)
            return sv
        if on_fail == 'source':
            return torch.where(ok.unsqueeze(-1), sv, torch.zeros((), dtype=sv.dtype, device=sv.device))
        if sv.ndim == 3:
            return hold_failed_rows_many(sv, ok)
        sv, self._carry, self._carry_valid = hold_failed_rows(sv, ok, self._carry, self._carry_valid)
        return sv

    @torch.no_grad()
    def analyse(self, frames):
        """The head chain of `target_shift_vectors` for frames [N,H,W,3] uint8 on the device, up to but not including make_shift, so
        without any source (it works before set_source): `batch` frames at a time preprocess_frames -> detect_landmarks(input_range=
        'gan') on the crops -> shape_params(boxes=, has_face=).  Returns a `TargetAnalysis`; the float crops live only inside a chunk.
        No host synchronisation of its own."""
        frames = _device_frames(frames, 'analyse')
        if frames.ndim != 4 or frames.shape[0] < 1:
            raise RuntimeError('analyse: expected frames [N,H,W,3], got %s' % (tuple(frames.shape),))
        frames = frames.contiguous()
        crops, angles, oks, valids, params = [], [], [], [], {}
        for lo in range(0, frames.shape[0], self.batch):
            crop, x, p, ang, has_frame, valid, has = self._head_chain(frames[lo:lo + self.batch])
            for k, v in p.items():
                params.setdefault(k, []).append(v)
            crops.append(crop)
            angles.append(ang)
            oks.append(has_frame & valid & has)
            valids.append(valid)
        return TargetAnalysis(torch.cat(crops, 0), {k: torch.cat(v, 0) for k, v in params.items()}, torch.cat(angles, 0),
                              torch.cat(oks, 0), torch.cat(valids, 0), self.batch)

    @torch.no_grad()
    def target_shift_vectors(self, frames):
        """The head chain of run_inference.py:173-178 for frames [N,H,W,3] uint8, `batch` at a time: preprocess_frames ->
        face_detector.detect_landmarks(input_range='gan') on the crops -> shape_params(boxes=, has_face=) -> shifts.make_shift
        against the source's rows.  Returns (x [N,3,256,256] the target crops, sv [N,D] before any policy, ok [N] bool =
        has_face on the frame & valid crop & has_face on the crop)."""
        xs, svs, oks = [], [], []
        for lo in range(0, frames.shape[0], self.batch):
            _, x, params, angles, has_frame, valid, has = self._head_chain(frames[lo:lo + self.batch])
            svs.append(self.shifts.make_shift(self.source_angles, angles, self.source_params, params))
            xs.append(x)
            oks.append(has_frame & valid & has)
        return torch.cat(xs, 0), torch.cat(svs, 0), torch.cat(oks, 0)

    @torch.no_grad()
    def reenact(self, frames, valid=None, on_fail='hold', output='video'):
        """run_inference.py:170-195 for target frames [N,H,W,3] uint8 on the device -> (frames, ok [N] bool, shift_vectors [N,D]).

        ok: has_face on the frame & valid crop & has_face on the crop & the caller's `valid` ([N] bool tensor, e.g. scene cuts).
        on_fail: what a row that is not ok renders -- 'hold': the shift vector of the nearest earlier ok row, earlier calls since
        set_source included (a device carry), zeros if there is none; 'source': zeros, which renders the inverted source; 'raise':
        ONE host read, then RuntimeError naming the rows.  shift_vectors are those rendered, after the policy.
        output: 'video' [N,256,768,3] uint8, source crop | target crop | reenacted with swap_rb (the --save_video frames,
        run_inference.py:188-195); 'images' [N,256,256,3] uint8 RGB, reenacted only (--save_images).

        Apart from on_fail='raise' nothing in this method's own code synchronises with the host; the session awaits each chunk's
        range check one chunk behind its launches, as it always does.  The target crops of a 'video' call stay on the device until
        it returns (0.79 MB per frame): hand a long video over in segments, the hold carry spans the calls -- or `analyse` it once
        (0.20 MB per frame, uint8) and render from that with `reenact_analysed` / `reenact_many`."""
        self._check_policy('reenact', on_fail, output)
        frames = _device_frames(frames, 'reenact')
        if self.session is None:
            raise RuntimeError('reenact: no source yet (call set_source first)')
        if frames.ndim != 4 or frames.shape[0] < 1:
            raise RuntimeError('reenact: expected frames [N,H,W,3], got %s' % (tuple(frames.shape),))
        self._check_valid('reenact', valid, frames.shape[0])
        x, sv, ok = self.target_shift_vectors(frames.contiguous())
        if valid is not None:
            ok = ok & valid.to(frames.device)
        sv = self._apply_on_fail('reenact', sv, ok, on_fail)
        if output == 'video':
            out = self.session.video_frames(self.source_x, x, sv, swap_rb=True)
        else:
            out = self.session.render(sv, as_uint8=True)
        return out, ok, sv

    def _check_analysed(self, who, analysis, valid, on_fail, output):
        """The argument checks shared by reenact_analysed and reenact_many -> (ok [N] with the caller's mask folded in)."""
        self._check_policy(who, on_fail, output)
        if not isinstance(analysis, TargetAnalysis):
            raise RuntimeError('%s: expected the TargetAnalysis of analyse(frames), got %s' % (who, type(analysis)))
        n = len(analysis)
        self._check_valid(who, valid, n)
        N.require_device(analysis.crops, dtype=torch.uint8)
        N.require_device(analysis.angles, *analysis.params.values())
        if n < 1 or tuple(analysis.crops.shape[1:]) != (256, 256, 3):
            raise RuntimeError('%s: expected an analysis of N >= 1 crops [N,256,256,3], got %s' % (who, tuple(analysis.crops.shape)))
        return analysis.ok if valid is None else analysis.ok & valid.to(analysis.ok.device)

    def _finish_target_panel(self, video, analysis):
        """The target panel of the rows whose crop is invalid: their float crop is 0.0 in every pixel (BLANK_BYTE in a frame), their
        bytes are zeros (which map to -1, byte 0).  One masked fill over the panel, no host read; `video` is [...,N,256,768,3]."""
        video[..., 256:512, :].masked_fill_(~analysis.valid.view(-1, 1, 1, 1), BLANK_BYTE)

    @torch.no_grad()
    def reenact_analysed(self, analysis, valid=None, on_fail='hold', output='video'):
        """`reenact` from the TargetAnalysis of its frames: make_shift against the current source, the same valid / on_fail / output
        rules, the same hold carry used and updated, the target panel converted from analysis.crops in the grid launch
        (video_frames_px).  -> (frames, ok, shift_vectors), bit for bit what reenact(frames) returns when the analysis was made
        with this Reenactor's batch.  No head runs.  Apart from on_fail='raise' nothing in this method's own code synchronises."""
        ok = self._check_analysed('reenact_analysed', analysis, valid, on_fail, output)
        if self.session is None:
            raise RuntimeError('reenact_analysed: no source yet (call set_source or use_source first)')
        sv = self.shifts.make_shift(self.source_angles, analysis.angles, self.source_params, analysis.params)
        sv = self._apply_on_fail('reenact_analysed', sv, ok, on_fail)
        if output == 'video':
            out = self.session.video_frames(self.source_x, analysis.crops, sv, swap_rb=True)
            self._finish_target_panel(out, analysis)
        else:
            out = self.session.render(sv, as_uint8=True)
        return out, ok, sv

    def _check_sources(self, who, sources):
        sources = list(sources)
        if not sources or not all(isinstance(s, Source) for s in sources):
            raise RuntimeError('%s: expected a non-empty list of the Sources make_source returns' % who)
        return sources

    @torch.no_grad()
    def reenact_many(self, sources, analysis, valid=None, on_fail='hold', output='video'):
        """Cross-reenactment: every Source of `sources` (make_source) rendered against the same TargetAnalysis -> (frames
        [S,N,256,768,3] uint8 for output='video' or [S,N,256,256,3] for 'images', ok [N] bool, shift_vectors [S,N,D]).  The video
        frames are 0.59 MB per frame and source, the images 0.20 MB: slice the analysis (a[lo:hi]) where S * N of them do not fit.

        Row s is what use_source(sources[s]) + reenact_analysed(analysis, ...) returns, bit for bit: each source is rendered by a
        ReenactmentSession of its own on its own G_source (sources that share a generator object share its weight packs and graphs),
        its N rows chunked by `batch` on their own, so a chunk never mixes sources.  ok depends on the targets alone: the rows the
        'hold' policy copies are found once for all sources.  Every source starts from an empty carry, nothing is carried out, and
        the Reenactor's current source and carry are untouched.  No head runs.  on_fail='raise' makes its ONE host read; nothing else
        in this method's own code synchronises."""
        sources = self._check_sources('reenact_many', sources)
        ok = self._check_analysed('reenact_many', analysis, valid, on_fail, output)
        sv = torch.stack([self.shifts.make_shift(s.angles, analysis.angles, s.params, analysis.params) for s in sources], 0)
        sv = self._apply_on_fail('reenact_many', sv, ok, on_fail)
        n = len(analysis)
        out = torch.empty(len(sources), n, 256, 768 if output == 'video' else 256, 3, device=sv.device, dtype=torch.uint8)
        for s, src in enumerate(sources):
            session = self._session_for(src)
            if output == 'video':
                session.video_frames(src.x, analysis.crops, sv[s], swap_rb=True, out=out[s])
            else:
                lo = 0
                for chunk in session.frames(sv[s], as_uint8=True):
                    out[s, lo:lo + chunk.shape[0]].copy_(chunk)
                    lo += chunk.shape[0]
        if output == 'video':
            self._finish_target_panel(out, analysis)
        return out, ok, sv

    @torch.no_grad()
    def cross_metrics(self, sources, analysis, shift_vectors, id_loss):
        """The scores of cross-reenactment for every (source, target frame) pair -> (csim, pose, exp_error: [S,N] float32 each,
        ok_reenacted [S,N] bool).  For every source, `batch` rows of `shift_vectors` [S,N,D] (reenact_many's) at a time: the float
        renders of its session (session.frames: no uint8 detour) -> detect_landmarks(input_range='gan') + shape_params on them ->
        train_step.evaluation_metrics against the targets' params / angles of the analysis, CSIM against the source crop x, as
        evaluate_model_reenactment_video scores against real frames.  ok_reenacted = analysis.ok & a face was found on the render;
        the scores of the other rows mean nothing.  id_loss: the id_loss.IDLoss head.  No host read."""
        from .face_detector import detect_landmarks
        from .train_step import evaluation_metrics, shape_params
        if not isinstance(analysis, TargetAnalysis):
            raise RuntimeError('cross_metrics: expected the TargetAnalysis of analyse(frames), got %s' % type(analysis))
        sources = self._check_sources('cross_metrics', sources)
        n, S = len(analysis), len(sources)
        if not torch.is_tensor(shift_vectors) or tuple(shift_vectors.shape) != (S, n, self.shifts.learned_directions):
            raise RuntimeError('cross_metrics: shift_vectors must be [%d,%d,%d] (reenact_many\'s third result)'
                               % (S, n, self.shifts.learned_directions))
        N.require_device(shift_vectors, analysis.angles)
        if id_loss is None:
            raise RuntimeError('cross_metrics: CSIM needs an id_loss head')
        dev = shift_vectors.device
        csim, pose, exp_error = (torch.empty(S, n, device=dev, dtype=torch.float32) for _ in range(3))
        ok_reenacted = torch.empty(S, n, device=dev, dtype=torch.bool)
        for s, src in enumerate(sources):
            lo = 0
            for img in self._session_for(src).frames(shift_vectors[s]):
                hi = lo + img.shape[0]
                _, boxes, has = detect_landmarks(self.det, self.fan, img, input_range='gan')
                params, angles = shape_params(self.det, self.fan, self.E, img, boxes=boxes, has_face=has)
                target = {k: v[lo:hi] for k, v in analysis.params.items()}
                c, p, e = evaluation_metrics(self.shifts, id_loss, params, target, angles, analysis.angles[lo:hi], img, src.x)
                csim[s, lo:hi], pose[s, lo:hi], exp_error[s, lo:hi] = c, p, e
                ok_reenacted[s, lo:hi] = analysis.ok[lo:hi] & has
                lo = hi
        return csim, pose, exp_error, ok_reenacted

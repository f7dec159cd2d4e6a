"""The FFHQ alignment crop on the HIP kernels of csrc/facecrop.hip: the counterpart of libs/face_models/ffhq_cropping.py
crop_using_landmarks (:49-69) with crop_from_bbox (:39-47) and pad_img_to_fit_bbox (:13-37), the step between the landmark detector
and the e4e encoder in preprocess_image (libs/utilities/utils_inference.py:61-82).

    crops, valid = crop_using_landmarks(frames, landmarks)                  # [B,256,256,3] uint8, [B] int32; no synchronisation
    (crops, x), valid = crop_using_landmarks(frames, landmarks, as_tensor=True)     # x [B,3,256,256] float32 in [-1,1] for e4e
    boxes, size = crop_boxes(landmarks)                                     # [B,4] int32 (x1, y1, x2, y2), [B] int32
    pix = crop_image(image, landmarks)                                      # numpy in, numpy out, the reference's signature

frames [B,H,W,3] uint8 and landmarks [B,68,2] float32, contiguous, on the device; one frame size per batch.  Rows whose box lies
inside the frame are resized directly; the others get the reference's reflected border, feathered Gaussian and median blends first.
The resize is Pillow's 8-bit bicubic resampler bit for bit.  `valid` is 0, and the row's crop zeros, where the box is empty
(size < 1), larger than `max_size` (default max(H, W) // 2, the workspace's capacity) or needs a border wider than the frame
dimension it reflects (the reference's border repeats there; such a box lies almost wholly outside the frame).  The frame is taken as
handed over: the reference's image_resize(width=1000) in front of the landmark detector is the caller's.
"""
import numpy as np
import torch

from . import _native as N

OUT_SIZE = 256
_workspaces = {}


def _check_landmarks(landmarks, B=None):
    if not torch.is_tensor(landmarks) or landmarks.dim() != 3 or tuple(landmarks.shape[1:]) != (68, 2) or landmarks.shape[0] < 1:
        raise ValueError('face_crop: expected [B,68,2] landmarks, got %s' % (tuple(landmarks.shape) if torch.is_tensor(landmarks) else
                                                                            type(landmarks),))
    if landmarks.dtype != torch.float32:
        raise ValueError('face_crop: landmarks must be float32, got %s' % landmarks.dtype)
    if not landmarks.is_contiguous():
        raise ValueError('face_crop: landmarks must be contiguous')
    if not landmarks.is_cuda:
        raise ValueError('face_crop: landmarks must be on the GPU, got %s: this package has no CPU path' % landmarks.device)
    if B is not None and landmarks.shape[0] != B:
        raise ValueError('face_crop: %d frames but %d landmark sets' % (B, landmarks.shape[0]))


def _check_frames(frames):
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError('face_crop: expected [B,H,W,3] frames, got %s' % (tuple(frames.shape) if torch.is_tensor(frames) else type(frames),))
    if frames.dtype != torch.uint8:
        raise ValueError('face_crop: frames must be uint8, got %s' % frames.dtype)
    if not frames.is_contiguous():
        raise ValueError('face_crop: frames must be contiguous')
    if not frames.is_cuda:
        raise ValueError('face_crop: frames must be on the GPU, got %s: this package has no CPU path' % frames.device)


def _check_sizes(out_size, max_size, H, W):
    if not isinstance(out_size, int) or isinstance(out_size, bool) or not 1 <= out_size <= 1024:
        raise ValueError('face_crop: out_size must be an integer in 1..1024, got %r' % (out_size,))
    if max_size is None:
        max_size = max(max(H, W) // 2, 1)
    if not isinstance(max_size, int) or isinstance(max_size, bool) or not 1 <= max_size <= 4096:
        raise ValueError('face_crop: max_size must be an integer in 1..4096, got %r' % (max_size,))
    return max_size


def _workspace(B, H, W, max_size, device):
    key = (B, H, W, max_size, device)
    hit = _workspaces.get(key)
    if hit is None:
        nbytes = N.size('sgdfr_facecrop_workspace_bytes', B, H, W, max_size,
                        error='face_crop: unsupported batch of %d frames of %dx%d with max_size %d (1..1024 rows, sides and max_size '
                              '1..4096)' % (B, H, W, max_size))
        hit = _workspaces[key] = (torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes)
    return hit


def clear_workspaces():
    """Drop the cached workspaces (one per (B, H, W, max_size, device) seen)."""
    _workspaces.clear()


def crop_boxes(landmarks):
    """The reference's crop box per row -> (boxes [B,4] int32 = x1, y1, x2, y2, size [B] int32), on the device."""
    _check_landmarks(landmarks)
    B = landmarks.shape[0]
    boxes = torch.empty((B, 4), dtype=torch.int32, device=landmarks.device)
    size = torch.empty(B, dtype=torch.int32, device=landmarks.device)
    with torch.cuda.device(landmarks.device):
        N.call('sgdfr_facecrop_boxes_f32', N.ptr(landmarks), B, N.ptr(boxes), N.ptr(size), N.stream())
    return boxes, size


def _forward(frames, landmarks, out_size, max_size, as_tensor, want_float):
    _check_frames(frames)
    B, H, W, _ = frames.shape
    _check_landmarks(landmarks, B)
    if landmarks.device != frames.device:
        raise ValueError('face_crop: frames on %s but landmarks on %s' % (frames.device, landmarks.device))
    max_size = _check_sizes(out_size, max_size, H, W)
    dev = frames.device
    ws, nbytes = _workspace(B, H, W, max_size, dev)
    crops = torch.empty((B, out_size, out_size, 3), dtype=torch.uint8, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    e4e = torch.empty((B, 3, out_size, out_size), dtype=torch.float32, device=dev) if as_tensor else None
    boxes = torch.empty((B, 4), dtype=torch.int32, device=dev) if want_float else None
    size = torch.empty(B, dtype=torch.int32, device=dev) if want_float else None
    flt = torch.zeros((B, 2 * max_size * 2 * max_size * 3), dtype=torch.float32, device=dev) if want_float else None
    with torch.cuda.device(dev):
        N.call('sgdfr_facecrop_forward_u8', N.ptr(frames), N.ptr(landmarks), B, H, W, out_size, max_size, N.ptr(crops), N.ptr(valid),
               N.ptr(e4e), N.ptr(boxes), N.ptr(size), N.ptr(flt), N.ptr(ws), nbytes, N.stream())
    return crops, valid, e4e, boxes, size, flt


def crop_using_landmarks(frames, landmarks, out_size=OUT_SIZE, max_size=None, as_tensor=False):
    """frames [B,H,W,3] uint8, landmarks [B,68,2] float32 -> (crops [B,S,S,3] uint8, valid [B] int32); with as_tensor the first
    element is (crops, x) with x [B,3,S,S] float32 = crops / 255 * 2 - 1, what image_to_tensor hands to e4e.  No synchronisation."""
    crops, valid, e4e, _, _, _ = _forward(frames, landmarks, out_size, max_size, as_tensor, False)
    return ((crops, e4e) if as_tensor else crops), valid


def padded_float(frames, landmarks, out_size=OUT_SIZE, max_size=None):
    """Debug view: per row the float32 crop [2 size, 2 size, 3] in front of the truncation to uint8 (the frame's own bytes as floats
    for a row whose box is inside the frame, None for an invalid row), and the crops of the same run -> (list, crops, valid).
    SYNCHRONISES: the crop sides are read back."""
    crops, valid, _, _, size, flt = _forward(frames, landmarks, out_size, max_size, False, True)
    out = []
    for b, (s, v) in enumerate(zip(size.cpu().tolist(), valid.cpu().tolist())):
        out.append(flt[b, :2 * s * 2 * s * 3].view(2 * s, 2 * s, 3) if v else None)
    return out, crops, valid


def crop_image(image, landmarks, out_size=OUT_SIZE, device=None):
    """ffhq_cropping.crop_using_landmarks(image, landmarks): numpy [H,W,3] uint8 and [68,2] landmarks in, numpy [S,S,3] uint8 out,
    None where the row is not valid.  Copies to the current GPU and back (and so synchronises), as the reference's caller does."""
    if not isinstance(image, np.ndarray) or image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise ValueError('face_crop: expected a [H,W,3] uint8 array, got %s' % (
            '%s %s' % (image.shape, image.dtype) if isinstance(image, np.ndarray) else type(image),))
    landmarks = np.asarray(landmarks)
    if landmarks.shape != (68, 2):
        raise ValueError('face_crop: expected [68,2] landmarks, got %s' % (landmarks.shape,))
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    frames = torch.from_numpy(np.ascontiguousarray(image)).unsqueeze(0).to(dev)
    lm = torch.from_numpy(np.ascontiguousarray(landmarks, dtype=np.float32)).unsqueeze(0).to(dev)
    crops, valid = crop_using_landmarks(frames, lm, out_size)
    return crops[0].cpu().numpy() if int(valid[0]) else None

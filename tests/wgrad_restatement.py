"""The weight gradient of the modulated 3x3 conv (csrc/wgrad.hip) restated in plain Python and float64 (no GPU, no library call, no
import from the package): the host split-K plan (`wgrad_shape` + `wgrad_ksplit`), the packed-weight gradient taken by autograd through
torch's own convolution (not from the kernel's index formula), the finish expression, and the table of shapes the GPU tests run.
tests/test_cpu_wgrad_plan.py pins `plan` to the C ABI, the tap convention to the whole-layer oracle, and asserts the coverage condition
over `CASES`; tests/test_gpu_wgrad_edges.py runs the cases."""
import math

import torch
import torch.nn.functional as F


def _ceil(a, b):
    return -(-a // b)


def plan(B, Cin, Cout, H, W, up):
    """None where only the direct kernel applies, else the pixel plan of the MFMA kernel: chunks of PC pixels inside one image row
    (PC = min(W, 64 plain / 32 up), a power of two >= 4 that divides W), K slices of `chunks_per_block` consecutive chunks each
    (about 1024 blocks over all channel tiles, at least 4 chunks per block), and three derived flags."""
    pcmax = 32 if up else 64
    PC = min(W, pcmax)
    if W % PC or PC < 4 or PC & (PC - 1):
        return None
    cpr = W // PC
    total = B * H * cpr
    ntile = _ceil(Cout, 64) * _ceil(Cin, 64)
    by_tiles = _ceil(1024, ntile)
    by_chunks = max(1, _ceil(total, 4))
    cpb = _ceil(total, min(by_tiles, by_chunks))
    K = _ceil(total, cpb)
    per_image = H * cpr
    blocks = [(k * cpb, min(total, (k + 1) * cpb)) for k in range(K)]
    return {'PC': PC, 'chunks_per_row': cpr, 'total_chunks': total, 'ntile': ntile, 'K': K, 'chunks_per_block': cpb,
            'ragged': total % cpb != 0,                                             # the last block is short
            'straddle': any(lo // per_image != (hi - 1) // per_image for lo, hi in blocks),     # a block spans two images
            'capped': by_tiles < by_chunks}                                         # K limited by 1024 / ntile, not by total / 4


def planes_to_image(planes):
    """[B, C, 4, H+1, W+1] parity planes -> [B, C, 2H+1, 2W+1]: plane 2*py+px, row r, col c is pixel (2r+py, 2c+px).  The last row
    of the odd-row planes and the last column of the odd-column planes lie outside the image and take no part."""
    B, C, _, R, P = planes.shape
    img = planes.new_zeros(B, C, 2 * R - 1, 2 * P - 1)
    for py in (0, 1):
        for px in (0, 1):
            img[:, :, py::2, px::2] = planes[:, :, 2 * py + px, :R - py, :P - px]
    return img


def image_to_planes(img, outside=0.0):
    """The inverse; the plane entries outside the image take the value `outside`."""
    B, C, Hh, Ww = img.shape
    R, P = (Hh + 1) // 2, (Ww + 1) // 2
    planes = img.new_full((B, C, 4, R, P), outside)
    for py in (0, 1):
        for px in (0, 1):
            planes[:, :, 2 * py + px, :R - py, :P - px] = img[:, :, py::2, px::2]
    return planes


def outside_mask(H, W):
    """[4, H+1, W+1] bool: the plane entries that lie outside the (2H+1) x (2W+1) image."""
    m = torch.zeros(4, H + 1, W + 1, dtype=torch.bool)
    m[2:, H, :] = True          # odd-row planes, last row
    m[1::2, :, W] = True        # odd-column planes, last column
    return m


def _contract(gd, xs, Cout, Cin, up):
    wz = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    if up:
        out = F.conv_transpose2d(xs, wz.transpose(0, 1), stride=2)
    else:
        out = F.conv2d(xs, wz, padding=1)
    assert out.shape == gd.shape, (out.shape, gd.shape)
    return torch.autograd.grad((out * gd).sum(), wz)[0]


def _operands(g, d, x, s, up):
    g, x, s = g.double(), x.double(), s.double()
    B, Cin = s.shape
    Cout = g.shape[1]
    if up:
        g = planes_to_image(g)
    gd = g if d is None else g * d.double().view(B, Cout, 1, 1)
    xs = x.expand(B, -1, -1, -1) * s.view(B, Cin, 1, 1)         # x with one row is the broadcast constant input
    return gd, xs, Cout, Cin


def dwc64(g, d, x, s, up):
    """[Cout, Cin, 3, 3] float64: dL/d(packed weight) = sum_{b,p} (d*g)[b,o,shifted p] * (x*s)[b,i,p], as autograd gives it for
    L = sum (conv(x*s, W) * d*g).  g: [B,Cout,H,W] (plain) or the parity planes [B,Cout,4,H+1,W+1] (up); d [B,Cout] or None (= 1);
    x [B or 1,Cin,H,W]; s [B,Cin]."""
    gd, xs, Cout, Cin = _operands(g, d, x, s, up)
    return _contract(gd, xs, Cout, Cin, up)


def absdwc64(g, d, x, s, up):
    """The same contraction of |d*g| with |x*s|: the magnitude the rounding-error bounds scale with."""
    gd, xs, Cout, Cin = _operands(g, d, x, s, up)
    return _contract(gd.abs(), xs.abs(), Cout, Cin, up)


def scale_of(Cin):
    return 1.0 / math.sqrt(9 * Cin)


def dq64(a, d, s):
    """[Cout, Cin] float64: dL/dQ of the demodulation d = rsqrt(sum_i Q[o,i] s_i^2 + eps) from a = d * dL/dd."""
    a, d, s = a.double(), d.double(), s.double()
    return torch.einsum('bo,bi->oi', -0.5 * (a / d) * d ** 3, s * s)


def absdq64(a, d, s):
    """sum_b |coeff * s^2|: what the rounding error of a dq formed in fp32 scales with."""
    a, d, s = a.double(), d.double(), s.double()
    return torch.einsum('bo,bi->oi', (0.5 * (a / d) * d ** 3).abs(), s * s)


def finish64(dwc, w, dq):
    """[Cout, Cin, 3, 3] float64: scale * (dwc + 2 * (w*scale) * dq); w [1,Cout,Cin,3,3] or [Cout,Cin,3,3], dq [Cout,Cin] or None."""
    Cout, Cin = dwc.shape[:2]
    scale = scale_of(Cin)
    out = dwc.double()
    if dq is not None:
        out = out + 2.0 * (w.double().view(Cout, Cin, 3, 3) * scale) * dq.double().view(Cout, Cin, 1, 1)
    return scale * out


U = 2.0 ** -24


def bound64(case_B, H, W, K, absdwc, w=None, dq=None, absdq=None):
    """The derived per-element bound on |fp32 result - finish64| (float64 [Cout,Cin,3,3]).
    m = B*H*W + K + 4 roundings on the dwc part: the longest addition chain (one fma per pixel, one add per slice) plus one each for
    x*s, g*d, the slice-sum tail (the fma that adds the demodulation term) and *scale: m*u / (1 - m*u) * absdwc * scale.
    The demodulation term 2*(w*scale)*dq*scale is rounded three times (w*scale, the fma, *scale) and holds the fp32 scale twice,
    itself 1/sqrtf rounded twice: t = 7 roundings, t*u / (1 - t*u) of its magnitude.
    Where dq itself was formed in fp32 (B fmas, and five roundings for a/d, d*d, *d, the product and s*s) its error, at most
    (B + 6) u * sum_b |coeff * s^2|, goes through the same factor 2*|w*scale|*scale with the same seven roundings."""
    Cout, Cin = absdwc.shape[:2]
    scale = scale_of(Cin)
    m = case_B * H * W + K + 4
    bound = m * U / (1 - m * U) * absdwc * scale
    if dq is not None:
        t = 7 * U / (1 - 7 * U)
        factor = 2.0 * (w.double().view(Cout, Cin, 3, 3) * scale).abs() * scale
        bound = bound + t * factor * dq.double().abs().view(Cout, Cin, 1, 1)
        if absdq is not None:
            bound = bound + (1 + t) * (case_B + 6) * U * factor * absdq.view(Cout, Cin, 1, 1)
    return bound


# The shapes tests/test_gpu_wgrad_edges.py runs: (B, Cin, Cout, H, W, up).  test_cpu_wgrad_plan.test_cases_cover_every_seam asserts
# what they cover between them; the comment of a case names what it is in the table for (K = number of pixel slices).
CASES = (
    (1, 8, 8, 4, 4, 0),             # K = 1
    (4, 8, 8, 1, 4, 0),             # K = 1, H = 1 (both neighbour rows out of range), the one block spans four images
    (1, 8, 8, 8, 4, 0),             # K = 2, W = 4 with H != 4
    (3, 8, 8, 3, 4, 0),             # K = 3
    (1, 8, 8, 4, 4, 1),             # up, K = 1
    (5, 16, 8, 4, 4, 1),            # up, K = 5
    (17, 6, 6, 1, 4, 1),            # up, K = 5, ragged, straddles, H = 1
    (1, 6, 6, 21, 4, 0),            # K = 6, ragged
    (1, 33, 31, 5, 4, 1),           # up, K = 2, ragged, second half-tile wave partly valid
    (1, 16, 8, 7, 8, 0),            # K = 2, ragged
    (3, 16, 8, 5, 8, 0),            # K = 4, ragged, straddles
    (3, 16, 8, 5, 8, 1),            # up, the same
    (3, 40, 24, 9, 8, 0),           # K = 7, ragged, straddles, 40 channels
    (2, 24, 40, 13, 8, 1),          # up, K = 7, ragged, straddles
    (2, 65, 70, 5, 16, 0),          # 4 tiles, K = 3, ragged, straddles
    (2, 70, 65, 5, 16, 1),          # up, the same
    (1, 8, 8, 3, 192, 0),           # three chunks per row: the middle one has a left and a right edge column
    (1, 8, 8, 3, 96, 1),            # up, three chunks per row
    (2, 16, 16, 9, 64, 1),          # up, K = 9
    (2, 192, 192, 57, 64, 0),       # 9 tiles, K = 29
    (1, 512, 512, 2, 4, 0),         # 64 tiles, K = 1; the finish kernels' grid-stride loops
    (5, 512, 512, 16, 16, 0),       # 64 tiles, K = 16 capped by 1024 / ntile
    (1, 8, 8, 3, 96, 0),            # direct kernel: 96 = 64 + 32
    (2, 8, 8, 4, 6, 0),             # direct kernel: W = 6
    (2, 6, 10, 3, 5, 1),            # up, direct kernel: odd width
    (1, 512, 512, 3, 3, 0),         # direct kernel past its 4096-block grid
)


def case_id(case):
    return 'B%d_i%d_o%d_%dx%d_%s' % (case[0], case[1], case[2], case[3], case[4], 'up' if case[5] else 'plain')

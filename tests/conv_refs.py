"""Reference machinery of tests/test_gpu_conv_edges.py: fp64 references of the fp32 convolution path (csrc/modconv.hip, csrc/wino.hip,
blur_bias_act_kernel of csrc/upfirdn2d.hip), input makers, a-priori bounds, the case lists, and host restatements of the dispatch and
staging rules.  Checked on the CPU by tests/test_cpu_conv_edges.py, so that a failure of the GPU module points at a kernel.

The references call no convolution routine: each is nine (blur / upsample: sixteen) shifted slices of the zero-padded input contracted
with einsum in fp64, and runs wherever its arguments live (the device for the large cases).  Two kinds of check, as in dense_refs.py:

  exact     small integers (x, w in [-8, 8]; s, d powers of two in {1/2, 1, 2}; integer noise, noise weight, bias; slope 1/4, gain 2):
            every partial sum is a multiple of 1/4 below 2^24 of that unit, so fp32 equals fp64 bit for bit whatever the summation order;
  bounded   synthetic.counter_tensor inputs with the per-element bound (K + c) 2^-24 (|x s| (*) |w| |d| + |noise term| + |bias|); K = the
            accumulated products, c = the other roundings on the longest path (counted at each reference below).
"""
import numpy as np
import torch

from dense_refs import F32, U, int_tensor, choice_tensor, ratio, wscale32  # noqa: F401  (re-exported for the two test modules)

PLAIN3, UP3, DOWN3 = 0, 1, 2
SLOPE, GAIN = 0.25, 2.0         # of the exact checks (both are arguments of the entry points)


# ------------------------------------------------------------------ fp64 references

def _bx(x, B):
    return x.expand(B, *x.shape[1:]) if (x.shape[0] == 1 and B != 1) else x


def _pad(x, top, bottom, left, right):
    B, C, H, W = x.shape
    out = x.new_zeros(B, C, H + top + bottom, W + left + right)
    out[:, :, top:top + H, left:left + W] = x
    return out


def _both(xs, w_t, acc, mag):
    """acc += xs . w_t, mag += |xs| . |w_t| over the channel axis (xs [B,Cin,h,w], w_t [Cin,Cout])."""
    a = torch.einsum('bihw,io->bohw', xs, w_t)
    m = torch.einsum('bihw,io->bohw', xs.abs(), w_t.abs())
    return (a if acc is None else acc + a), (m if mag is None else mag + m)


def _act(ref, bound, act, slope, gain):
    if not act:
        return ref, bound
    sl, gn = float(F32(slope)), float(F32(gain))
    ref = torch.where(ref > 0, ref, ref * sl) * gn
    return ref, bound * gn + 2.0 ** -23 * ref.abs()


apply_act = _act


def _finish(acc, mag, K, c, d, noise, noise_w, bias, act, slope, gain):
    """d * acc + noise_w * noise + bias, activation; (reference, bound).  noise [1 or B,1,h,w]; noise_w a one-element tensor."""
    if d is not None:
        dd = d.double()[:, :, None, None]
        acc, mag = acc * dd, mag * dd.abs()
    if noise is not None:
        t = noise.double() * float(noise_w.double().reshape(-1)[0])
        acc, mag = acc + t, mag + t.abs()
    if bias is not None:
        bb = bias.double()[None, :, None, None]
        acc, mag = acc + bb, mag + bb.abs()
    return _act(acc, (K + c) * U * mag, act, slope, gain)


def plain3_ref(x, wp, s, d=None, noise=None, noise_w=None, bias=None, act=False, slope=0.2, gain=2 ** 0.5, batch=None, c=8):
    """y[b,o] = act(d[b,o] sum_{i,t} (x[b,i] s[b,i])[a+ky-1, b+kx-1] wp[i,t,o] + noise_w noise + bias[o]), t = 3 ky + kx: the packed
    weight [Cin, 9, Cout] of functional.prepack as it is.  K = 9 Cin; c = 8: the pack's scale, x*s, *d, noise_w*noise, two adds, slack 2."""
    B = s.shape[0] if batch is None else batch
    H, W = x.shape[2:]
    xs = _pad(_bx(x.double(), B) * s.double()[:, :, None, None], 1, 1, 1, 1)
    wd = wp.double()
    acc = mag = None
    for t in range(9):
        ky, kx = divmod(t, 3)
        acc, mag = _both(xs[:, :, ky:ky + H, kx:kx + W], wd[:, t], acc, mag)
    return _finish(acc, mag, 9 * x.shape[1], c, d, noise, noise_w, bias, act, slope, gain)


def up3_ref(x, wp, s, d=None, batch=None, c=8):
    """Parity planes [B,Cout,4,H+1,W+1] of the stride-2 transposed conv T = conv_transpose2d(x s, w[i,o,ky,kx] = wp[i,3ky+kx,o]):
    plane 2 py + px at [a,b] = T[2a+py, 2b+px] = sum_{ky = py, kx = px (mod 2)} (x s)[a - (ky==2), b - (kx==2)] w[ky,kx].
    The entries outside the (2H+1) x (2W+1) result (a = H with py = 1, b = W with px = 1) read only the zero padding: the kernels
    store 0 there (modconv.hip:194-222 okmask, :446 of the direct kernel; blur_bias_act_kernel's load_row reads them as "stored
    zeros"), and so does this reference.  K = 4 Cin (at most 2 x 2 taps per output)."""
    B = s.shape[0] if batch is None else batch
    H, W = x.shape[2:]
    xs = _pad(_bx(x.double(), B) * s.double()[:, :, None, None], 1, 1, 1, 1)
    wd = wp.double()
    acc = [None] * 4
    mag = [None] * 4
    for t in range(9):
        ky, kx = divmod(t, 3)
        ph, dy, dx = 2 * (ky & 1) + (kx & 1), int(ky == 2), int(kx == 2)
        acc[ph], mag[ph] = _both(xs[:, :, 1 - dy:2 - dy + H, 1 - dx:2 - dx + W], wd[:, t], acc[ph], mag[ph])
    acc, mag = torch.stack(acc, 2), torch.stack(mag, 2)
    if d is not None:
        dd = d.double()[:, :, None, None, None]
        acc, mag = acc * dd, mag * dd.abs()
    return acc, (4 * x.shape[1] + c) * U * mag


def planes_outside(H, W, device='cpu'):
    """Mask [4,H+1,W+1] of the plane entries outside the (2H+1) x (2W+1) transposed-conv result."""
    m = torch.zeros(4, H + 1, W + 1, dtype=torch.bool, device=device)
    m[2:, H, :] = True
    m[1::2, :, W] = True
    return m


def planes_to_full(planes):
    """[...,4,R,P] -> T [...,2R,2P] with T[2a+py, 2b+px] = planes[2py+px, a, b]."""
    R, P = planes.shape[-2:]
    T = planes.new_zeros(*planes.shape[:-3], 2 * R, 2 * P)
    for ph in range(4):
        T[..., (ph >> 1)::2, (ph & 1)::2] = planes[..., ph, :, :]
    return T


def down3_ref(planes, wp, s, d=None, noise=None, noise_w=None, bias=None, act=False, slope=0.2, gain=2 ** 0.5, c=8):
    """planes [B,Cin,4,H+1,W+1] -> [B,Cout,H,W]: y[a,b] = sum T[2a+ky, 2b+kx] w[ky,kx], T[2a+ky, 2b+kx] = plane (ky&1, kx&1) at
    [a + (ky>>1), b + (kx>>1)] (every plane entry is data).  K = 9 Cin."""
    H, W = planes.shape[3] - 1, planes.shape[4] - 1
    ps = planes.double() * s.double()[:, :, None, None, None]
    wd = wp.double()
    acc = mag = None
    for t in range(9):
        ky, kx = divmod(t, 3)
        sl = ps[:, :, 2 * (ky & 1) + (kx & 1), (ky >> 1):(ky >> 1) + H, (kx >> 1):(kx >> 1) + W]
        acc, mag = _both(sl, wd[:, t], acc, mag)
    return _finish(acc, mag, 9 * planes.shape[1], c, d, noise, noise_w, bias, act, slope, gain)


def blur_ref(planes, fir, noise=None, noise_w=None, bias=None, act=False, slope=0.2, gain=2 ** 0.5):
    """y[oy,ox] = sum_{ky,kx < 4} Tpad[oy+ky, ox+kx] K[3-ky][3-kx] + noise_w noise + bias, activation; Tpad[i,j] = T[i-1,j-1], T the
    interleaved planes (all their entries, rows / columns 2H+1, 2W+1 included: the kernel reads them).  K = 16; c = 4 (bias, the
    noise fma, slack 2)."""
    T = planes_to_full(planes.double())                 # [B,C,2H+2,2W+2]
    H2, W2 = T.shape[2] - 2, T.shape[3] - 2
    Tp = _pad(T, 1, 0, 1, 0)
    kd = fir.double()
    acc = mag = None
    for ky in range(4):
        for kx in range(4):
            sl = Tp[:, :, ky:ky + H2, kx:kx + W2] * float(kd[3 - ky, 3 - kx])
            acc, mag = (sl, sl.abs()) if acc is None else (acc + sl, mag + sl.abs())
    return _finish(acc, mag, 16, 4, None, noise, noise_w, bias, act, slope, gain)


def upsample_ref(skip, fir):
    """upfirdn2d(skip, fir, up=2, pad=(2,1)) in fp64 with its magnitude: sample (m,n) sits at padded position (2m+2, 2n+2)."""
    B, C, Hs, Ws = skip.shape
    up = skip.new_zeros(B, C, 2 * Hs + 3, 2 * Ws + 3, dtype=torch.float64)
    up[:, :, 2:2 + 2 * Hs:2, 2:2 + 2 * Ws:2] = skip.double()
    kd = fir.double()
    acc = mag = None
    for ky in range(4):
        for kx in range(4):
            sl = up[:, :, ky:ky + 2 * Hs, kx:kx + 2 * Ws] * float(kd[3 - ky, 3 - kx])
            acc, mag = (sl, sl.abs()) if acc is None else (acc + sl, mag + sl.abs())
    return acc, mag


def torgb_ref(x, w_rgb, s, bias=None, skip=None, fir=None):
    """y[b,j] = sum_i x[b,i] s[b,i] w[j,i] / sqrtf(Cin) + bias[j] + upfirdn2d(skip, fir, up=2, pad=(2,1)).  K = Cin (+ the LDS sum of
    the channel groups, part of the same sum); c = 8: s*scale, w*that, bias, four skip fmas, slack 1."""
    cin = x.shape[1]
    wd = w_rgb.double().reshape(3, cin) * wscale32(cin)
    xs = x.double() * s.double()[:, :, None, None]
    acc, mag = _both(xs, wd.t(), None, None)
    if bias is not None:
        bb = bias.double().reshape(1, 3, 1, 1)
        acc, mag = acc + bb, mag + bb.abs()
    if skip is not None:
        a, m = upsample_ref(skip, fir)
        acc, mag = acc + a, mag + m
    return acc, (cin + 8) * U * mag


# ------------------------------------------------------------------ Winograd F(2x2, 3x3)

WG = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
WBT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
WAT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def wino_pack(w, G=WG):
    """The pack layout of prepack_wino_kernel (wino.hip:582-616) restated, without the scale: w [Cout,Cin,3,3] ->
    U[ci][o][(a ^ (o & 3)) * 4 + b] = (G w G^T)[a][b] in fp64."""
    cout, cin = w.shape[:2]
    G = G.to(w.device)
    u = torch.einsum('ak,oikl,bl->ioab', G, w.double(), G)          # [Cin,Cout,4,4]
    out = torch.empty_like(u)
    o = torch.arange(cout, device=w.device)
    for a in range(4):
        out[:, o, a ^ (o & 3)] = u[:, :, a]
    return out.reshape(cin, cout, 16)


def wino_bound(x, w, s, d=None, noise=None, noise_w=None, bias=None, batch=None, c=20):
    """The Winograd algorithm on absolute values: |A^T| ((|B^T| |x s| |B|) (.) sum_i (|G| |w| |G^T|)) |A| per 2x2 tile, times |d|, plus
    the epilogue terms, times (K + c) 2^-24.  K = Cin products per transform-domain element; c = 20: the pack (scale, 2 + 2 adds),
    the input transform (1 + 1 adds, the style), the output transform (2 + 2 adds), *d, noise_w*noise, two adds, slack 6.
    w [Cout,Cin,3,3] carries the pack's scale already."""
    B = s.shape[0] if batch is None else batch
    H, W = x.shape[2:]
    dev = x.device
    xs = _pad((_bx(x.double(), B) * s.double()[:, :, None, None]).abs(), 1, 1, 1, 1)
    pt = xs.unfold(2, 4, 2).unfold(3, 4, 2)                        # [B,Cin,TH,TW,4,4]
    Ba, Ga, Aa = WBT.abs().to(dev), WG.abs().to(dev), WAT.abs().to(dev)
    V = torch.einsum('ak,bihwkl,cl->bihwac', Ba, pt, Ba)
    Ua = torch.einsum('ak,oikl,bl->ioab', Ga, w.double().abs(), Ga)
    M = torch.einsum('bihwac,ioac->bohwac', V, Ua)
    Y = torch.einsum('pa,bohwac,qc->bohpwq', Aa, M, Aa)            # [B,Cout,TH,2,TW,2]
    mag = Y.reshape(B, w.shape[0], H, W)
    if d is not None:
        mag = mag * d.double().abs()[:, :, None, None]
    if noise is not None:
        mag = mag + (noise.double() * float(noise_w.double().reshape(-1)[0])).abs()
    if bias is not None:
        mag = mag + bias.double().abs()[None, :, None, None]
    return (x.shape[1] + c) * U * mag


def wp_of(w):
    """[Cout,Cin,3,3] -> the packed layout [Cin,9,Cout] (no scale)."""
    return w.reshape(w.shape[0], w.shape[1], 9).permute(1, 2, 0).contiguous()


# ------------------------------------------------------------------ the rules of csrc/modconv.hip and csrc/wino.hip, restated

def tile_of(mode, B, cin, cout, H, W, aligned=True):
    """sgdfr_modconv2d_fwd_f32's choice (modconv.hip:660-695): 'direct', or (NT couts, PT pixels, EX staging rows of 256)."""
    if cin % 4 or cout % 4 or not aligned:
        return 'direct'
    if mode == UP3:
        pix = B * (H + 1) * (W + 1)
        if cout % 128 == 0 and ((pix + 63) // 64) * ((cout + 127) // 128) >= 512:
            return (128, 64, 3)
        return (64, 64, 3) if cout > 32 else (32, 128, 3)
    pix = B * H * W
    if cout % 128 == 0 and ((pix + 127) // 128) * ((cout + 127) // 128) >= 512:
        return (128, 128, 3)
    if mode == PLAIN3 and cout % 64 == 0 and pix >= 256 * 1024:
        return (64, 256, 4)
    if mode == PLAIN3 and cout % 64 == 0 and pix >= 128 * 512:
        return (64, 128, 3)
    return (64, 64, 3) if cout > 32 else (32, 128, 3)


def staged(mode, PT, EX, H, W):
    """launch_modconv's staged range (modconv.hip:585-611): dict(rows, imgs, xlen, seg, ok)."""
    P, HW = W + 1, H * W
    rows = 0 if W % PT == 0 else (PT // W - 1 if PT % W == 0 else (PT - 1) // W + 1)
    imgs = 0 if HW % PT == 0 else (PT // HW - 1 if PT % HW == 0 else (PT - 1) // HW + 1)
    if mode == PLAIN3:
        xlen = (PT - 1) + rows + imgs * P + 2 * P + 3
    elif mode == DOWN3:
        xlen = (PT - 1) + rows + imgs * (P + 1) + P + 2
    else:
        rows = imgs = 0
        xlen = PT + P + 2
    seg = mode == PLAIN3 and W % PT == 0 and 3 * (PT + 2) < xlen
    if seg:
        xlen = 3 * (PT + 2)
    return dict(rows=rows, imgs=imgs, xlen=xlen, seg=seg, ok=xlen <= EX * 256)


def plan(mode, B, cin, cout, H, W):
    """('direct', None) or ((NT, PT, EX), staged(...)) of one sgdfr_modconv2d_fwd_f32 call."""
    t = tile_of(mode, B, cin, cout, H, W)
    return (t, None) if t == 'direct' else (t, staged(mode, t[1], t[2], H, W))


def first_refused_w(mode, B, cin, cout, H):
    """The smallest W whose staged range the launch rule refuses (every narrower image is accepted)."""
    W = 1
    while plan(mode, B, cin, cout, H, W)[1]['ok']:
        W += 1
    return W


def splitk_hint(B, cin, cout, H, W, mode):
    """sgdfr_modconv2d_splitk_hint (modconv.hip:836-846)."""
    if cin % 4 or cout % 4 or cout <= 32 or mode == DOWN3:
        return 1
    pix = B * (H + 1) * (W + 1) if mode == UP3 else B * H * W
    blocks = ((pix + 63) // 64) * ((cout + 63) // 64)
    if blocks >= 192:
        return 1
    s = min(1024 // blocks, cin // 4 // 8, 16)
    return 1 if s < 2 else s


def wino_span(H, W):
    """wino.hip:624-631: (span, branch) with branch 'row' | 'rows' | 'general'."""
    TW, TH, P = W // 2, H // 2, W + 2
    per = TW * TH
    if TW % 64 == 0:
        return 2 * 63, 'row'
    if 64 % TW == 0 and per % 64 == 0:
        return (64 // TW - 1) * 2 * P + 2 * (TW - 1), 'rows'
    return (63 // TW + 1) * 2 * P + (63 // per + 1) * P + 2 * (TW - 1), 'general'


def wino_xlen(H, W):
    return wino_span(H, W)[0] + 3 * (W + 2) + 4


def wino_supported(B, cin, cout, H, W):
    """sgdfr_modconv2d_wino_supported (wino.hip:645-649)."""
    if cin % 8 or cout % 64 or (H & 1) or (W & 1) or H < 2 or W < 2:
        return 0
    return int(wino_xlen(H, W) <= 1024)


def wino_simgs(H, W):
    per = (W // 2) * (H // 2)
    return 1 if per % 64 == 0 else 63 // per + 2


# ------------------------------------------------------------------ inputs

def conv_inputs(kind, mode, B, cin, cout, H, W, noise='none', bias=True, bcast=False, seed=13, lo=-8, hi=8, s_values=(0.5, 1.0, 2.0)):
    """dict(x, wp, s, d, noise, noise_w, bias) on the CPU.  kind 'int': the exact inputs; 'real': counter tensors with the weights
    in the packed layout but unscaled (F.prepack is applied by the caller where it is under test)."""
    key = 'cv.%d.%d.%d.%d.%d.%d.%s' % (mode, B, cin, cout, H, W, kind)
    xshape = (1 if bcast else B, cin, 4, H + 1, W + 1) if mode == DOWN3 else (1 if bcast else B, cin, H, W)
    oh, ow = H, W
    out = {}
    if kind == 'int':
        n = int(np.prod(xshape))            # (large inputs: int_tensor's no-equal-rows rule over rows of 256, which is quick)
        out['x'] = int_tensor(seed, key + 'x', (n // 256, 16, 16) if n >= 1 << 18 and n % 256 == 0 else xshape, lo, hi).view(xshape)
        out['wp'] = int_tensor(seed, key + 'w', (cin, 9, cout), lo, hi)
        out['s'] = choice_tensor(seed, key + 's', (B, cin), s_values)
        out['d'] = choice_tensor(seed, key + 'd', (B, cout), (0.5, 1.0, 2.0))
        for a in (out['x'], out['wp']):              # the corners a wrong halo or tail would drop are non-zero
            f = a.view(-1)
            f[0] = 5.0 if float(f[0]) == 0 else f[0]
            f[-1] = 3.0 if float(f[-1]) == 0 else f[-1]
        mk = lambda k, shape: int_tensor(seed, key + k, shape, -8, 8)       # noqa: E731
        out['noise_w'] = torch.tensor([3.0])
    else:
        from stylegan_directions_face_reenactment_amd import synthetic as S
        out['x'] = S.counter_tensor(seed, key + 'x', xshape)
        out['wp'] = S.counter_tensor(seed, key + 'w', (cin, 9, cout)) * wscale32(9 * cin)
        out['s'] = S.counter_tensor(seed, key + 's', (B, cin), 1.0, 0.3)
        out['d'] = S.counter_tensor(seed, key + 'd', (B, cout), 1.0, 0.3)
        mk = lambda k, shape: S.counter_tensor(seed, key + k, shape)         # noqa: E731
        out['noise_w'] = torch.tensor([0.3])
    out['noise'] = None if (noise == 'none' or mode == UP3) else mk('n', (1 if noise == 'shared' else B, 1, oh, ow))
    out['bias'] = mk('b', (cout, 1)).view(cout) if (bias and mode != UP3) else None
    if out['noise'] is None:
        out['noise_w'] = None
    return out


def exact_condition(cin, taps=9, x=8, w=8, s=(0.5, 2.0), d=2.0, noise=8 * 3, bias=8):
    """The a-priori condition of an exact case: taps Cin max|x s| max|w| max|d| + |noise term| + |bias| < 2^24, with the sum taken in
    units of the smallest style (s = 1/2 makes the terms half-integers: they are exact below 2^24 of THAT unit)."""
    return taps * cin * x * (s[1] / s[0]) * w * max(d, 1.0) + (noise + bias) / s[0] < 2 ** 24


# ------------------------------------------------------------------ the cases (mode, B, Cin, Cout, H, W, options)

def C(mode, B, cin, cout, H, W, **kw):
    kw.setdefault('noise', ('none', 'shared', 'per')[(B + cin + H + W) % 3] if mode == PLAIN3 else 'none')   # (modconv_raw: PLAIN3 only)
    kw.setdefault('bias', bool((cout // 4 + W) % 2))
    kw.setdefault('act', bool((cin // 4 + H) % 2))
    kw.setdefault('bcast', False)
    kw.setdefault('real', B * H * W * max(cin, cout) <= 1 << 24)     # the bounded run too (always on the small shapes)
    return dict(mode=mode, B=B, cin=cin, cout=cout, H=H, W=W, **kw)


def case_id(c):
    return '%s-B%d-%dto%d-%dx%d%s' % (('plain', 'up', 'down')[c['mode']], c['B'], c['cin'], c['cout'], c['H'], c['W'],
                                      '-bcast' if c['bcast'] else '')


STRADDLE = ((7, 1), (5, 2), (5, 3), (7, 5), (5, 19), (3, 33), (3, 63), (2, 65))          # (H, W): H W % 64 != 0 and % 128 != 0

PLAIN_TILE_CASES = [
    C(PLAIN3, 1, 4, 128, 255, 256, real=True), C(PLAIN3, 1, 4, 128, 256, 256, real=True),           # 64x64 | 128x128
    C(PLAIN3, 1, 4, 256, 255, 128), C(PLAIN3, 2, 4, 256, 128, 128),                                  # 32640 | 32768 pixels
    C(PLAIN3, 1, 4, 64, 255, 256), C(PLAIN3, 1, 4, 64, 256, 256, real=True),                         # 64x64 | 64x128
    C(PLAIN3, 3, 4, 64, 256, 256), C(PLAIN3, 4, 4, 64, 256, 256, real=True),                         # 64x128 | 64x256
    C(PLAIN3, 3, 4, 192, 256, 256), C(PLAIN3, 4, 8, 192, 256, 256),
] + [C(PLAIN3, 3, 8, co, 9, 11) for co in (4, 32, 36, 100, 132)]
PLAIN_K_CASES = [C(PLAIN3, 2, ci, 64, 24, 40) for ci in (4, 8, 12, 64)] + [C(PLAIN3, 2, 64, 32, 24, 40)]
PLAIN_STRADDLE_CASES = ([C(PLAIN3, 3, 8, co, H, W) for H, W in STRADDLE for co in (64, 32)] +
                        [C(PLAIN3, 70, 8, co, n, n) for n in (2, 3, 4) for co in (64, 32)])
PLAIN_SEG_CASES = [C(PLAIN3, 2, 8, 64, 2, 128), C(PLAIN3, 2, 8, 64, 3, 256), C(PLAIN3, 2, 8, 32, 2, 256), C(PLAIN3, 2, 8, 64, 2, 64),
                   C(PLAIN3, 2, 8, 32, 3, 128)]
PLAIN_LIMIT_CASES = [C(PLAIN3, 2, 8, 64, 3, 232), C(PLAIN3, 1, 4, 64, 64, 349), C(PLAIN3, 2, 8, 32, 3, 211), C(PLAIN3, 2, 8, 64, 1, 232)]
PLAIN_REFUSED = [(2, 8, 64, 1, 233), (2, 8, 64, 3, 233), (1, 4, 64, 64, 350), (2, 8, 32, 3, 212)]
PLAIN_BCAST_CASES = [C(PLAIN3, 5, 8, 64, 9, 11, bcast=True), C(PLAIN3, 70, 8, 32, 3, 3, bcast=True)]
PLAIN_CASES = PLAIN_TILE_CASES + PLAIN_K_CASES + PLAIN_STRADDLE_CASES + PLAIN_SEG_CASES + PLAIN_LIMIT_CASES + PLAIN_BCAST_CASES

DIRECT_CASES = [C(m, 3, ci, co, 7, 9) for m in (PLAIN3, UP3, DOWN3) for ci, co in ((6, 10), (10, 6), (5, 4))]
DIRECT_STRIDE_CASE = C(PLAIN3, 2, 5, 6, 300, 300)           # 1,080,000 outputs > 4096 blocks x 256 threads

UP_CASES = [
    C(UP3, 2, 4, 128, 127, 126), C(UP3, 2, 4, 128, 127, 127, real=True),              # 32512 | 32768 super-pixels: 64x64 | 128x64
    C(UP3, 3, 8, 64, 9, 11), C(UP3, 3, 8, 32, 9, 11), C(UP3, 3, 8, 36, 5, 19), C(UP3, 3, 8, 132, 5, 19),
    C(UP3, 3, 8, 64, 1, 37), C(UP3, 3, 8, 64, 37, 1), C(UP3, 3, 8, 32, 1, 1), C(UP3, 5, 12, 64, 3, 65, bcast=True),
    C(UP3, 2, 4, 64, 1, 700), C(UP3, 2, 4, 64, 1, 701), C(UP3, 2, 4, 32, 1, 637),
]
UP_REFUSED = [(2, 4, 64, 1, 702), (2, 4, 32, 1, 638)]

DOWN_CASES = [
    C(DOWN3, 1, 4, 128, 255, 256), C(DOWN3, 1, 4, 128, 256, 256, real=True),          # 64x64 | 128x128
    C(DOWN3, 3, 8, 64, 9, 11), C(DOWN3, 3, 8, 32, 9, 11), C(DOWN3, 3, 12, 36, 5, 19),
] + [C(DOWN3, 3, 8, co, H, W) for H, W in ((7, 1), (5, 3), (3, 33), (2, 65)) for co in (64, 32)] + [
    C(DOWN3, 70, 8, 64, 2, 2), C(DOWN3, 2, 8, 64, 3, 349), C(DOWN3, 2, 8, 32, 3, 317),
]
DOWN_REFUSED = [(2, 8, 64, 3, 350), (2, 8, 32, 3, 318)]

# split-K through modconv_raw (use_splitk on): (mode, B, Cin, Cout, H, W, bcast, splits the hint must give)
SPLITK_RAW_CASES = [(PLAIN3, 2, 64, 64, 8, 8, False, 2), (UP3, 2, 64, 64, 8, 8, False, 2), (PLAIN3, 2, 68, 64, 8, 8, False, 2),
                    (UP3, 2, 68, 64, 7, 7, False, 2), (PLAIN3, 1, 512, 512, 4, 4, True, 16), (UP3, 1, 512, 512, 4, 4, True, 16),
                    (PLAIN3, 191, 160, 64, 8, 8, False, 5), (PLAIN3, 192, 160, 64, 8, 8, False, 1)]
# straight through sgdfr_modconv2d_splitk_f32: (mode, B, Cin, Cout, H, W, splits)
SPLITK_DIRECT_CASES = [(PLAIN3, 3, 16, 64, 5, 7, 4), (UP3, 3, 16, 64, 5, 7, 4), (PLAIN3, 3, 64, 64, 5, 7, 3), (UP3, 3, 64, 36, 5, 7, 3),
                       (PLAIN3, 3, 64, 100, 9, 11, 16)]

BLUR_H = (1, 2, 3, 4, 5, 8, 9)
BLUR_W = (1, 2, 3, 31, 32, 33, 64)
BLUR_STRIDE_CASE = (17, 256, 1, 512)        # B, C, H, W: B C = 4352 > 4096 planes of 512 strips = 2,228,224 strips > 4096 x 256 x 2

TORGB_CASES = [  # (B, Cin, H, W, skip, bias)
    (2, 16, 5, 5, False, True), (2, 16, 1, 1, False, True), (2, 4, 1, 3, False, False), (2, 64, 2, 2, True, True),
    (2, 16, 1, 5, False, True), (2, 3, 2, 8, True, True), (2, 20, 4, 4, True, False), (2, 256, 6, 42, True, True),
    (2, 64, 16, 16, True, True), (2, 512, 10, 26, True, True), (3, 4, 2, 6, True, True), (2, 16, 4, 5, False, True),
    (2, 256, 16, 16, False, False), (2, 512, 4, 4, True, True),
]
TORGB_EXACT_CIN = (4, 16, 64, 256)

WINO_SHAPES = [  # (B, H, W): every branch of wino_span
    (2, 2, 128), (2, 2, 256), (2, 16, 16), (2, 16, 32), (2, 64, 64), (70, 2, 2), (5, 4, 4), (3, 6, 6), (5, 8, 8), (2, 40, 40),
    (2, 6, 100), (3, 2, 130), (2, 2, 144),
]
WINO_CHANNELS = ((8, 64), (16, 128), (64, 64))
WINO_REFUSED = [(2, 2, 258), (2, 2, 146), (2, 4, 148)]


def wino_cases():
    """(B, Cin, Cout, H, W, noise kind, bcast): every shape at (8, 64), a few at the other channel counts, noise kinds rotating."""
    out = []
    for n, (B, H, W) in enumerate(WINO_SHAPES):
        out.append((B, 8, 64, H, W, ('none', 'shared', 'per')[n % 3], False))
    out += [(2, 16, 128, 16, 16, 'per', False), (2, 64, 64, 6, 100, 'shared', False), (5, 16, 128, 8, 8, 'shared', True),
            (70, 64, 128, 2, 2, 'per', False), (3, 64, 64, 40, 40, 'none', True)]
    return out


def wino_exact_condition(cin, x=4, s=2, wk=2):
    """|V| <= 16 max|x| ... in fact each entry of B^T x B sums four inputs: 4 x s; |U| <= 9/4 max|w| = 9 wk for w = 4 [-wk, wk];
    the transform-domain sums over Cin and the nine-term output transform stay below 2^24."""
    return 9 * cin * (4 * x * s) * (9 * wk) < 2 ** 24

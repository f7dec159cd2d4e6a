"""Reference machinery of tests/test_gpu_dense_edges.py: inputs, fp64 references, a-priori bounds, host restatements.

Everything here runs on the CPU (numpy / torch-CPU) and is itself checked by tests/test_cpu_dense_edges.py, so that a failure of the GPU
module points at a kernel and not at the test.  Two kinds of check are served:

  exact     small-integer inputs: every product and every partial sum is an integer (or a dyadic fraction) below 2^24, so the fp32
            result does not depend on summation order or fma contraction and must equal the fp64 reference bit for bit;
  bounded   real inputs (synthetic.counter_tensor) against fp64 with the per-element bound
                |y - ref| <= (K + 8) * 2^-24 * (|x| @ |w|^T * |wscale| + |bias| * |bscale|),
            rigorous for any fp32 summation order of K terms (K - 1 additions, K products; 8 roundings left for scales, bias and casts).
"""
import itertools

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32
F32 = np.float32


# ------------------------------------------------------------------ inputs

def _rng(seed, key):
    import zlib
    return np.random.default_rng([int(seed), zlib.crc32(key.encode()) & 0xFFFFFFFF])


def int_tensor(seed, key, shape, lo=-8, hi=8, nonzero=False):
    """Seeded integers in [lo, hi] as fp32, 2-D (rows, cols): no all-zero row, and no two equal rows / no two equal columns wherever
    the value range has room for that (rows of one or two elements cannot all differ: there adjacent rows differ), so that a swapped
    or shifted row or column changes the answer.  Other ranks: flattened to (shape[0], -1) for the row rule only."""
    rng = _rng(seed, key)
    rows = int(shape[0]) if len(shape) else 1
    cols = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    vals = np.array([v for v in range(lo, hi + 1) if not (nonzero and v == 0)])

    def fix(a):             # resample duplicated / all-zero rows of a (in place), a few rounds
        room = a.shape[1] * np.log(len(vals)) >= np.log(8.0 * a.shape[0])
        for _ in range(64):
            bad = ~a.any(1)
            if room:
                _, first, inv = np.unique(a, axis=0, return_index=True, return_inverse=True)
                dup = np.ones(a.shape[0], bool)
                dup[first] = False
                bad |= dup
            else:
                bad[1:] |= (a[1:] == a[:-1]).all(1)
            if not bad.any():
                return
            a[bad] = rng.choice(vals, size=(int(bad.sum()), a.shape[1]))
        raise AssertionError('int_tensor: no discriminating fill for %s' % (shape,))

    a = rng.choice(vals, size=(rows, cols))
    fix(a)
    if len(shape) == 2 and rows > 1 and cols > 1:
        for _ in range(8):
            at = np.ascontiguousarray(a.T)
            fix(at)
            a = np.ascontiguousarray(at.T)
            before = a.copy()
            fix(a)
            if (a == before).all():
                break
    return torch.from_numpy(a.astype(np.float32).reshape(tuple(shape)))


def choice_tensor(seed, key, shape, values):
    rng = _rng(seed, key)
    return torch.from_numpy(rng.choice(np.asarray(values, np.float32), size=tuple(shape)).astype(np.float32))


# ------------------------------------------------------------------ F.linear: the sweep and its dispatch rule

LIN_M = (1, 3, 4, 5, 127, 128, 129)
LIN_K = (1, 63, 64, 65, 511, 512, 513)
LIN_N = (1, 63, 64, 65, 67)


def is_skinny(M, K, N):
    """The dispatch rule of sgdfr_linear_f32 as the issue states it (not read from the kernel)."""
    return M <= 128 and K <= 512 and N >= 64


def linear_cases():
    """About 50 of the 245 (M, K, N): every value of every axis, every pair of values of two axes (a greedy pairwise cover), and both
    sides of each of the three dispatch thresholds with the other two conditions held true."""
    want = [(128, 512, 64), (129, 512, 64), (128, 513, 64), (128, 512, 63), (1, 1, 1), (1, 1, 64), (129, 513, 67), (5, 65, 65),
            (3, 511, 67), (4, 64, 64), (127, 63, 65), (5, 512, 67)]
    pairs = set()
    for (ia, a), (ib, b) in itertools.combinations(enumerate((LIN_M, LIN_K, LIN_N)), 2):
        pairs |= {(ia, va, ib, vb) for va in a for vb in b}

    def cov(c):
        return {(ia, c[ia], ib, c[ib]) for ia, ib in ((0, 1), (0, 2), (1, 2))}
    for c in want:
        pairs -= cov(c)
    every = list(itertools.product(LIN_M, LIN_K, LIN_N))
    while pairs:
        best = max(every, key=lambda c: (len(cov(c) & pairs), -every.index(c)))
        want.append(best)
        pairs -= cov(best)
    return want


def linear_inputs(kind, M, K, N, seed=7):
    """(x [M,K], w [N,K], b [N]) of a sweep case: kind 'int' (integers in [-8, 8]; the corner elements, which a wrong tail would drop,
    are non-zero) or 'real' (synthetic.counter_tensor)."""
    key = 'lin.%d.%d.%d' % (M, K, N)
    if kind == 'real':
        from stylegan_directions_face_reenactment_amd import synthetic as S
        return S.counter_tensor(seed, key + 'x', (M, K)), S.counter_tensor(seed, key + 'w', (N, K)), S.counter_tensor(seed, key + 'b', (N,))
    x, w = int_tensor(seed, key + 'x', (M, K)), int_tensor(seed, key + 'w', (N, K))
    for a, v in ((x, 5.0), (w, 3.0)):
        for i in (0, -1):
            for j in (0, -1):
                if float(a[i, j]) == 0.0:
                    a[i, j] = v
    return x, w, int_tensor(seed, key + 'b', (N, 1)).view(N)


def linear_ref(x, w, b=None, wscale=1.0, bscale=1.0, lrelu=False, slope=0.2, gain=2 ** 0.5):
    """(fp64 reference, per-element bound) of F.linear.  Scales, slope and gain are taken at the fp32 values the C ABI receives."""
    ws, bs, sl, gn = (float(F32(v)) for v in (wscale, bscale, slope, gain))
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t() * ws
    mag = xd.abs() @ wd.abs().t() * abs(ws)
    if b is not None:
        ref = ref + b.double() * bs
        mag = mag + b.double().abs() * abs(bs)
    bound = (x.shape[-1] + 8) * U * mag
    if lrelu:
        ref = torch.where(ref > 0, ref, ref * sl) * gn
        bound = bound * gn + 2.0 ** -23 * ref.abs()
    return ref, bound


def ratio(y, ref, bound):
    """Worst error / bound over the elements (0/0 counts as 0: an exact zero under a zero bound is right)."""
    err = (y.detach().double().cpu() - ref.cpu()).abs()
    bound = bound.cpu()
    assert bool((err[bound == 0] == 0).all()), 'error under a zero bound'
    r = err / bound.clamp_min(1e-300)
    return float(r[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def ulps(y, ref64):
    """Worst distance of fp32 y from the fp64 value ref64, in units of the fp32 spacing at ref64."""
    y, ref64 = y.detach().double().cpu(), ref64.cpu()
    sp = torch.from_numpy(np.spacing(np.abs(ref64.numpy()).astype(np.float32)).astype(np.float64))
    return float(((y - ref64).abs() / sp).max())


# ---- the two accumulation orders, emulated in numpy float32 (fma = one rounding of the fp64 product-sum, exact for fp32 operands)

def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_skinny(x, w, drop=None):
    """linear_skinny_kernel's order: lane-strided fma over k = lane + 64 j, then the 6-step xor butterfly over the 64 lanes (lane i
    takes lane i ^ 32, then ^ 16, ... ^ 1; every lane ends with the same sum, as fp32 addition commutes).
    drop = (m, n, k): that one product is left out (a kernel with a wrong tail)."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    M, K = x.shape
    N = w.shape[0]
    lanes = np.zeros((M, N, 64), np.float32)
    for j in range((K + 63) // 64):
        ks = np.arange(64 * j, min(64 * j + 64, K))
        xa = np.zeros((M, 1, 64), np.float32)
        wa = np.zeros((1, N, 64), np.float32)
        xa[:, 0, :len(ks)] = x[:, ks]
        wa[0, :, :len(ks)] = w[:, ks]
        prod_x = np.broadcast_to(xa, (M, N, 64)).copy()
        if drop is not None and 64 * j <= drop[2] < 64 * j + 64:
            prod_x[drop[0], drop[1], drop[2] - 64 * j] = 0
        lanes = _fma32(prod_x, np.broadcast_to(wa, (M, N, 64)), lanes)
    while lanes.shape[-1] > 1:
        h = lanes.shape[-1] // 2
        lanes = (lanes[..., :h] + lanes[..., h:]).astype(np.float32)
    return lanes[..., 0]


def emulate_tiled(x, w, drop=None):
    """linear_kernel's order: one fma chain, serial over k."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k in range(x.shape[1]):
        xa = np.broadcast_to(x[:, k:k + 1], acc.shape)
        if drop is not None and drop[2] == k:
            xa = xa.copy()
            xa[drop[0], drop[1]] = 0
        acc = _fma32(xa, np.broadcast_to(w[None, :, k], acc.shape), acc)
    return acc


def epilogue32(acc, b, wscale, bscale):
    """EPI 0 without activation in float32: acc * wscale + bias * bscale (two roundings, or one when contracted: the bound covers both)."""
    y = (acc * F32(wscale)).astype(np.float32)
    if b is not None:
        y = (y + (np.asarray(b, np.float32) * F32(bscale)).astype(np.float32)).astype(np.float32)
    return y


# ------------------------------------------------------------------ styles: structured integer layers, references

def wscale32(D):
    """1 / sqrt(D) as the host side of the library forms it (fp32 sqrt, fp32 divide)."""
    return float(F32(1.0) / np.sqrt(F32(D)))


def pow4(D):
    return D in (4, 16, 64, 256, 1024)


def structured_style_layer(seed, key, D, cin, cout):
    """(mod_w, mod_b, q) with which integer styles in [-2, 2] give integer s in [-4, 4] with a non-zero entry in every row, and integer
    q in [1, 4]: sum s^2 q is then an exact integer >= 1.  D a power of four: one entry sqrt(D) per weight row (s varies with the image);
    otherwise zero weights (s = bias for every image)."""
    mw = torch.zeros(cin, D)
    if pow4(D):
        mw[torch.arange(cin), (torch.arange(cin) * 7 + 3) % D] = float(int(round(D ** 0.5)))
    mb = int_tensor(seed, key + '.b', (cin, 1), -2, 2).view(cin)
    mw[0] = 0.0
    mb[0] = 3.0             # s[:, 0] = 3 for every image: no all-zero row
    q = int_tensor(seed, key + '.q', (cout, cin), 1, 4) if cout else None
    return mw, mb, q


def style_ref(style, mw, mb, D):
    """fp64 s (with its bound) of a modulation; the demodulation is referenced from the device's own s (demod_ref)."""
    ref, bound = linear_ref(style, mw, mb, wscale=wscale32(D))
    return ref, bound


def demod_ref(s_dev, q):
    """(fp64 d from the device's fp32 s, relative bound): d = rsqrt(sum_i s^2 q + 1e-8); the argument's bound propagates through
    the rsqrt with the factor 1/2, plus 4 ulp for the argument's rounding, the hardware rsqrt and the result."""
    s2 = s_dev.detach().double().cpu() ** 2
    qd = q.detach().double().cpu()
    acc = s2 @ qd.t() + float(F32(1e-8))
    bound_acc = (s2.shape[1] + 8) * U * (s2 @ qd.abs().t())
    return acc.rsqrt(), 0.5 * bound_acc / acc + 4 * 2.0 ** -23


# ------------------------------------------------------------------ the range-exponent rule (include/sgdfr.h, sgdfr_style_layer)

def _floor_log2_bits(bits):
    return max(int(bits) >> 23, 1) - 127         # subnormals count as 2^-126


def range_exponent(max_s, headroom, x_log2=None, word=None):
    """e = clamp(18 - headroom - L - floor(log2 max|s|), +-120); L = x_log2, or floor(log2 max|x|) + 1 from an absmax word.
    e = 0 for an all-zero or non-finite style row and for a zero or non-finite word."""
    mb = int(np.asarray(max_s, np.float32).view(np.uint32)) & 0x7fffffff
    if mb == 0 or mb >= 0x7f800000:
        return 0
    L = x_log2
    if word is not None:
        word = int(word) & 0xffffffff
        if word == 0 or word >= 0x7f800000:
            return 0
        L = _floor_log2_bits(word) + 1
    return min(max(18 - int(headroom) - int(L) - _floor_log2_bits(mb), -120), 120)


def apply_range(s, d, headroom, x_log2=None, word=None):
    """(s * 2^e, d * 2^-e, e) per row, from fp32 tensors on the host, with exact ldexp."""
    s_, d_ = s.detach().cpu().numpy(), d.detach().cpu().numpy()
    e = np.array([range_exponent(np.abs(r).max(), headroom, x_log2, word) for r in s_], np.int32)
    return torch.from_numpy(np.ldexp(s_, e[:, None])), torch.from_numpy(np.ldexp(d_, -e[:, None])), e


# ------------------------------------------------------------------ backward of the batched styles (fp64 expressions)

def style_bwd_layer_ds(kind, e):
    """dL/ds of one layer of functional.styles_batched_bwd in fp64: kind 'rgb' | 'plain' | 'demod' (autograd.ToRGBFn / StyledConvFn /
    StyleFn backward)."""
    cin = e['mod_w'].shape[0]
    if kind == 'rgb':
        return (e['rgb_r'].double() * e['rgb_w'].double().unsqueeze(0)).sum(1) / cin ** 0.5
    if kind == 'plain':
        return e['gs'].double()
    a, d = e['a'].double(), e['d'].double()
    return e['gs'].double() + e['s'].double() * ((-(a / d) * d ** 3) @ e['qt'].double().t())


def style_bwd_reference(layers, latent, B, L, D):
    """layers: [(kind, entry dict)].  Returns (glat [B,L,D], [(ds, gmod_w, gmod_b)] per layer) in fp64."""
    want = torch.zeros(B, L, D, dtype=torch.float64, device=latent.device)
    per = []
    for kind, e in layers:
        ds = style_bwd_layer_ds(kind, e)
        want[:, e['latent_index']] += ds @ e['mod_w'].double() / D ** 0.5
        per.append((ds, ds.t() @ latent[:, e['latent_index']].double() / D ** 0.5, ds.sum(0)))
    return want, per


def style_bwd_ds_bound(kind, e):
    """A-priori bound of the fp32 ds of one layer (same shape as ds)."""
    cin = e['mod_w'].shape[0]
    if kind == 'rgb':
        return 8 * U * (e['rgb_r'].double().abs() * e['rgb_w'].double().abs().unsqueeze(0)).sum(1) / cin ** 0.5
    if kind == 'plain':
        return torch.zeros_like(e['gs'], dtype=torch.float64)
    a, d = e['a'].double(), e['d'].double()
    v = ((a / d) * d ** 3).abs()
    return (d.shape[1] + 8) * U * (e['gs'].double().abs() + e['s'].double().abs() * (v @ e['qt'].double().abs().t()))


def demod_dq_reference(a, d, s):
    coeff = (a.double() / d.double()) * d.double() ** 3 * -0.5
    return coeff.t() @ (s.double() ** 2)


# ------------------------------------------------------------------ uint8 packing

def _ord(x):
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7fffffff))


def _unord(o):
    o = np.asarray(o, np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(np.float32)


def u8_np32(x):
    """uint8((clamp(v, -1, 1) + 1) / (2 + 1e-5) * 255) in IEEE float32 (libs/utilities/image_utils.py:87-110 as the kernel states it)."""
    v = np.clip(np.asarray(x, np.float32), F32(-1), F32(1)).astype(np.float32)
    return ((v + F32(1)) / (F32(2) + F32(1e-5)) * F32(255)).astype(np.float32).astype(np.uint8)


def u8_torch32(x):
    v = torch.as_tensor(np.asarray(x, np.float32)).clamp(-1.0, 1.0)
    return ((v + 1.0) / torch.tensor(2.0, dtype=torch.float32).add(torch.tensor(1e-5, dtype=torch.float32)) * 255.0).to(torch.uint8).numpy()


def u8_f64(x):
    v = np.clip(np.asarray(x, np.float32).astype(np.float64), -1.0, 1.0)
    return ((v + 1.0) / (2.0 + 1e-5) * 255.0).astype(np.uint8)


_PROBES = []


def u8_probe_set():
    """For every k in 1..254 the smallest fp32 v whose byte is >= k (bisection over the ordered fp32 values, numpy float32 evaluation)
    with its three fp32 neighbours on each side, then +-1, +-(1 + 2^-23), +-5, +-0.0 and the smallest subnormals: 1788 values."""
    if _PROBES:
        return _PROBES[0]
    out = []
    for k in range(1, 255):
        lo, hi = int(_ord(F32(-1))), int(_ord(F32(1)))          # byte(lo) < k <= byte(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if int(u8_np32(_unord(mid))) >= k:
                hi = mid
            else:
                lo = mid
        out.extend(_unord(np.arange(hi - 3, hi + 4)).tolist())
    tiny = float(np.float32(1e-45))
    out += [1.0, -1.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 5.0, -5.0, 0.0, -0.0, tiny, -tiny]
    _PROBES.append(np.asarray(out, np.float32))
    return _PROBES[0]


def u8_image(B, H, W, offset=0):
    """[B,3,H,W] fp32 filled cyclically with the probe set (starting at `offset`)."""
    p = u8_probe_set()
    n = B * 3 * H * W
    idx = (np.arange(n) + offset) % len(p)
    return p[idx].reshape(B, 3, H, W)


def u8_grid_host(panels, B, swap_rb):
    """Host assembly of grid_frames_uint8: panels = list of [B or 1,3,H,W] float32 arrays or None -> ([B,H,K*W,3] uint8, written mask)."""
    H, W = next(p for p in panels if p is not None).shape[2:]
    out = np.zeros((B, H, len(panels) * W, 3), np.uint8)
    mask = np.zeros(out.shape, bool)
    for k, p in enumerate(panels):
        if p is None:
            continue
        img = np.broadcast_to(u8_np32(p), (B, 3, H, W)).transpose(0, 2, 3, 1)
        out[:, :, k * W:(k + 1) * W] = img[..., ::-1] if swap_rb else img
        mask[:, :, k * W:(k + 1) * W] = True
    return out, mask


# ------------------------------------------------------------------ Adam (torch/optim/adam.py _single_tensor_adam, fp64)

class Adam64:
    """fp64 restatement of torch.optim.Adam (default betas / eps, no weight decay, one step count per parameter).
    shared_count=True is FusedAdam's variant: ONE count for all parameters, which moves once per step in which any parameter has a
    gradient; a parameter skipped at some steps then takes the bias correction of the shared count, not of its own."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, shared_count=False):
        self.p = [p.detach().double().cpu().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.shared, self.count = shared_count, 0
        self.lr, self.betas, self.eps = lr, betas, eps

    def step(self, grads):
        b1, b2 = self.betas
        self.count += any(g is not None for g in grads)
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.detach().double().cpu()
            self.t[i] = self.count if self.shared else self.t[i] + 1
            self.m[i] = self.m[i] + (g - self.m[i]) * (1 - b1)
            self.v[i] = self.v[i] * b2 + (1 - b2) * g * g
            bc1, bc2 = 1 - b1 ** self.t[i], 1 - b2 ** self.t[i]
            denom = self.v[i].sqrt() / bc2 ** 0.5 + self.eps
            self.p[i] = self.p[i] - (self.lr / bc1) * (self.m[i] / denom)


ADAM_SIZES = (1, 255, 256, 1023, 1024, 1025, 2049, 4097)


# ------------------------------------------------------------------ pixel norm

PIXELNORM_EPS = float(F32(1e-8))


def pixelnorm_ref(x, g):
    """fp64 autograd of x * rsqrt(mean(x^2) + 1e-8): (y, dL/dx for the upstream gradient g)."""
    xr = x.double().requires_grad_(True)
    y = xr * torch.rsqrt((xr ** 2).mean(1, keepdim=True) + PIXELNORM_EPS)
    y.backward(g.double())
    return y.detach(), xr.grad


def pixelnorm_bar(D):
    """Relative to max |ref| per row: D/64 serial adds per lane, the 6-step butterfly, the rsqrt and the final products."""
    return (D / 64 + 16) * 2.0 ** -23


def pixelnorm_bwd_emulated(x, g, form):
    """The gradient kernel's arithmetic on the host.  form 'difference': r*g - x*r^3*mean(g*x) in float32 (its two terms cancel to
    eps*r^2 of their size along x); form 'eps-apart': r^3 * (eps*g + (g*sum x^2 - x*sum g*x)/D) with sums and combination in float64."""
    D = x.shape[1]
    if form == 'difference':
        x, g = np.asarray(x, np.float32), np.asarray(g, np.float32)
        sq = (x * x).sum(1, keepdims=True, dtype=np.float32)
        gx = (g * x).sum(1, keepdims=True, dtype=np.float32)
        r = (1.0 / np.sqrt((sq / F32(D) + F32(1e-8)).astype(np.float64))).astype(np.float32)
        c = r * r * r * (gx / F32(D))
        return (r * g).astype(np.float32) - (x * c).astype(np.float32)
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    sq, gx = (x * x).sum(1, keepdims=True), (g * x).sum(1, keepdims=True)
    r = 1.0 / np.sqrt(sq / D + PIXELNORM_EPS)
    return (r ** 3 * (PIXELNORM_EPS * g + (g * sq - x * gx) / D)).astype(np.float32)

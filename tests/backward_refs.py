"""Reference machinery of tests/test_gpu_backward_edges.py: fp64 references of the bandwidth-bound backward helpers (csrc/backward.hip
and blur_adjoint_split_kernel of csrc/upfirdn2d.hip), input makers, a-priori bounds, the case lists, and host restatements of the
launch rules.  Checked on the CPU by tests/test_cpu_backward_edges.py, so that a failure of the GPU module points at a kernel.

The references are plain tensor expressions in float64 and run wherever their arguments live (the device for the grid-stride
cases).  Two kinds of check, as in conv_refs.py:

  exact     small integers, gain 2, slope 1/4, scales that are powers of two, channel counts in {4, 16, 64} (1/sqrt(C) a power of
            two), integer FIRs: every product and every partial sum is a multiple of one power of two below 2^24 of that unit, so
            the fp32 result is the fp64 one bit for bit whatever the order of the lanes, the wave tree and the atomics;
  bounded   synthetic.counter_tensor inputs, gain sqrt(2), slope 0.2, with (K + c) 2^-24 magnitude: elementwise K = the added
            terms and the magnitude is the same expression on absolute values; reductions K = the depth the code gives (a lane's
            serial terms, the six-level wave tree, one atomic per further partial) and the magnitude is the sum of |terms|.
"""
import numpy as np
import torch

from dense_refs import F32, U, _rng, choice_tensor, ratio, wscale32  # noqa: F401  (re-exported for the two test modules)

SLOPE, GAIN = 0.25, 2.0          # of the exact checks
CHUNK = 2048                     # kChunk of csrc/backward.hip: elements of a plane that one wave handles
GJ_CPW = 4                       # channels per wave of grad_join_rgb_kernel
ADJ_QV = 4                       # super-pixel rows per strip (blur_adjoint_kernel) and per tile (BLUR_QV, the split kernel)
ADJ_GRID_CAP = 256 * 32          # blocks of either blur adjoint before its grid-stride loop starts
PREPACK_GRID_CAP = 4096


# ------------------------------------------------------------------ depth of the per-plane reductions

def chunks_of(HW):
    return (HW + CHUNK - 1) // CHUNK


def wave_depth(HW):
    """Additions on the longest path of a wave-per-chunk sum: a lane adds ceil(min(HW, 2048) / 64) terms in sequence (the float4
    kernels 8 x 4 of them: the same count), the xor tree has six levels, and chunks - 1 atomics follow the first."""
    return (min(HW, CHUNK) + 63) // 64 + 6 + chunks_of(HW) - 1


def adjoint_depth(H, W):
    """asum of both blur adjoints, the worst order the code allows: 16 roundings in each gT, up to 24 serial fmas in a thread (the
    split kernel's thread of column W - 1 owns column W too), six tree levels, and one atomic per STRIP of the plane: the per-lane
    atomic path of blur_adjoint_kernel."""
    return 16 + 24 + 6 + ((H + 1 + ADJ_QV - 1) // ADJ_QV) * (W + 1)


# ------------------------------------------------------------------ fp64 references

def _f(v):
    return float(F32(v))


def _noise_term(noise, noise_w, B):
    if noise is None:
        return None, 0.0
    nz = noise.double()
    return (nz.expand(B, *nz.shape[1:]) if nz.shape[0] == 1 else nz), float(noise_w.double().reshape(-1)[0])


def act_grad_ref(g, out, noise=None, noise_w=None, bias=None, slope=0.2, gain=2 ** 0.5, want_y=True, g_mag=None, kc=3):
    """act_grad_reduce_kernel: g_pre = g (out > 0 ? 1 : slope) gain -- at out == 0 the factor is `slope`, as the kernel's
    `o > 0.f ? 1 : slope`; sums[b,c] = (sum g_pre, sum g_pre noise, sum g_pre y), y = out / (out > 0 ? gain : gain slope)
    - noise_w noise - bias (y = -noise_w noise - bias at out == 0); sums[..., 2] = 0 without want_y.
    Returns dict(g_pre, sums, b_pre, b_sums).  g_mag: the magnitude of g (|g| when g is an input, the sum of |terms| when it was
    formed by grad_join); kc = K + c of g_pre: K = 1 term, c = 2: the products with slope and with gain.
    The sums: K = wave_depth(HW), c = kc (each term carries g_pre's roundings; the fmas add none) and, for the third, 7 more:
    1/gain or 1/(gain slope) (2), out * that, noise_w * noise, the two subtractions, slack 1."""
    B, C = out.shape[:2]
    HW = out.shape[2] * out.shape[3]
    sl, gn = _f(slope), _f(gain)
    o, gd = out.double(), g.double()
    fac = torch.where(o > 0, torch.ones_like(o), torch.full_like(o, sl)) * gn
    g_pre = gd * fac
    m_pre = (gd.abs() if g_mag is None else g_mag) * fac
    nz, nw = _noise_term(noise, noise_w, B)
    bb = bias.double().view(1, C, 1, 1) if bias is not None else None
    sums = torch.zeros(B, C, 3, dtype=torch.float64, device=out.device)
    mags = torch.zeros_like(sums)
    sums[..., 0], mags[..., 0] = g_pre.sum((2, 3)), m_pre.sum((2, 3))
    if nz is not None:
        sums[..., 1], mags[..., 1] = (g_pre * nz).sum((2, 3)), (m_pre * nz.abs()).sum((2, 3))
    if want_y:
        pre = o / torch.where(o > 0, torch.full_like(o, gn), torch.full_like(o, gn * sl))
        y, ym = pre, pre.abs()
        if nz is not None:
            y, ym = y - nw * nz, ym + abs(nw) * nz.abs()
        if bb is not None:
            y, ym = y - bb, ym + bb.abs()
        sums[..., 2], mags[..., 2] = (g_pre * y).sum((2, 3)), (m_pre * ym).sum((2, 3))
    depth = wave_depth(HW)
    kcs = torch.tensor([depth + kc, depth + kc, depth + kc + 7], dtype=torch.float64, device=out.device)
    return dict(g_pre=g_pre, sums=sums, b_pre=kc * U * m_pre, b_sums=kcs * U * mags)


def grad_join_ref(out, gu=None, s_next=None, g_rgb=None, w_rgb=None, s_rgb=None, g_add=None, noise=None, noise_w=None, bias=None,
                  slope=0.2, gain=2 ** 0.5, want_y=True):
    """grad_join: g = gu s_next + s_rgb sum_j (w_rgb[j,c] / sqrtf(C)) g_rgb[b,j] + g_add (any non-empty subset), then act_grad_ref;
    r_next[b,c] = sum out gu, r_rgb[b,j,c] = sum out g_rgb[b,j].  g_pre: K = the added terms (1 + 3 + 1), c = 4: the products
    with rgb_scale, s_rgb, slope and gain.  r_next, r_rgb: K = wave_depth(HW), c = 0 (fmas of the inputs)."""
    B, C = out.shape[:2]
    HW = out.shape[2] * out.shape[3]
    o = out.double()
    g = torch.zeros_like(o)
    mag = torch.zeros_like(o)
    K = 0
    res = {}
    depth = wave_depth(HW)
    if gu is not None:
        t = gu.double() * s_next.double()[:, :, None, None]
        g, mag, K = g + t, mag + t.abs(), K + 1
        res['r_next'] = (o * gu.double()).sum((2, 3))
        res['b_next'] = depth * U * (o * gu.double()).abs().sum((2, 3))
    if g_rgb is not None:
        wd = w_rgb.double().reshape(3, C) * wscale32(C)
        gr = g_rgb.double()
        sr = s_rgb.double()[:, :, None, None]
        g = g + sr * torch.einsum('jc,bjhw->bchw', wd, gr)
        mag = mag + sr.abs() * torch.einsum('jc,bjhw->bchw', wd.abs(), gr.abs())
        K += 3
        res['r_rgb'] = torch.einsum('bchw,bjhw->bjc', o, gr)
        res['b_rgb'] = depth * U * torch.einsum('bchw,bjhw->bjc', o.abs(), gr.abs())
    if g_add is not None:
        g, mag, K = g + g_add.double(), mag + g_add.double().abs(), K + 1
    assert K, 'grad_join_ref: no incoming gradient term'
    res.update(act_grad_ref(g, out, noise, noise_w, bias, slope, gain, want_y, g_mag=mag, kc=K + 4))
    return res


def scale_reduce_ref(gu, x, s):
    """dx = gu s[b,c] (K = 1, c = 0: one product), r[b,c] = sum x gu (x [1,C,H,W] broadcasts; K = wave_depth(HW), c = 0)."""
    gd, xd = gu.double(), x.double()
    dx = gd * s.double()[:, :, None, None]
    HW = gu.shape[2] * gu.shape[3]
    return dict(dx=dx, r=(xd * gd).sum((2, 3)), b_dx=U * dx.abs(), b_r=wave_depth(HW) * U * (xd * gd).abs().sum((2, 3)))


def torgb_bwd_ref(x, g, w_rgb, s):
    """dx[b,i] = s[b,i] sum_j (w[j,i] / sqrtf(Cin)) g[b,j] (K = 3, c = 2: the products with the scale and with s), r[b,j,i] =
    sum_p x[b,i] g[b,j] (K = wave_depth(HW), c = 0)."""
    cin = x.shape[1]
    HW = x.shape[2] * x.shape[3]
    wd = w_rgb.double().reshape(3, cin) * wscale32(cin)
    xd, gd, sd = x.double(), g.double(), s.double()[:, :, None, None]
    dx = sd * torch.einsum('ji,bjhw->bihw', wd, gd)
    mag = sd.abs() * torch.einsum('ji,bjhw->bihw', wd.abs(), gd.abs())
    return dict(dx=dx, r=torch.einsum('bihw,bjhw->bji', xd, gd), b_dx=5 * U * mag,
                b_r=wave_depth(HW) * U * torch.einsum('bihw,bjhw->bji', xd.abs(), gd.abs()))


def blur_adjoint_ref(g, fir, planes=None):
    """gT[2a+py, 2b+px] = sum_{dy,dx < 4} g[2a+py+1-dy, 2b+px+1-dx] K[3-dy][3-dx] (g [B,C,2H,2W], zero outside), sixteen shifted
    slices of the zero-padded g, written as parity planes [B,C,4,H+1,W+1] (plane 2 py + px at [a,b]); the planes' padding row
    and column (rows / cols 2H+1, 2W+1 of the interleaved array) are 0.  asum[b,c] = sum gT t over all four planes.
    K = 16, c = 0 (an fma chain); asum: K = adjoint_depth(H, W)."""
    B, C, H2, W2 = g.shape
    H, W = H2 // 2, W2 // 2
    gp = g.new_zeros(B, C, H2 + 5, W2 + 5, dtype=torch.float64)
    gp[:, :, 2:2 + H2, 2:2 + W2] = g.double()
    kd = fir.double()
    acc = mag = None
    for dy in range(4):
        for dx in range(4):           # row i + 1 - dy of g is row i + 3 - dy of the padded array
            sl = gp[:, :, 3 - dy:3 - dy + H2 + 2, 3 - dx:3 - dx + W2 + 2] * float(kd[3 - dy, 3 - dx])
            acc, mag = (sl, sl.abs()) if acc is None else (acc + sl, mag + sl.abs())
    for a in (acc, mag):
        a[:, :, H2 + 1] = 0
        a[:, :, :, W2 + 1] = 0
    gt = torch.stack([acc[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], 2)
    gm = torch.stack([mag[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], 2)
    res = dict(gt=gt, b_gt=16 * U * gm)
    if planes is not None:
        td = planes.double()
        res['asum'] = (gt * td).sum((2, 3, 4))
        res['b_asum'] = adjoint_depth(H, W) * U * (gm * td.abs()).sum((2, 3, 4))
    return res


def prepack_t_ref(w, flip):
    """w [Cout,Cin,k,k] -> fp64 [Cout, k k, Cin], taps reversed for flip; WITHOUT the scale fp32(1 / sqrtf(Cin k k))."""
    cout, cin, k, _ = w.shape
    t = w.double().reshape(cout, cin, k * k)
    if flip:
        t = t.flip(2)
    return t.permute(0, 2, 1).contiguous()


def decode_split(xs, shape, arith):
    """XS [B, C/8, 2, HW, 8] int16 -> fp64 [B,C,H,W] = hi + lo (tests/test_gpu_split.py::_decode_split)."""
    B, C, H, W = shape
    v = xs.view(torch.float16 if arith == 'fp16x3' else torch.bfloat16).double()
    v = v[:, :, 0] + v[:, :, 1]
    return v.permute(0, 1, 3, 2).reshape(B, C, H, W) * (16.0 if arith == 'fp16x3' else 1.0)


def decode_split_planes(xs, B, C, H, W, arith):
    """The DOWN3 phase-major form [B, 4 C/8, 2, (H+1)(W+1), 8] int16 (chunk index ph C/8 + c/8) -> fp64 planes [B,C,4,H+1,W+1]."""
    G, RP = C // 8, (H + 1) * (W + 1)
    assert tuple(xs.shape) == (B, 4 * G, 2, RP, 8) and xs.dtype == torch.int16
    v = xs.view(torch.float16 if arith == 'fp16x3' else torch.bfloat16).double()
    v = (v[:, :, 0] + v[:, :, 1]).view(B, 4, G, RP, 8)
    v = v.permute(0, 2, 4, 1, 3).reshape(B, C, 4, H + 1, W + 1)
    return v * (16.0 if arith == 'fp16x3' else 1.0)


def split_step(ref, arith):
    """What hi + lo may miss of a value, whichever way the conversions round: bf16x3 keeps 8 + 8 significand bits (2^-16 |v|);
    fp16x3 11 + 11 (2^-22 |v|) of v / 16, whose low term ends at fp16's subnormal step 2^-24 (2^-20 of v); and the product with
    d (times 1/16) before the split is one fp32 rounding."""
    a = ref.abs()
    return U * a + (2.0 ** -16 * a if arith == 'bf16x3' else 2.0 ** -22 * a + 2.0 ** -20)


def split_fits(v, arith):
    """Exact regime: every value has at most 16 significant bits (bf16x3), or 22 with v / 16 inside fp16's range and a multiple
    of its subnormal step (fp16x3), so that hi + lo is the value itself."""
    a = v.abs().double().reshape(-1)
    a = a[a > 0]
    if a.numel() == 0:
        return True
    m, _ = torch.frexp(a)                                       # a = m 2^e, 1/2 <= m < 1
    bits = 16 if arith == 'bf16x3' else 22
    ok = bool((m * 2.0 ** bits == (m * 2.0 ** bits).round()).all())
    if arith == 'fp16x3':
        ok = ok and float(a.max()) / 16 <= 65504.0 and bool(((a / 16) * 2.0 ** 24 == ((a / 16) * 2.0 ** 24).round()).all())
    return ok


# ------------------------------------------------------------------ the launch rules, restated

def grad_join_path(HW, noise_bstride, offsets, has_rgb, has_add):
    """sgdfr_grad_join_f32's choice of kernel: 'rgb' | 'vec4' | 'scalar'.  offsets: the distance in floats of every tensor pointer
    (out, gu, g_rgb, g_add, noise, g_pre; absent ones left out) from a 16-byte boundary."""
    vec = HW % 4 == 0 and noise_bstride % 4 == 0 and all(o % 4 == 0 for o in offsets)
    if vec and has_rgb and not has_add and HW >= 1024:
        return 'rgb'
    return 'vec4' if vec else 'scalar'


def adjoint_strips(planes, H, W):
    return planes * ((H + 1 + ADJ_QV - 1) // ADJ_QV) * (W + 1)


def adjoint_tail(planes, H, W):
    """(lanes of the last wave of the second grid-stride pass, whether that wave's 64 strips of the FIRST pass lay in one plane)."""
    per = ((H + 1 + ADJ_QV - 1) // ADJ_QV) * (W + 1)
    strips, threads = planes * per, ADJ_GRID_CAP * 256
    assert threads < strips <= 2 * threads
    lanes = strips % 64
    first = strips - threads - lanes
    return lanes, first // per == (first + 63) // per


def adjoint_strides(planes, H, W):
    """blur_adjoint_kernel loops when there are more strips than 8192 blocks x 256 threads."""
    return adjoint_strips(planes, H, W) > ADJ_GRID_CAP * 256


def split_plan(B, C, H, W):
    """sgdfr_blur_adjoint_split_f32: dict(QC, extra: column W rides on the thread of column W - 1, col_tiles, tiles, last: the
    columns of the last column tile)."""
    QC = 64 if W >= 64 else 32
    extra = W % QC == 0
    col_tiles = W // QC if extra else (W + 1 + QC - 1) // QC
    tiles = B * (C // 8) * ((H + 1 + ADJ_QV - 1) // ADJ_QV) * col_tiles
    last = QC + 1 if extra else (W + 1) - (col_tiles - 1) * QC
    return dict(QC=QC, extra=extra, col_tiles=col_tiles, tiles=tiles, last=last, strides=tiles > ADJ_GRID_CAP)


def prepack_strides(cout, cin, k):
    return cout * cin * k * k > PREPACK_GRID_CAP * 256


# ------------------------------------------------------------------ inputs

def ints(seed, key, shape, lo, hi, ends=True):
    """Seeded integers in [lo, hi] as fp32; with `ends` the first and the last element along the last axis are non-zero (what a
    dropped head or tail element would lose)."""
    a = _rng(seed, key).integers(lo, hi + 1, size=tuple(shape)).astype(np.float32)
    if ends and a.size:
        for i in (0, -1):
            e = a[..., i]
            e[e == 0] = 1.0
    return torch.from_numpy(a)


def _real(seed, key, shape, mean=0.0, std=1.0):
    from stylegan_directions_face_reenactment_amd import synthetic as S
    return S.counter_tensor(seed, key, shape, mean, std)


# the ranges of the exact inputs (out has five values, so it holds zeros in plenty; a few more are planted)
EX_ACT = dict(g=8, out=8, noise=8, nw=3.0, bias=8)
EX_JOIN = dict(g=2, out=2, noise=1, nw=2.0, bias=1, w=2, s=(1.0, 2.0))


def act_inputs(kind, B, C, HW, noise='none', bias=True, seed=41):
    """dict(g, out, noise, noise_w, bias) of act_grad_reduce on the CPU, planes [B,C,1,HW]."""
    key = 'ag.%s.%d.%d.%d.' % (kind, B, C, HW)
    nshape = (1 if noise == 'shared' else B, 1, 1, HW)
    if kind == 'exact':
        r = EX_ACT
        i = dict(g=ints(seed, key + 'g', (B, C, 1, HW), -r['g'], r['g']), out=ints(seed, key + 'o', (B, C, 1, HW), -r['out'], r['out']),
                 noise=ints(seed, key + 'n', nshape, -r['noise'], r['noise']), noise_w=torch.tensor([r['nw']]),
                 bias=ints(seed, key + 'b', (C,), -r['bias'], r['bias']))
    else:
        i = dict(g=_real(seed, key + 'g', (B, C, 1, HW)), out=_real(seed, key + 'o', (B, C, 1, HW)), noise=_real(seed, key + 'n', nshape),
                 noise_w=torch.tensor([0.3]), bias=_real(seed, key + 'b', (C,)))
    i['out'].view(-1)[1::5] = 0.0                   # exact zeros: the factor there is `slope`
    if noise == 'none':
        i['noise'] = i['noise_w'] = None
    if not bias:
        i['bias'] = None
    return i


def join_inputs(kind, B, C, HW, terms=('gu', 'rgb', 'add'), noise='none', bias=True, seed=43):
    """dict(out, gu, s_next, g_rgb, w_rgb, s_rgb, g_add, noise, noise_w, bias) of grad_join on the CPU (absent terms None)."""
    key = 'gj.%s.%d.%d.%d.' % (kind, B, C, HW)
    nshape = (1 if noise == 'shared' else B, 1, 1, HW)
    if kind == 'exact':
        r = EX_JOIN
        mk = lambda k, shape, m: ints(seed, key + k, shape, -m, m)                                # noqa: E731
        sc = lambda k: choice_tensor(seed, key + k, (B, C), r['s'])                                 # noqa: E731
        i = dict(out=mk('o', (B, C, 1, HW), r['out']), gu=mk('u', (B, C, 1, HW), r['g']), s_next=sc('sn'),
                 g_rgb=mk('r', (B, 3, 1, HW), r['g']), w_rgb=mk('w', (3, C), r['w']), s_rgb=sc('sr'), g_add=mk('a', (B, C, 1, HW), r['g']),
                 noise=mk('n', nshape, r['noise']), noise_w=torch.tensor([r['nw']]), bias=mk('b', (C,), r['bias']))
    else:
        mk = lambda k, shape, m=None: _real(seed, key + k, shape)                                  # noqa: E731
        sc = lambda k: _real(seed, key + k, (B, C), 1.0, 0.3)                                       # noqa: E731
        i = dict(out=mk('o', (B, C, 1, HW)), gu=mk('u', (B, C, 1, HW)), s_next=sc('sn'), g_rgb=mk('r', (B, 3, 1, HW)),
                 w_rgb=mk('w', (3, C)), s_rgb=sc('sr'), g_add=mk('a', (B, C, 1, HW)), noise=mk('n', nshape),
                 noise_w=torch.tensor([0.3]), bias=mk('b', (C,)))
    i['out'].view(-1)[1::5] = 0.0
    if 'gu' not in terms:
        i['gu'] = i['s_next'] = None
    if 'rgb' not in terms:
        i['g_rgb'] = i['w_rgb'] = i['s_rgb'] = None
    if 'add' not in terms:
        i['g_add'] = None
    if noise == 'none':
        i['noise'] = i['noise_w'] = None
    if not bias:
        i['bias'] = None
    return i


def sum_exact_condition(HW, gmax, gunit, omax, nzmax, nw, bmax, slope=SLOPE, gain=GAIN):
    """The a-priori condition of an exact act_grad_reduce / grad_join case: the largest sum, HW max|g_pre| max|y|, counted in the
    product of the two units (g_pre: gunit slope gain; y: 1/gain, of out / gain), stays below 2^24; so do the smaller sums."""
    gp_max, gp_unit = gmax * gain, gunit * slope * gain
    y_max, y_unit = omax / (gain * slope) + nw * nzmax + bmax, 1.0 / gain
    return HW * gp_max * y_max / (gp_unit * y_unit) < 2 ** 24


def act_exact_condition(HW):
    r = EX_ACT
    return sum_exact_condition(HW, r['g'], 1.0, r['out'], r['noise'], r['nw'], r['bias'])


def join_exact_condition(C, HW):
    """|g| <= max|gu| max s + max s 3 max|w| max|g_rgb| / sqrt(C) + max|g_add| in units of 1 / sqrt(C) (a power of two); the r sums
    are integers below HW max|out| max|g|."""
    r = EX_JOIN
    sc = wscale32(C)
    if sc not in (1.0, 0.5, 0.25, 0.125):
        return False
    gmax = r['g'] * max(r['s']) + max(r['s']) * 3 * r['w'] * sc * r['g'] + r['g']
    return sum_exact_condition(HW, gmax, sc, r['out'], r['noise'], r['nw'], r['bias']) and HW * r['out'] * r['g'] < 2 ** 24


def reduce_inputs(kind, what, B, C, HW, seed=47, bcast=False):
    """scale_reduce: dict(gu, x, s); torgb_bwd: dict(x, g, w_rgb, s).  Exact: integers in [-8, 8], s in {1/2, 1, 2}: the sums stay
    below 64 HW, dx a multiple of 1 / (2 sqrt(C))."""
    key = 'rd.%s.%s.%d.%d.%d.' % (kind, what, B, C, HW)
    if kind == 'exact':
        mk = lambda k, shape: ints(seed, key + k, shape, -8, 8)                                     # noqa: E731
        s = choice_tensor(seed, key + 's', (B, C), (0.5, 1.0, 2.0))
    else:
        mk = lambda k, shape: _real(seed, key + k, shape)                                           # noqa: E731
        s = _real(seed, key + 's', (B, C), 1.0, 0.3)
    if what == 'scale':
        return dict(gu=mk('u', (B, C, 1, HW)), x=mk('x', (1 if bcast else B, C, 1, HW)), s=s)
    return dict(x=mk('x', (B, C, 1, HW)), g=mk('g', (B, 3, 1, HW)), w_rgb=mk('w', (3, C)), s=s)


def reduce_exact_condition(HW, cin=None):
    """sum x g: integers below 64 HW; torgb_bwd's dx needs 1 / sqrt(Cin) a power of two."""
    return 64 * HW < 2 ** 24 and (cin is None or wscale32(cin) in (1.0, 0.5, 0.25, 0.125))


def exact_firs():
    """The symmetric [1,3,3,1] (x) [1,3,3,1], unnormalised, and an asymmetric integer 4x4."""
    sym = torch.outer(torch.tensor([1., 3., 3., 1.]), torch.tensor([1., 3., 3., 1.]))
    asym = torch.tensor([[1, -2, 3, 4], [5, 6, -7, 8], [-3, 2, 1, 7], [4, -6, 5, 2]], dtype=torch.float32)
    return sym, asym


def real_firs():
    sym, asym = exact_firs()
    return sym / 16, asym / 16         # sym / 16 = make_fir([1,3,3,1], gain=4), the generator's


EX_BLUR = dict(g=4, t=4, d=(0.5, 1.0, 2.0))


def blur_inputs(kind, B, C, H, W, seed=53, device='cpu'):
    """dict(g [B,C,2H,2W], planes [B,C,4,H+1,W+1], d [B,C]).  The large cases are drawn on `device` with torch's generator."""
    key = 'ba.%s.%d.%d.%d.%d.' % (kind, B, C, H, W)
    if device != 'cpu':
        gen = torch.Generator(device=device).manual_seed(seed)
        m = EX_BLUR['g']
        g = torch.randint(-m, m + 1, (B, C, 2 * H, 2 * W), generator=gen, device=device).float()
        t = torch.randint(-m, m + 1, (B, C, 4, H + 1, W + 1), generator=gen, device=device).float()
        d = torch.tensor(EX_BLUR['d'], device=device)[torch.randint(0, 3, (B, C), generator=gen, device=device)]
        g[..., 0][g[..., 0] == 0] = 1.0
        g[..., -1][g[..., -1] == 0] = 1.0
        return dict(g=g, planes=t, d=d)
    if kind == 'exact':
        return dict(g=ints(seed, key + 'g', (B, C, 2 * H, 2 * W), -EX_BLUR['g'], EX_BLUR['g']),
                    planes=ints(seed, key + 't', (B, C, 4, H + 1, W + 1), -EX_BLUR['t'], EX_BLUR['t']),
                    d=choice_tensor(seed, key + 'd', (B, C), EX_BLUR['d']))
    return dict(g=_real(seed, key + 'g', (B, C, 2 * H, 2 * W)), planes=_real(seed, key + 't', (B, C, 4, H + 1, W + 1)),
                d=_real(seed, key + 'd', (B, C), 1.0, 0.2))


def blur_exact_condition(H, W, fir):
    """|gT| <= max|g| sum|K| and asum <= 4 (H+1)(W+1) max|gT| max|t|, integers, below 2^24; times d in {1/2, 1, 2} the values are
    half-integers below 2^16 of that unit (the split forms hold them whole)."""
    gt = EX_BLUR['g'] * float(fir.abs().sum())
    return (bool(torch.equal(fir, fir.round())) and 4 * (H + 1) * (W + 1) * gt * EX_BLUR['t'] < 2 ** 24 and
            gt * max(EX_BLUR['d']) / min(EX_BLUR['d']) < 2 ** 16)


# ------------------------------------------------------------------ the cases

CHUNK_HW = (1, 63, 64, 65, 2047, 2048, 2049, 4100)
# (B, C, HW): every HW at waves B C chunks that are and are not a multiple of 4, and wave counts 1, 5, 7
CHUNK_CASES = ([(2, 3, hw) for hw in CHUNK_HW] + [(1, 4, 2048), (1, 1, 1), (1, 1, 65), (1, 5, 2047), (1, 7, 64), (3, 4, 2049)])


def waves_of(B, C, HW):
    return B * C * chunks_of(HW)


# act_grad_reduce: (B, C, HW, noise, bias, want_y)
ACT_CASES = [(B, C, HW, ('none', 'shared', 'per')[n % 3], bool(n % 2), bool((n // 2) % 2 == 0)) for n, (B, C, HW) in enumerate(CHUNK_CASES)]
ACT_CASES += [(2, 3, 2049, nz, b, wy) for nz in ('none', 'shared', 'per') for b in (True, False) for wy in (True, False)]

TERM_SUBSETS = [('gu',), ('rgb',), ('add',), ('gu', 'rgb'), ('gu', 'add'), ('rgb', 'add'), ('gu', 'rgb', 'add')]


def J(B, C, HW, terms=('gu', 'rgb'), noise='shared', bias=True, want_y=True, off=None, work=False, exact=None, real=True):
    """A grad_join case.  off: the tensor handed over as a view one float into its storage; work: the caller's zeroed workspace."""
    exact = join_exact_condition(C, HW) if exact is None else exact
    return dict(B=B, C=C, HW=HW, terms=tuple(terms), noise=noise, bias=bias, want_y=want_y, off=off, work=work, exact=exact, real=real)


def join_id(c):
    return 'B%d-C%d-HW%d-%s-%s%s%s%s%s' % (c['B'], c['C'], c['HW'], '+'.join(c['terms']), c['noise'], '' if c['bias'] else '-nobias',
                                          '' if c['want_y'] else '-noy', '-off_' + c['off'] if c['off'] else '', '-work' if c['work'] else '')


def join_path(c):
    """The kernel a case must reach: out, g_pre and the noise are aligned; the tensor named by c['off'] sits one float off."""
    off = [int(c['off'] == name) for name, term in (('gu', 'gu'), ('g_rgb', 'rgb'), ('g_add', 'add')) if term in c['terms']]
    nbs = c['HW'] if c['noise'] == 'per' else 0
    return grad_join_path(c['HW'], nbs, [0, 0] + off + ([0] if c['noise'] != 'none' else []), 'rgb' in c['terms'], 'add' in c['terms'])


# all seven subsets at one scalar shape (HW % 4 != 0) and one float4 shape, with and without the caller's workspace
JOIN_SUBSET_CASES = [J(2, 4, hw, t, noise=('per', 'shared', 'none')[n % 3], want_y=bool(n % 2), work=w)
                     for hw in (2049, 2052) for n, t in enumerate(TERM_SUBSETS) for w in (False, True)]
# chunk edges of the scalar and float4 kernels (gu + add keeps them off the rgb kernel)
JOIN_CHUNK_CASES = [J(B, C if C != 3 else 4, hw, ('gu', 'rgb', 'add'), noise=('none', 'shared', 'per')[n % 3])
                    for n, (B, C, hw) in enumerate(CHUNK_CASES)] + [J(1, 4, 4, ('gu',)), J(1, 5, 64, ('gu', 'rgb')), J(1, 7, 2048, ('add',))]
JOIN_PATH_CASES = (
    [J(2, C, hw) for hw in (1020, 1024, 1028, 2048, 2052, 4096) for C in (4, 16)] +                    # exact: C 4, 16
    [J(2, C, hw, exact=False) for C in (5, 6, 7, 8) for hw in (1028, 2052)] +                           # C % GJ_CPW, real only
    [J(3, 5, 4096, exact=False), J(1, 7, 1024, exact=False)] +
    [J(2, 4, 2052, ('rgb',)), J(2, 6, 1028, ('rgb',), exact=False), J(2, 16, 2052, noise='per'), J(2, 5, 4096, noise='per', exact=False),
     J(2, 4, 2052, noise='none'), J(2, 7, 1028, noise='none', bias=False, exact=False), J(2, 4, 2052, want_y=False),
     J(2, 6, 2052, ('rgb',), want_y=False, work=True, exact=False), J(2, 4, 1028, work=True)] +
    [J(2, 4, 2052, ('gu', 'rgb', 'add')), J(2, 5, 1028, ('rgb', 'add'), exact=False)] +                 # g_add leaves the rgb path
    [J(2, 4, 2052, ('gu', 'rgb', 'add'), off=o) for o in ('gu', 'g_rgb', 'g_add')] + [J(2, 4, 1028, off='g_rgb'), J(2, 5, 1028, off='gu', exact=False)] +
    [J(2, 4, hw) for hw in (1021, 1026, 2050)] + [J(2, 4, 1023, noise='per')])                           # HW % 4 != 0 (and the noise stride)
JOIN_CASES = JOIN_SUBSET_CASES + JOIN_CHUNK_CASES + JOIN_PATH_CASES

# scale_reduce: (B, C, HW, bcast)
SCALE_CASES = [(B, C, hw, False) for B, C, hw in CHUNK_CASES] + [(3, 4, 65, True), (3, 5, 2049, True)]
# torgb_bwd: (B, Cin, HW)
TORGB_BWD_CASES = [(2, cin, hw) for cin in (1, 3, 4, 64) for hw in (2048, 2049)] + [(B, 4 if C == 3 else C, hw) for B, C, hw in CHUNK_CASES]
# prepack_t: (Cout, Cin, k): Cout Cin k k below, at and above one block of 256, and above 4096 x 256
PREPACK_T_CASES = [(3, 5, 3), (5, 51, 1), (4, 64, 1), (16, 16, 1), (1, 257, 1), (7, 4, 3), (3, 4, 1), (2, 13, 3), (260, 449, 3), (1030, 1024, 1)]

BLUR_ADJ_H = (1, 2, 3, 4, 5, 8)
BLUR_ADJ_W = (1, 2, 3, 31, 32, 33)
BLUR_ADJ_PLANES = ((1, 3), (2, 1), (1, 1))                   # (B, C), rotating: B C = 3 at (2, 2) is a wave across two planes
# B C = 4065 planes of 520 strips = 2,113,800 > 8192 x 256: the last wave of the second pass keeps 8 lanes, and all 64 of them sat in ONE
# plane in the first pass (the wave-sum path: what a reduction that ignores EXEC would pick up from the lanes that have left)
BLUR_ADJ_STRIDE = (15, 271, 1, 519)

SPLIT_W = (1, 31, 32, 33, 63, 64, 65, 96, 128)
SPLIT_H = (1, 4, 5)
SPLIT_STRIDE = [(17, 512, 1, 512), (129, 512, 1, 32)]          # 8704 tiles at QC 64, 8256 at QC 32: both above 8192

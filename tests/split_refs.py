"""Reference machinery of tests/test_gpu_split_edges.py: the split-operand convs (csrc/split.hip, csrc/split_kernel.h, csrc/wsplit.hip,
csrc/wswide.hip) and their producers against the fp64 references of conv_refs.py, with a-priori bounds of the split arithmetics,
decoders of the documented operand forms, the exact inputs, the case lists, and the host rules of the launches restated in Python.
Checked on the CPU by tests/test_cpu_split_edges.py, so that a failure of the GPU module points at a kernel.

The weight.  The references take the raw weight w [Cout,Cin,3,3] and apply 1/sqrt(9 Cin) in fp64; the pack's own fp32 multiply
(w * fl32(64 / sqrtf(9 Cin)), bf16: fl32(1 / sqrtf)) is one rounding of the constant c.  The fp16 range shifts (x / 16, w * 64,
result / 4) are powers of two and cost nothing.

The bound of a split arithmetic (conv_reference, split_terms), per output element, a priori:

    (K (1 + 2^-10) + c) 2^-24 mag          the fp32 accumulation of conv_refs.py; K products, of which the two cross products of every
                                           operand pair are below 2^-10 of the main one, c the other roundings on the path
  + 3 step mag                             a product of two split operands (a + da)(b + db) - lo lo: the two representation residuals
                                           and the dropped lo lo term, each at most step |a b|; step = 2^-16 (bf16x3: 8 + 8 bits),
                                           2^-22 (fp16x3 and the fp16 pairs of fp16f8: 11 + 11 bits)
  + 2^-20 magw + 2^-30 magx                fp16 only: the low term ends at fp16's subnormal step 2^-24, which is 2^-20 of x s (x s / 16
                                           is stored) and 2^-30 of w / sqrt(9 Cin) (64 times it is stored); magw = sum |w| over the
                                           products of the element, magx = sum |x s|
  + fp16f8: 2^-13 mag + 2^-12 magw + 2^-27 max|w| magx        (derived next)

mag = sum |x s| |w| |d| over the products of the element (+ |noise term| + |bias| where the accumulation term is concerned).

fp16f8 (include/sgdfr.h SGDFR_SPLIT_FP16F8): the main product x_hi w_hi is fp16, both cross products run in e4m3.  In the stored
domain X = x s / 16 = X_hi + X_lo, Wd = 64 w = W_hi + W_lo, |X_lo| <= 2^-11 |X_hi|, |W_lo| <= 2^-11 |W_hi|; the chunks hold
e4m3(X_lo 2^7), e4m3(X_hi 2^-4), e4m3(W_hi 2^-EW), e4m3(W_lo 2^(11-EW)) with 2^(EW+7) <= max|Wd| < 2^(EW+8).  e4m3 keeps three
fraction bits down to 2^-6 and a fixed step 2^-9 below: |e4m3(q) - q| <= 2^-4 |q| + 2^-10 while |q| <= 448 (asserted of every case: no
clamp).  So the four errors of W_hi X_lo + W_lo X_hi are at most
    |W_hi| (2^-4 |X_lo| + 2^-17) + (2^-4 |W_hi| + 2^(EW-10)) |X_lo| + |W_lo| (2^-4 |X_hi| + 2^-6) + (2^-4 |W_lo| + 2^(EW-21)) |X_hi|
 <= 4 2^-15 |Wd X| + 2^-16 |Wd| + 2^(EW-20) |X|,
and in output units (X Wd / 4 = x s w): 2^-13 |x s w| + 2^-12 |w| + 2^-27 max|w| |x s|.  With operands of order one the second
term rules (the e4m3 values are subnormal: the range plan of the generator puts activations near 2^10 of the stored domain, and
the fp16f8 cases here are as loud).

Winograd forms F(f,3) along rows (wsplit_reference): "the algorithm itself on absolute values", as conv_refs.wino_bound does for
wino.hip: |A^T| ((|B^T| |x s|) (.) (|G| |w|)) with the accumulation K = 3 Cin products per transform-domain element, and the split
terms on the transformed operands (3 step, the fp16 floors with |V| <= 2 / 10 max|x s|: WSPLIT_GROWTH_LOG2).  The growth of B^T and
G is in those absolute-value sums (row sums of |B^T| up to 2 / 10).

Exact inputs (case_inputs, kind 'int'): integers in [-8, 8]; s, d, s_next in {1/2, 1, 2}; integer noise and bias, slope 1/4, gain 2; weights
k sqrt(9 Cin) with integer k in [-8, 8] for Cin in {16, 64, 256}, where sqrt(9 Cin) = 12, 24, 48 (F(2,3): even k, so that G w stays
integral).  exact_weight_values proves with numpy float32 that the pack's multiply maps every such value to the dyadic 64 k (bf16:
k), and drops a value that does not.  Such operands have a zero low term in both 16-bit formats, so all three arithmetics must
return the fp64 value bit for bit."""
import numpy as np
import torch

import conv_refs as R
from backward_refs import decode_split_planes, split_fits, split_step  # noqa: F401  (re-exported)
from dense_refs import F32, U, choice_tensor, int_tensor, ratio, wscale32  # noqa: F401

PLAIN3, UP3, DOWN3 = R.PLAIN3, R.UP3, R.DOWN3
SLOPE, GAIN = R.SLOPE, R.GAIN
ARITHS = ('fp16x3', 'bf16x3')
STEP = {'bf16x3': 2.0 ** -16, 'fp16x3': 2.0 ** -22, 'fp16f8': 2.0 ** -22}
SPLIT_CB = 16


# ------------------------------------------------------------------ the host rules of csrc/split.hip, restated (environment at its defaults)

class Plan(dict):
    __getattr__ = dict.__getitem__


def _plan(name, cfg, nt, pt, nss, nw):
    return Plan(name=name, cfg=cfg, nt=nt, pt=pt, nss=nss, nw=nw)


PLAIN_WIDE = _plan('plain 128x256', 0, 128, 256, 3, 8)
PLAIN_NARROW = _plan('plain 64x512', 1, 64, 512, 3, 8)
UP_WIDE = _plan('up 128x128', 2, 128, 128, 3, 8)
UP_NARROW = _plan('up 64x256 rows', 3, 64, 256, 3, 8)
UP_DEEP = _plan('up 64x256 deep', 4, 64, 256, 1, 8)
DOWN = _plan('down 128x256', 5, 128, 256, 1, 8)
PLAIN_XL = _plan('plain 128x512', 6, 128, 512, 3, 8)
PLAIN_4WAVE = _plan('plain 64x256 4-wave', 8, 64, 256, 3, 4)
PLANS = (PLAIN_WIDE, PLAIN_NARROW, UP_WIDE, UP_NARROW, UP_DEEP, DOWN, PLAIN_XL, PLAIN_4WAVE)


def split_lds_bytes(g, NT, nss, down=False, nws=2, PT=256, slim=False):
    """split_lds_bytes (split.hip): g carries xs, simgs and the K channel count Cin."""
    wslot = NT * 256 if down else NT * 192 * (3 // nss)
    loop = 2 * 64 * g['xs'] + nws * wslot + (0 if (down or slim) else ((g['simgs'] * g['Cin'] + 3) & ~3) * 4)
    epi = (g['simgs'] * NT * 6 + NT + (1024 if NT * PT > 128 * 256 else 512) * 3) * 4
    return loop + epi if g['simgs'] <= 2 else max(loop, epi)


def split_geometry(B, cin, cout, H, W, mode, plan):
    """split_geometry (split.hip): the pixel tiling of one plan as a dict, or None when the shape cannot use it."""
    down = mode == DOWN3
    half = plan.nt == 64 and cout % 64 == 32 and not down
    if cin % SPLIT_CB or (cout % plan.nt and not half) or B < 1:
        return None
    K = cin * 4 if down else cin
    PT, HW, P, Rr = plan.pt, H * W, W + 1, H + 1
    g = dict(B=B, Cin=K, Cout=cout, H=H, W=W, P=P, R=Rr, half=half, plan=plan, TC=0, TR=0)
    if B * Rr * P + 4 * P + 8 >= 2 ** 31 or B * HW >= 2 ** 31:
        return None
    if mode == UP3 or down:
        g.update(kind='flat', total_pix=B * Rr * P, xlen=PT + P + 2, rps=Rr * P)
        g['simgs'] = (g['xlen'] - 1) // (Rr * P) + 2
        g['n_pix_tiles'] = (g['total_pix'] + PT - 1) // PT
    elif W > 64:
        TC = 32 if ((plan.nt == 128 and plan.pt == 512) or plan.cfg == 8) else 64
        TR = PT // TC
        if W % TC or H % TR:
            return None
        g.update(kind='patch', TC=TC, TR=TR, total_pix=B * HW, xlen=(TR + 2) * (TC + 2), simgs=1, n_pix_tiles=B * (W // TC) * (H // TR))
    else:
        if PT % W == 0 and HW % PT == 0:
            span, simgs, kind = (PT // W - 1) * P + (W - 1), 1, 'rows'
        elif PT % HW == 0:
            span, simgs, kind = (PT // HW - 1) * Rr * P + (H - 1) * P + (W - 1), PT // HW, 'images'
        else:
            return None
        g.update(kind=kind, total_pix=B * HW, xlen=span + 2 * P + 3, simgs=simgs, n_pix_tiles=(B * HW + PT - 1) // PT)
    slim = plan.cfg == 8
    g['xs'] = (g['xlen'] + 63) & ~63 if (plan.nw == 8 or slim) else (g['xlen'] + 7) & ~7
    g['n_cout_tiles'] = (cout + plan.nt - 1) // plan.nt
    nthr = plan.nw * 64
    g['nex'] = (2 * g['xs'] + nthr - 1) // nthr
    if g['nex'] > (3 if down else 4):
        return None
    g['lds'] = split_lds_bytes(g, plan.nt, plan.nss, down, 2, plan.pt, slim)
    if g['lds'] > (160 if plan.nw == 8 else 80) * 1024:
        return None
    if slim and g['simgs'] > 2:
        return None
    g['NEX'] = 2 if g['nex'] <= 2 else 3 if g['nex'] == 3 else (3 if down else 4)      # launch_split's instantiation
    g['ragged'] = g['total_pix'] % PT != 0 and g['kind'] != 'patch'                     # a partial last pixel tile
    return g


def split_plan(B, cin, cout, H, W, mode, xin_whole=False, p4=64):
    """split_plan (split.hip): the first plan of the mode's order that fits, as its geometry dict (g['plan'] the plan), or None.
    p4: SGDFR_SPLIT_P4, which the library reads per call (default 64)."""
    order = []
    if mode == UP3:
        big = B * (H + 1) * (W + 1) * (cout // 64) >= 256 * 256
        if big:
            order.append(UP_DEEP)
        if cout % 128 == 0:
            order.append(UP_WIDE)
        order.append(UP_NARROW)
    elif mode == PLAIN3:
        if xin_whole and cout % 128 == 0 and B * H * W * (cout // 128) >= 2 * 256 * 512:
            order.append(PLAIN_XL)
        p4_ok = p4 > 0 and xin_whole and cin <= p4 and B * H * W * ((cout + 63) // 64) >= 4 * 512 * 256
        if p4_ok and cout % 128 == 0 and p4 >= 128:
            order.append(PLAIN_4WAVE)
        if cout % 128 == 0:
            order.append(PLAIN_WIDE)
        if p4_ok:
            order.append(PLAIN_4WAVE)
        order.append(PLAIN_NARROW)
    elif mode == DOWN3:
        order.append(DOWN)
    for plan in order:
        g = split_geometry(B, cin, cout, H, W, mode, plan)
        if g is not None:
            return g
    return None


def split_supported(B, cin, cout, H, W, mode):
    return int(split_plan(B, cin, cout, H, W, mode) is not None)


def split_f8_ok(B, cin, cout, H, W, mode):
    if mode not in (UP3, PLAIN3):
        return 0
    g = split_plan(B, cin, cout, H, W, mode, True)
    return int(g is not None and g['plan'].cfg == (4 if mode == UP3 else 8))


def ksplit_hint(B, cin, cout, H, W, mode):
    g = split_plan(B, cin, cout, H, W, mode)
    if g is None:
        return 1
    blocks = g['n_pix_tiles'] * g['n_cout_tiles']
    if blocks >= 192:
        return 1
    s = min(256 // blocks, (cin // SPLIT_CB) // 2, 16)
    return 1 if s < 2 else s


def xin_supported(B, cin, cout, H, W, mode):
    g = split_plan(B, cin, cout, H, W, mode)
    if g is None or g['plan'].cfg not in (0, 1, 3, 4, 5):
        return 0
    p = g['plan']
    if p.nss == 3 and p.cfg != 5 and split_lds_bytes(g, p.nt, p.nss, False, 3) > 160 * 1024:
        return 0
    return 1


def cout_tiles(B, cin, cout, H, W, mode, xin_whole=False):
    g = split_plan(B, cin, cout, H, W, mode, xin_whole)
    return 0 if g is None else g['n_cout_tiles']


def plan_info(B, cin, cout, H, W, mode, xin_whole=False):
    """sgdfr_modconv2d_split_plan_info's word."""
    g = split_plan(B, cin, cout, H, W, mode, xin_whole)
    return -1 if g is None else g['plan'].cfg | g['NEX'] << 4 | g['simgs'] << 8 | int(g['half']) << 20


def launch_facts(B, cin, cout, H, W, mode, xin=False, ksplit=1, up_tail=None):
    """What one sgdfr_modconv2d_split_f32 call launches, from split_plan, launch_plan, launch_split and launch_deep_tail: the geometry
    dict plus persistent (bool), grid, and for the deep plans the tail round (n_full, tail, lid0, count) or tail_round = None.
    up_tail: SGDFR_SPLIT_UP_TAIL (read per call; None = unset)."""
    g = split_plan(B, cin, cout, H, W, mode, xin and ksplit <= 1)
    if g is None:
        return None
    g = dict(g)
    p = g['plan']
    total = g['n_pix_tiles'] * g['n_cout_tiles'] * ksplit
    can_persist = xin and p.nss == 3 and p.nw == 8 and mode in (PLAIN3, UP3)
    g['persistent'] = bool(can_persist and total >= 4 * 256)
    g['grid'] = 256 if g['persistent'] else total
    g['ksplit'] = ksplit
    g['tail_round'] = None
    if p.cfg in (4, 5):
        t = g['n_pix_tiles'] * g['n_cout_tiles']
        n_full, tail = t // 256 * 256, t % 256
        max_full = up_tail if (up_tail is not None and up_tail > 1) else (1024 if mode == DOWN3 else 512)
        g['n_full'], g['tail'] = n_full, tail
        if not (up_tail == 0 or ksplit != 1 or n_full == 0 or n_full > max_full or tail == 0 or tail > 128):
            npt2 = (g['total_pix'] + 127) // 128
            c0 = n_full // g['n_pix_tiles']
            p0 = n_full - c0 * g['n_pix_tiles']
            lid0 = c0 * npt2 + 2 * p0
            xlen2 = 128 + g['P'] + 2
            g['tail_round'] = dict(n_full=n_full, tail=tail, lid0=lid0, count=g['n_cout_tiles'] * npt2 - lid0,
                                   xs=(xlen2 + 63) & ~63, simgs=(xlen2 - 1) // g['rps'] + 2, n_pix_tiles=npt2)
    return g


# ------------------------------------------------------------------ csrc/wsplit.hip and csrc/wswide.hip

def wsplit_geometry(B, cin, cout, H, W, f):
    if f not in (2, 4) or B < 1 or cin % 16 or cout % 128 or W % f or W < 16 or H < 1:
        return None
    TW = W // f
    tiles, runs, tct_max = (128, 16, 16) if f == 2 else (64, 24, 8)
    TCT = tct_max if TW >= tct_max else tct_max // 2
    TR = tiles // TCT
    if TW % TCT or H % TR:
        return None
    xs = (TR + 2) * TCT
    if (runs * xs) % 64 or runs * xs > (5 if f == 2 else 4) * 512:
        return None
    g = dict(B=B, Cin=cin, Cout=cout, H=H, W=W, f=f, TW=TW, TCT=TCT, TR=TR, xs=xs, n_pix_tiles=B * (TW // TCT) * (H // TR),
             n_cout_tiles=cout // 128)
    if g['n_pix_tiles'] * g['n_cout_tiles'] >= 2 ** 30 or B * cout * H * W >= 2 ** 40:
        return None
    return g


def wsplit_supported(B, cin, cout, H, W, f):
    return int(wsplit_geometry(B, cin, cout, H, W, f) is not None)


def wswide_plan(g, mode_now):
    """wswide_plan (wswide.hip) on wsplit_geometry's dict for f = 4: the wide tiling (dict) or None.  mode_now: 0 never, 1 by tile
    count, 2 whenever the shape allows (SGDFR_WSPLIT_WIDE_NOW)."""
    if mode_now == 0 or g is None:
        return None
    if g['Cin'] % 16 or g['Cin'] < 64 or g['Cout'] % 128 or g['W'] % 32 or g['H'] % 16:
        return None
    old_blocks = g['n_pix_tiles'] * g['n_cout_tiles']
    TW = g['W'] // 4
    w = dict(g, TW=TW, TCT=8, TR=16, xs=144, n_pix_tiles=g['B'] * (TW // 8) * (g['H'] // 16))
    w['total_blocks'] = w['n_pix_tiles'] * w['n_cout_tiles']
    if (g['Cin'] // 8) * 12 * g['H'] * TW * 16 >= 2 ** 31 or g['Cout'] * g['Cin'] * 72 >= 2 ** 31:
        return None
    if mode_now == 1:
        r_wide, r_old = (w['total_blocks'] + 255) // 256, (old_blocks + 255) // 256
        if w['total_blocks'] < 192 or r_wide * 2 * 0.76 >= float(r_old):
            return None
    return w


def wsplit_wide(B, cin, cout, H, W):
    g = wsplit_geometry(B, cin, cout, H, W, 4)
    return int(g is not None and cin % 32 == 0 and wswide_plan(g, 1) is not None)


# ------------------------------------------------------------------ exact weights

def exact_weight_values(cs, arith, even=False):
    """The integers k in [-8, 8] (even: the even ones) for which the pack's own fp32 multiply maps the weight k sqrt(9 cs) to the
    dyadic it is meant to be: fl32(fl32(k m) * fl32(64 / sqrtf(9 cs))) == 64 k (bf16x3: scale fl32(1 / sqrtf(9 cs)), result k), as
    sgdfr_modconv_prepack_split_f32 / _wsplit_f32 form it.  cs: the channel count of the scale (Cin; DOWN3: the conv's Cout)."""
    root = np.sqrt(F32(cs) * F32(9))
    assert root.dtype == np.float32 and float(root) == round(float(root)), cs
    scale = (F32(1.0) if arith == 'bf16x3' else F32(64.0)) / root
    good = []
    for k in range(-8, 9, 2 if even else 1):
        w = F32(k) * root                                        # the fp32 weight the test hands to the pack
        got = F32(w * scale)
        if float(w) == k * float(root) and float(got) == (k if arith == 'bf16x3' else 64 * k):
            good.append(k)
    return good


def exact_condition(cin, taps=9, x=8, w=8, s=(0.5, 2.0), d=2.0, noise=8 * 3, bias=8, gain=GAIN, s_next=2.0, arith='fp16x3', growth=1):
    """conv_refs.exact_condition extended to the split case: the fp32 sums stay below 2^24 of their unit (as there), every operand has
    a zero low term (|x s| growth and |w| are integers over 2 of at most 8 bits, inside fp16's range after the shifts / 16 and * 64),
    and the fp16 accumulator unit (x s / 16 times 64 w, a multiple of 2^-5 growth) is far above the fp32 subnormals."""
    ok = R.exact_condition(cin, taps, x * growth, w, s, d, noise, bias)
    xs_max, w_max = x * s[1] * growth, w
    ok = ok and xs_max < 2 ** 8 and w_max < 2 ** 8                       # 8 significant bits: no low term in bf16 either
    if arith != 'bf16x3':
        ok = ok and xs_max / 16 <= 65504 and 64 * w_max <= 65504
    return bool(ok)


# ------------------------------------------------------------------ inputs

def _w_from_wp(wp):
    """packed [Cin,9,Cout] -> [1,Cout,Cin,3,3]"""
    cin, _, cout = wp.shape
    return wp.permute(2, 0, 1).reshape(1, cout, cin, 3, 3).contiguous()


def case_inputs(kind, c, arith='fp16x3', seed=17):
    """The tensors of one case on the CPU: dict(x, w, wp64, s, d, noise, noise_w, bias, s_next, rgb_w, rgb_s).
    w [1,Cout,Cin,3,3] is what prepack_split / prepack_wsplit take (DOWN3: the forward layer's [1, C planes, Cout, 3, 3], packed with
    adjoint='down'); wp64 [K channels, 9, Cout] fp64 = w / sqrt(9 cs) in conv_refs' packed layout, the references' weight.
    kind 'int': the exact inputs (weights k sqrt(9 cs), k from exact_weight_values); 'real': counter tensors; 'loud': those with x
    times 2^10 and d times 2^-10 (where the range plan of the generator puts activations: the fp16f8 cases)."""
    mode, B, cin, cout, H, W = c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W']
    cs = cout if mode == DOWN3 else cin
    i = R.conv_inputs('int' if kind == 'int' else 'real', mode, B, cin, cout, H, W, noise=c['noise'], bias=c['bias'], bcast=c['bcast'], seed=seed)
    root = float(np.sqrt(F32(cs) * F32(9)))
    if kind == 'int':
        good = exact_weight_values(cs, arith, even=c.get('f') == 2)
        k = i['wp']
        k = torch.where(torch.isin(k, torch.tensor(good, dtype=k.dtype)), k, torch.zeros_like(k))
        k.view(-1)[0], k.view(-1)[-1] = float(good[-1]), float(good[0])          # the corner weights stay non-zero
        i['wp64'] = k.double()
        wp32 = (k * root).float()
    else:
        from stylegan_directions_face_reenactment_amd import synthetic as S
        wp32 = S.counter_tensor(seed, 'sp.w.%d.%d.%d' % (mode, cin, cout), (cin, 9, cout))
        i['wp64'] = wp32.double() / root
        if kind == 'loud':
            i['x'] = i['x'] * 2.0 ** 10
            i['d'] = i['d'] * 2.0 ** -10
    if mode == DOWN3:       # wp[i = plane channel, t, o] = w[i, o, t]: the forward weight is indexed [C planes][Cout of the conv]
        i['w'] = wp32.permute(0, 2, 1).reshape(1, cin, cout, 3, 3).contiguous()
    else:
        i['w'] = _w_from_wp(wp32)
    del i['wp']
    key = 'sp.%d.%d.%d.%d.%d.%d' % (mode, B, cin, cout, H, W)
    if kind == 'int':
        i['s_next'] = choice_tensor(seed, key + 'sn', (B, cout), (0.5, 1.0, 2.0))
        i['rgb_w'] = int_tensor(seed, key + 'rw', (3, cout), -8, 8)
        i['rgb_s'] = choice_tensor(seed, key + 'rs', (B, cout), (0.5, 1.0, 2.0))
    else:
        from stylegan_directions_face_reenactment_amd import synthetic as S
        i['s_next'] = S.counter_tensor(seed, key + 'sn', (B, cout), 1.0, 0.3)
        i['rgb_w'] = S.counter_tensor(seed, key + 'rw', (3, cout))
        i['rgb_s'] = S.counter_tensor(seed, key + 'rs', (B, cout), 1.0, 0.3)
    return i


# ------------------------------------------------------------------ references with the bound of a split arithmetic

C_BASE = 10         # roundings beside the accumulation: the pack's scale, s * range shift, x * that, d * range shift, acc * d, the noise
#                     fma (2), bias, slack 2


def _ref_call(mode, x, wp64, s, d, noise, noise_w, bias, batch, c):
    if mode == PLAIN3:
        return R.plain3_ref(x, wp64, s, d, noise, noise_w, bias, batch=batch, c=c)
    if mode == UP3:
        return R.up3_ref(x, wp64, s, d, batch=batch, c=c)
    return R.down3_ref(x, wp64, s, d, c=c)


def split_terms(arith, mag, magw, magx, wmax):
    """What the split products add to the accumulation bound (module docstring): mag = sum |x s| |w| |d|, magw = sum |w| |d|,
    magx = sum |x s| |d| over the products of each element, wmax = max |w / sqrt(9 Cin)|."""
    t = 3 * STEP[arith] * mag
    if arith != 'bf16x3':
        t = t + 2.0 ** -20 * magw + 2.0 ** -30 * magx
    if arith == 'fp16f8':
        t = t + 2.0 ** -13 * mag + 2.0 ** -12 * magw + 2.0 ** -27 * wmax * magx
    return t


def conv_pieces(c, i, ksplit=1, bounds=True):
    """The arithmetic-independent part of conv_reference: dict(ref, acc, mag, magw, magx, wmax) before the activation (acc: the
    accumulation bound; bounds=False: the reference alone, for the exact checks)."""
    mode, B, cin = c['mode'], c['B'], c['cin']
    K = (4 if mode == UP3 else 9) * cin
    cc = C_BASE + ksplit + K * 2.0 ** -10
    d = None if mode == DOWN3 else i['d']
    ref, acc = _ref_call(mode, i['x'], i['wp64'], i['s'], d, i.get('noise'), i.get('noise_w'), i.get('bias'), B, cc)
    if not bounds:
        return dict(ref=ref)
    unit = (K + cc) * U
    one_x, one_s, one_w = torch.ones_like(i['x'][:1]), torch.ones_like(i['s']), torch.ones_like(i['wp64'])
    mag = _ref_call(mode, i['x'], i['wp64'], i['s'], d, None, None, None, B, cc)[1] / unit
    magw = _ref_call(mode, one_x, i['wp64'], one_s, d, None, None, None, B, cc)[1] / unit
    magx = _ref_call(mode, i['x'], one_w, i['s'], d, None, None, None, B, cc)[1] / unit
    return dict(ref=ref, acc=acc, mag=mag, magw=magw, magx=magx, wmax=float(i['wp64'].abs().max()))


def conv_finish(c, pc, arith, act=None):
    """(reference, bound) of the launch in one arithmetic from conv_pieces' dict."""
    act = c['act'] if act is None else act
    bound = pc['acc'] + split_terms(arith, pc['mag'], pc['magw'], pc['magx'], pc['wmax'])
    return R.apply_act(pc['ref'], bound, act and c['mode'] == PLAIN3, SLOPE, GAIN)


def conv_exact(c, pc, act=None):
    act = c['act'] if act is None else act
    return R.apply_act(pc['ref'], torch.zeros_like(pc['ref']), act and c['mode'] == PLAIN3, SLOPE, GAIN)[0]


def conv_reference(c, i, arith, ksplit=1, act=None):
    """(fp64 reference, per-element bound) of one direct split conv launch for the case c with the tensors i (any device).
    DOWN3: i['x'] the planes, i['s'] their per-channel scale (what planes_to_split applied), no d."""
    return conv_finish(c, conv_pieces(c, i, ksplit), arith, act)


def handover_reference(y_ref, y_bound, s_next, arith):
    """xs_out decoded = act(y) s_next within: the conv's own bound times |s_next|, and the form's step (split_step: the fp32
    multiply and what hi + lo may miss)."""
    sn = s_next.double()[:, :, None, None]
    ref = y_ref * sn
    return ref, y_bound * sn.abs() + split_step(ref, 'bf16x3' if arith == 'bf16x3' else 'fp16x3')


def rgb_reference(y_ref, y_bound, rgb_w, rgb_s):
    """The fused ToRGB partial sums, summed over the cout tiles = torgb_ref(y) without bias and skip.  Bound: torgb_ref's own (K = Cout,
    c = 8) with 4 more roundings for the kernel's table (w (s rsqrtf(Cout)): rsqrtf within one ulp) and its cross-wave sum, plus the
    conv's own error carried through |w s| / sqrt(Cout)."""
    cout = y_ref.shape[1]
    ref, bound = R.torgb_ref(y_ref, rgb_w.reshape(1, 3, cout, 1, 1), rgb_s)
    coef = (rgb_w.double().reshape(1, 3, cout) * rgb_s.double()[:, None, :]).abs() * wscale32(cout)
    carried = torch.einsum('bchw,bjc->bjhw', y_bound, coef)
    return ref, bound * (cout + 12) / (cout + 8) + carried


# ------------------------------------------------------------------ decoders of the documented operand forms (include/sgdfr.h)

def _dtype(arith):
    return torch.bfloat16 if arith == 'bf16x3' else torch.float16


def _shift(arith):
    return 1.0 if arith == 'bf16x3' else 16.0


def decode_xs(xs, B, C, H, W, arith):
    """xs [B][C/8][hi,lo][H W][8] int16 -> fp64 [B,C,H,W] = hi + lo with the range shift undone (fp16x3 / bf16x3)."""
    assert tuple(xs.shape) == (B, C // 8, 2, H * W, 8) and xs.dtype == torch.int16
    v = xs.view(_dtype(arith)).double()
    v = v[:, :, 0] + v[:, :, 1]
    return v.permute(0, 1, 3, 2).reshape(B, C, H, W) * _shift(arith)


def decode_ws(vs, B, C, H, W, f, arith):
    """The WS form [B][C/8][t f+2][hi,lo][H W/f][8] int16 -> fp64 V [B,C,f+2,H,W/f]."""
    assert tuple(vs.shape) == (B, C // 8, f + 2, 2, H * W // f, 8) and vs.dtype == torch.int16
    v = vs.view(_dtype(arith)).double()
    v = v[:, :, :, 0] + v[:, :, :, 1]                                 # [B, C/8, f+2, HT, 8]
    return v.permute(0, 1, 4, 2, 3).reshape(B, C, f + 2, H, W // f) * _shift(arith)


def decode_planes_il(y, B, cout, H, W, stride):
    """The interleaved padded planes [B][Cout][stride][px][py] (modconv_split returns them as [B,Cout,4,stride] flat) ->
    (planes [B,Cout,4,H+1,W+1] with phase 2 py + px, the padding positions [B,Cout,stride - (H+1)(W+1),4])."""
    RP = (H + 1) * (W + 1)
    il = y.reshape(B, cout, stride, 2, 2)
    planes = il[:, :, :RP].permute(0, 1, 4, 3, 2).reshape(B, cout, 4, H + 1, W + 1)
    return planes, il[:, :, RP:].reshape(B, cout, stride - RP, 4)


# ------------------------------------------------------------------ the Winograd forms F(f,3) along rows (csrc/wsplit.hip, csrc/common.h)

WS_BT = {2: torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64),
         4: torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                          [0, 4, 0, -5, 0, 1]], dtype=torch.float64)}
WS_G = {2: torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64),
        4: torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=torch.float64) / 24}
WS_AT = {2: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64),
         4: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)}
WSPLIT_GROWTH_LOG2 = {2: 1, 4: 4}      # functional.WSPLIT_GROWTH_LOG2: |B^T d| <= 2 / 10 max|d|


def ws_input_ref(xs, f):
    """V [B,C,f+2,H,W/f] = B^T d per tile of f outputs, d_j = xs[.., f tile - 1 + j] (zero outside the row); xs = x s in fp64."""
    d = R._pad(xs, 0, 0, 1, 1).unfold(3, f + 2, f)                     # [B,C,H,TW,f+2]
    return torch.einsum('tj,bchwj->bcthw', WS_BT[f].to(xs.device), d)


def ws_conv(V, w64, f, absolute=False):
    """A^T ((V rows a + ky - 1) (.) (G w[ky])) summed over ky and Cin -> [B,Cout,H,W]; V [B,C,f+2,H,TW], w64 [Cout,Cin,3,3] scaled.
    absolute: every matrix and operand by magnitude (the bound's mag)."""
    G, AT = WS_G[f].to(V.device), WS_AT[f].to(V.device)
    if absolute:
        G, AT, V, w64 = G.abs(), AT.abs(), V.abs(), w64.abs()
    Uw = torch.einsum('tk,ocyk->ocyt', G, w64)                         # [Cout,Cin,ky,t]
    B, C, T, H, TW = V.shape
    Vp = V.new_zeros(B, C, T, H + 2, TW)
    Vp[:, :, :, 1:H + 1] = V
    M = None
    for ky in range(3):
        m = torch.einsum('bcthw,oct->bothw', Vp[:, :, :, ky:ky + H], Uw[:, :, ky])
        M = m if M is None else M + m
    Y = torch.einsum('jt,bothw->bohwj', AT, M)
    return Y.reshape(B, Uw.shape[0], H, TW * f)


def wsplit_reference(c, i, arith):
    """(reference, bound) of one modconv_wsplit launch: the reference is plain3_ref's; the bound is the Winograd algorithm on
    absolute values (module docstring), K = 3 Cin products per transform-domain element, c = 24: the pack (scale, up to 4 of G), the
    input transform (s * shift, x * that, up to 3), the output transform (up to 5), * d, the noise fma (2), bias, slack 5."""
    f, B, cin = c['f'], c['B'], c['cin']
    ref, _ = R.plain3_ref(i['x'], i['wp64'], i['s'], i['d'], i.get('noise'), i.get('noise_w'), i.get('bias'), batch=B)
    w64 = i['wp64'].permute(2, 0, 1).reshape(c['cout'], cin, 3, 3)
    xs = R._bx(i['x'].double(), B) * i['s'].double()[:, :, None, None]
    V = torch.einsum('tj,bchwj->bcthw', WS_BT[f].abs().to(xs.device), R._pad(xs.abs(), 0, 0, 1, 1).unfold(3, f + 2, f))      # |B^T| |d|
    dd = i['d'].double().abs()[:, :, None, None]
    mag = ws_conv(V, w64, f, True) * dd
    magw = ws_conv(torch.ones_like(V[:1]), w64, f, True) * dd
    magx = ws_conv(V, torch.ones_like(w64), f, True) * dd
    K = 3 * cin
    extra = 0
    if i.get('noise') is not None:
        extra = extra + (i['noise'].double() * float(i['noise_w'].double().reshape(-1)[0])).abs()
    if i.get('bias') is not None:
        extra = extra + i['bias'].double().abs()[None, :, None, None]
    bound = (K * (1 + 2.0 ** -10) + 24) * U * (mag + extra) + split_terms(arith, mag, magw, magx, float(w64.abs().max()))
    return R.apply_act(ref, bound, c['act'], SLOPE, GAIN)


# ------------------------------------------------------------------ the cases

def C(mode, B, cin, cout, H, W, **kw):
    """One case; the options rotate over the cases as conv_refs.C does.  xin: also run with a pre-split input; f8: fp16f8 too."""
    kw.setdefault('noise', ('none', 'shared', 'per')[(B + cin + H + W) % 3] if mode == PLAIN3 else 'none')
    kw.setdefault('bias', bool((cout // 32 + W) % 2) and mode == PLAIN3)
    kw.setdefault('act', bool((cin // 16 + H) % 2) and mode == PLAIN3)
    kw.setdefault('bcast', False)
    kw.setdefault('with_d', mode == DOWN3 or bool((B + H + cout // 32) % 2 == 0) or mode == UP3)
    return dict(mode=mode, B=B, cin=cin, cout=cout, H=H, W=W, **kw)


def case_id(c):
    return '%s-B%d-%dto%d-%dx%d%s%s' % (('plain', 'up', 'down')[c['mode']], c['B'], c['cin'], c['cout'], c['H'], c['W'],
                                        '-bcast' if c['bcast'] else '', '-f%d' % c['f'] if c.get('f') else '')


PLAIN_CASES = [
    C(PLAIN3, 1, 16, 64, 4, 4), C(PLAIN3, 3, 16, 64, 4, 4),                      # 32 images per 512-pixel tile: one image, a ragged tile
    C(PLAIN3, 33, 16, 64, 4, 4, bcast=True),                                      # ... two tiles, the second ragged; constant input
    C(PLAIN3, 1, 16, 32, 4, 4), C(PLAIN3, 3, 16, 96, 8, 8),                       # the half cout tile, alone and after a full one
    C(PLAIN3, 2, 16, 64, 8, 4), C(PLAIN3, 2, 16, 64, 4, 8), C(PLAIN3, 1, 16, 64, 16, 32),      # H != W; whole rows of one image
    C(PLAIN3, 1, 16, 128, 4, 64), C(PLAIN3, 5, 16, 128, 4, 4), C(PLAIN3, 16, 16, 128, 4, 4),      # the 128 x 256 plan: rows, 16 images per tile (ragged, whole)
    C(PLAIN3, 1, 16, 64, 8, 128), C(PLAIN3, 1, 16, 64, 8, 192), C(PLAIN3, 1, 16, 64, 8, 512),  # 64-wide patches, 2 / 3 / 8 across
    C(PLAIN3, 1, 16, 128, 4, 128), C(PLAIN3, 2, 16, 32, 8, 128),                  # patches of the 128 x 256 plan; half tile on patches
    C(PLAIN3, 1, 64, 64, 4, 4), C(PLAIN3, 1, 112, 64, 4, 4), C(PLAIN3, 1, 512, 512, 4, 4, bcast=True),     # K slices 2, 3 (uneven), 16
    C(PLAIN3, 2, 64, 64, 8, 8), C(PLAIN3, 1, 256, 128, 8, 8),                     # exact weights at Cin = 64 and 256, K-sliced
]
# the plans only a pre-split input without K slices takes: 4-wave (cfg 8), 128 x 512 (cfg 6), and the persistent launch (>= 1024 tiles)
PLAIN_XIN_CASES = [C(PLAIN3, 8, 16, 64, 256, 256), C(PLAIN3, 4, 16, 128, 256, 256), C(PLAIN3, 64, 16, 128, 64, 64),
                   C(PLAIN3, 513, 16, 128, 4, 128)]
PLAIN_REFUSED = [(1, 16, 64, 6, 6), (1, 16, 64, 12, 12), (1, 16, 64, 24, 24), (1, 16, 64, 48, 48), (1, 16, 64, 8, 96), (1, 16, 64, 4, 128),
                 (1, 16, 64, 7, 128), (1, 8, 64, 4, 4), (1, 24, 64, 4, 4), (1, 16, 16, 4, 4), (1, 16, 48, 4, 4), (1, 16, 80, 4, 4)]
PLAIN_LAST = [((1, 16, 64, 8, 128), (1, 16, 64, 4, 128)), ((1, 16, 64, 8, 192), (1, 16, 64, 8, 96)), ((1, 16, 32, 4, 4), (1, 16, 16, 4, 4)),
              ((3, 16, 96, 8, 8), (3, 16, 80, 8, 8)), ((1, 16, 64, 4, 4), (1, 24, 64, 4, 4))]      # (last accepted, first refused) pairs

UP_CASES = [
    C(UP3, 1, 16, 64, 1, 1), C(UP3, 2, 16, 64, 2, 2), C(UP3, 3, 16, 64, 5, 7), C(UP3, 1, 16, 64, 15, 15), C(UP3, 3, 16, 32, 5, 7),
    C(UP3, 1, 16, 64, 3, 250), C(UP3, 1, 16, 64, 2, 512), C(UP3, 1, 16, 64, 2, 637), C(UP3, 1, 16, 64, 2, 700), C(UP3, 1, 16, 64, 2, 701),
    C(UP3, 1, 16, 128, 4, 4), C(UP3, 3, 16, 128, 5, 7), C(UP3, 2, 64, 64, 4, 4), C(UP3, 5, 16, 64, 7, 5, bcast=True),
    C(UP3, 16, 16, 64, 64, 64),                                                   # the deep plan: 265 tiles, tail round of 9
    C(UP3, 1, 16, 64, 255, 255), C(UP3, 1, 16, 64, 255, 256),                     # 256 tiles: no tail; 257: tail = 1
    C(UP3, 6, 16, 64, 127, 127), C(UP3, 5, 16, 64, 63, 307),                      # 384 tiles: tail = 128 (taken); 385: tail = 129 (not taken)
    C(UP3, 1, 16, 96, 127, 255),                                                  # deep plan with a half cout tile
]
UP_REFUSED = [(1, 16, 64, 2, 702), (1, 16, 128, 2, 702), (1, 8, 64, 4, 4), (1, 16, 48, 4, 4)]
UP_XIN_REFUSED = [(1, 16, 64, 2, 638), (1, 16, 64, 2, 700), (1, 16, 128, 4, 4)]

DOWN_CASES = [C(DOWN3, 1, 16, 128, 4, 4), C(DOWN3, 3, 16, 128, 5, 7), C(DOWN3, 2, 16, 128, 2, 300), C(DOWN3, 2, 16, 128, 2, 381),
              C(DOWN3, 2, 32, 256, 3, 5), C(DOWN3, 1, 16, 128, 127, 255), C(DOWN3, 1, 16, 128, 255, 257)]
#             (Cout = 256: exact weights; the last two: 256 tiles of 128 x 256 = whole rounds only; 258 = a tail round of two tiles, which
#              hold rows 254 and 255 of the (H+1) x (W+1) grid: a tail of one tile would hold the padding row alone and store nothing)
DOWN_REFUSED = [(2, 16, 128, 2, 382), (2, 16, 128, 2, 500), (1, 16, 64, 4, 4), (1, 16, 192, 4, 4), (1, 8, 128, 4, 4)]


def W(B, cin, cout, H, Wd, f, **kw):
    c = C(PLAIN3, B, cin, cout, H, Wd, **kw)
    c.update(f=f, with_d=True, bias=True if kw.get('wide') else c['bias'])
    c.setdefault('wide', False)
    return c


WSPLIT_CASES = [W(B, cin, 128, H, Wd, f) for f in (2, 4) for B, cin, H, Wd in
                ((1, 16, 16, 16), (3, 16, 8, 32), (1, 32, 8, 64), (2, 48, 16, 96), (1, 64, 16, 32))] + \
               [W(1, 64, 128, 16, 32, 4, wide=True), W(2, 96, 256, 16, 64, 4, wide=True)]
WSPLIT_REFUSED = [(1, 16, 128, 16, 12, 2), (1, 16, 128, 16, 12, 4), (1, 16, 128, 8, 16, 2), (1, 16, 128, 8, 16, 4), (1, 16, 128, 4, 32, 2),
                  (1, 16, 128, 4, 32, 4), (1, 16, 128, 16, 24, 2), (1, 16, 128, 16, 24, 4), (1, 16, 64, 16, 16, 2), (1, 8, 128, 16, 16, 2),
                  (1, 16, 128, 16, 18, 4)]
WSPLIT_LAST = [((1, 16, 128, 16, 16, 2), (1, 16, 128, 16, 14, 2)), ((1, 16, 128, 16, 16, 4), (1, 16, 128, 16, 12, 4)),
               ((1, 16, 128, 16, 16, 2), (1, 16, 128, 8, 16, 2)), ((1, 16, 128, 8, 32, 4), (1, 16, 128, 4, 32, 4))]


def all_direct_cases():
    return PLAIN_CASES + PLAIN_XIN_CASES + UP_CASES + DOWN_CASES

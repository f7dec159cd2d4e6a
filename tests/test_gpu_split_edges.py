"""The split-operand convolution path (csrc/split.hip, csrc/split_kernel.h, csrc/wsplit.hip, csrc/wswide.hip and the producers of their
inputs) at its plan, geometry and slice seams, each launch against a plain fp64 reference (tests/split_refs.py, itself checked on the
CPU by tests/test_cpu_split_edges.py, which also proves that the case lists reach every plan, geometry class, staging-slot count, slice
count and launch form, and finds every accept / refuse boundary from both sides).

Two kinds of check per case and arithmetic (split_refs.py):
  EXACT    integer operands with zero low terms (weights k sqrt(9 Cin) at Cin 16 / 64 / 256): fp16x3, bf16x3 and fp16f8 must return
           the fp64 value bit for bit, every word of the output;
  BOUNDED  counter-tensor operands within the a-priori per-element bound of the arithmetic (accumulation + 3 step + the fp16 floors +
           the e4m3 terms of fp16f8; the Winograd forms: the algorithm on absolute values).
The scope is the whole output.  The plane entries of UP3 outside the (2H+1) x (2W+1) result are STORED ZEROS (split_kernel.h stores
every position rem < (H+1)(W+1) of a plane; those read only the staged zero halo) and are held to it.  With plane_stride the
positions (H+1)(W+1) <= rem < plane_stride are UNSPECIFIED (ybase = -1: computed and dropped, never stored); exactly they are left out.

Every test prints its worst error / bound per group on a line starting with "split-edges" (pytest -s).  The figures measured on an
MI355X are in DESIGN.md section 2, "The split-operand path at its edges"."""
import pytest
import torch

import conv_refs as R
import split_refs as Q
from util import S  # noqa: F401  (also puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EX = dict(slope=Q.SLOPE, gain=Q.GAIN)
P3, U3, D3 = Q.PLAIN3, Q.UP3, Q.DOWN3
BIG = 1 << 22           # outputs above which a case checks its side outputs once (pre-split input, real operands) and runs no padded planes


def _F():
    from stylegan_directions_face_reenactment_amd import functional as F_
    return F_


def _say(what, **figures):
    print('split-edges %-52s %s' % (what, '  '.join('%s %.3g' % kv for kv in figures.items())))


def _dev(i):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in i.items()}


def _eq(y, ref64):
    return y.dtype == torch.float32 and y.shape == ref64.shape and torch.equal(y, ref64.float())


def _ratio(y, ref, bound):
    err = (y.double() - ref).abs()
    assert y.shape == ref.shape and bool((err[bound == 0] == 0).all()), 'error under a zero bound'
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


def _no_splitk(F_):
    return F_.using(F_.config().replace(use_splitk=False))


def _inputs(kind, c):
    i = _dev(Q.case_inputs(kind, c))
    if not c['with_d']:
        i['d'] = None
    return i


def _exact_capable(c):
    cs = c['cout'] if c['mode'] == D3 else c['cin']
    return cs in (16, 64, 256)


def _conv(F_, c, i, arith, xin, **kw):
    """One modconv_split call of the case: fp32 input, or the pre-split form made by to_split / planes_to_split."""
    mode, B, cin, cout, H, W = c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W']
    wsp = F_.prepack_split(i['w'], arith, adjoint='down' if mode == D3 else False)
    if mode == D3:
        xs = F_.planes_to_split(i['x'], i['s'], arith)
        return F_.modconv_split(xs, wsp, None, None, cout, mode=mode, arith=arith, x_split=(B, cin, H, W), batch=B)
    common = dict(noise=i['noise'], noise_weight=i['noise_w'], bias=i['bias'], activate=c['act'], mode=mode, arith=arith, batch=B, **EX, **kw)
    if xin:
        xs = F_.to_split(i['x'], i['s'], arith)
        return F_.modconv_split(xs, wsp, None, i['d'], cout, x_split=(B, cin, H, W), **common)
    return F_.modconv_split(i['x'], wsp, i['s'], i['d'], cout, **common)


def _check_outside(c, y, tag):
    if c['mode'] == U3:
        assert bool((y[:, :, R.planes_outside(c['H'], c['W'], DEV)] == 0).all()), (tag, 'entries outside the result are stored zeros')


def _check_side_outputs(F_, c, i, arith, xin, pc, kind, worst):
    """rgb_part, xs_out and want_y=False of a PLAIN3 launch without K slices, each against its reference."""
    B, cout, H, W = c['B'], c['cout'], c['H'], c['W']
    cid = Q.case_id(c)
    y_ref, y_bound = Q.conv_finish(c, pc, arith) if kind != 'int' else (Q.conv_exact(c, pc), torch.zeros_like(pc['ref']))
    with _no_splitk(F_):
        y, part, xs_out = _conv(F_, c, i, arith, xin, rgb=(i['rgb_w'], i['rgb_s']), s_next=i['s_next'])
        none_y, part2, xs2 = _conv(F_, c, i, arith, xin, rgb=(i['rgb_w'], i['rgb_s']), s_next=i['s_next'], want_y=False)
    assert none_y is None
    if kind == 'int':
        assert _eq(y, y_ref), (cid, arith, xin, 'y beside the side outputs')
    else:
        assert _ratio(y, y_ref, y_bound) <= 1.0, (cid, arith, xin, 'y beside the side outputs')
    a = (B, c['cin'], cout, H, W, P3)
    T = Q.cout_tiles(*a, xin_whole=xin)
    assert part.shape == (B, 3 * T, H, W) == part2.shape
    x_ref, x_bound = Q.handover_reference(y_ref, y_bound, i['s_next'], arith)
    r_ref, r_bound = Q.rgb_reference(y_ref, y_bound, i['rgb_w'], i['rgb_s'])
    for tag, pt, xo in (('', part, xs_out), (' want_y=False', part2, xs2)):
        got = Q.decode_xs(xo, B, cout, H, W, arith)
        if kind == 'int' and Q.split_fits(x_ref, arith):
            assert torch.equal(got, x_ref), (cid, arith, xin, 'xs_out exact' + tag)
        r = _ratio(got, x_ref, x_bound)
        assert r <= 1.0, (cid, arith, xin, 'xs_out' + tag, r)
        worst['xs_out ' + arith] = max(worst.get('xs_out ' + arith, 0.0), r)
        r = _ratio(pt.double().view(B, T, 3, H, W).sum(1), r_ref, r_bound)
        assert r <= 1.0, (cid, arith, xin, 'rgb_part' + tag, r)
        worst['rgb_part ' + arith] = max(worst.get('rgb_part ' + arith, 0.0), r)


def _check_direct(c, f8_kind='loud'):
    """Every launch form of a direct case in every arithmetic it has, EXACT then BOUNDED; prints and returns the worst ratios."""
    F_ = _F()
    lib = F_.N.load()
    mode, B, cin, cout, H, W = c['mode'], c['B'], c['cin'], c['cout'], c['H'], c['W']
    a = (B, cin, cout, H, W, mode)
    cid = Q.case_id(c)
    assert lib.sgdfr_modconv2d_split_supported(*a) == 1
    xin_ok = bool(lib.sgdfr_modconv2d_split_xin_supported(*a)) and not c['bcast']
    f8 = bool(lib.sgdfr_modconv2d_split_f8_ok(*a)) and xin_ok
    ks = lib.sgdfr_modconv2d_split_ksplit_hint(*a) if mode != D3 else 1
    big = B * cout * H * W * (4 if mode == U3 else 1) > BIG
    forms = ([] if mode == D3 else [('fp32', False, ks)]) + ([('xin', True, 1)] if xin_ok else [])
    worst = {}
    for kind in (['int'] if _exact_capable(c) else []) + ['real']:
        i = _inputs(kind, c)
        pcs = {k: Q.conv_pieces(c, i, k, bounds=kind != 'int') for k in {k for _, _, k in forms}}
        pc1 = pcs[1] if 1 in pcs else Q.conv_pieces(c, i, 1, bounds=kind != 'int')
        for arith in Q.ARITHS:
            for label, xin, k in forms:
                with (_no_splitk(F_) if (xin and ks > 1) else F_.using(F_.config())):
                    assert F_.config().use_splitk or xin
                    y = _conv(F_, c, i, arith, xin)
                tag = (cid, kind, arith, label, 'K/%d' % k)
                if kind == 'int':
                    ref = Q.conv_exact(c, pcs[k])
                    assert _eq(y, ref), tag + ('exact', float((y.double() - ref).abs().max()))
                else:
                    r = _ratio(y, *Q.conv_finish(c, pcs[k], arith))
                    assert r <= 1.0, tag + (r,)
                    worst[arith + ' ' + label] = max(worst.get(arith + ' ' + label, 0.0), r)
                _check_outside(c, y, tag)
            if mode == P3:
                for xin in ([True] if xin_ok and kind == 'real' and arith == 'fp16x3' else []) if big else ([False, True] if xin_ok else [False]):
                    _check_side_outputs(F_, c, i, arith, xin, pc1, kind, worst)
        if f8 and kind == 'int':
            y = _conv(F_, c, i, 'fp16f8', True)
            assert _eq(y, Q.conv_exact(c, pcs[1])), (cid, 'fp16f8 exact', float((y.double() - Q.conv_exact(c, pcs[1])).abs().max()))
            _check_outside(c, y, (cid, 'fp16f8'))
    if f8:      # as loud as the range plan of the generator leaves activations; the cross terms must not clamp (saturation word)
        i = _inputs(f8_kind, c)
        pc = Q.conv_pieces(c, i, 1)
        word = F_.new_saturation_word(torch.device(DEV))
        with F_.saturation_sink(word):
            y = _conv(F_, c, i, 'fp16f8', True)
            y3 = _conv(F_, c, i, 'fp16x3', True)
        assert int(word.item()) == 0, (cid, 'the loud inputs clamp')
        r8, r3 = _ratio(y, *Q.conv_finish(c, pc, 'fp16f8')), _ratio(y3, *Q.conv_finish(c, pc, 'fp16x3'))
        assert r8 <= 1.0 and r3 <= 1.0, (cid, 'loud', r8, r3)
        assert not torch.equal(y, y3)                   # the fp8 instantiation really ran
        worst['fp16f8 xin'], worst['fp16x3 xin loud'] = r8, r3
        _check_outside(c, y, (cid, 'fp16f8 loud'))
    _say(cid, **worst)
    return worst


@pytest.mark.parametrize('c', Q.PLAIN_CASES, ids=Q.case_id)
def test_plain3_plans_geometries_and_slices(c):
    _check_direct(c)


@pytest.mark.parametrize('c', Q.PLAIN_XIN_CASES, ids=Q.case_id)
def test_plain3_plans_of_the_pre_split_input(c):
    """The 4-wave plan (cfg 8, with fp16f8), the 128 x 512 plan (cfg 6, rows and 32 x 16 patches) and the persistent launch."""
    lib = _F().N.load()
    a = (c['B'], c['cin'], c['cout'], c['H'], c['W'], P3)
    info = lib.sgdfr_modconv2d_split_plan_info(*a, 1)
    assert info == Q.plan_info(*a, xin_whole=True) and (info & 15) in (0, 6, 8)
    _check_direct(c)


@pytest.mark.parametrize('c', Q.UP_CASES, ids=Q.case_id)
def test_up3_flat_space_plans_and_tail_rounds(c):
    _check_direct(c)


@pytest.mark.parametrize('c', [c for c in Q.UP_CASES if c['B'] * c['cout'] * c['H'] * c['W'] * 4 <= BIG], ids=Q.case_id)
def test_up3_padded_interleaved_planes(c):
    """plane_stride: the interleaved form [B][Cout][stride][px][py] against the same reference, EXACT and BOUNDED, fp32 and pre-split
    input; the stride padding (never stored: the buffer arrives full of NaN) is left out, nothing else."""
    F_ = _F()
    B, cin, cout, H, W = c['B'], c['cin'], c['cout'], c['H'], c['W']
    RP = (H + 1) * (W + 1)
    stride = (RP + 32) // 32 * 32                      # a multiple of 32 positions with at least one of padding
    xin_ok = bool(F_.N.load().sgdfr_modconv2d_split_xin_supported(B, cin, cout, H, W, U3)) and not c['bcast']
    worst = 0.0
    for kind in ('int', 'real'):
        i = _inputs(kind, c)
        pc = Q.conv_pieces(c, i, 1, bounds=kind != 'int')
        for arith in Q.ARITHS:
            for xin in ([False, True] if xin_ok else [False]):
                out = torch.full((B, cout, 4, stride), float('nan'), device=DEV)
                with _no_splitk(F_):
                    y = _conv(F_, c, i, arith, xin, plane_stride=stride, out=out)
                planes, pad = Q.decode_planes_il(y, B, cout, H, W, stride)
                assert pad.shape[2] == stride - RP >= 1
                if kind == 'int':
                    assert _eq(planes.contiguous(), Q.conv_exact(c, pc)), (Q.case_id(c), arith, xin)
                else:
                    r = _ratio(planes, *Q.conv_finish(c, pc, arith))
                    assert r <= 1.0, (Q.case_id(c), arith, xin, r)
                    worst = max(worst, r)
                _check_outside(c, planes, (Q.case_id(c), arith, xin))
    _say(Q.case_id(c) + ' plane_stride', worst=worst)


@pytest.mark.parametrize('c', Q.DOWN_CASES, ids=Q.case_id)
def test_down3_flat_space_and_tail_rounds(c):
    _check_direct(c)


# ------------------------------------------------------------------ the Winograd forms

def _wsplit(F_, c, i, arith, **kw):
    f, B, cin, cout, H, W = c['f'], c['B'], c['cin'], c['cout'], c['H'], c['W']
    vs = F_.to_wsplit(i['x'], i['s'], arith, f=f)
    wsp = F_.prepack_wsplit(i['w'], arith, f=f)
    return F_.modconv_wsplit(vs, (B, cin, H, W), wsp, i['d'], cout, i['noise'], i['noise_w'], i['bias'], c['act'], arith=arith, f=f, **EX, **kw)


@pytest.mark.parametrize('c', Q.WSPLIT_CASES, ids=lambda c: Q.case_id(c) + ('-wide' if c['wide'] else ''))
def test_winograd_forms_tile_widths_and_the_wide_kernel(c, monkeypatch):
    """F(2,3) and F(4,3), both patch widths of each, odd and even channel-block counts, the 64-tile and (SGDFR_WSPLIT_WIDE_NOW = 2, read
    per launch) the wide kernel: EXACT where G w stays integral (F(2,3), even weights), BOUNDED everywhere; fp16f8 on the wide kernel."""
    F_ = _F()
    f, B, cin, cout, H, W = c['f'], c['B'], c['cin'], c['cout'], c['H'], c['W']
    assert F_.N.load().sgdfr_modconv2d_wsplit_supported(B, cin, cout, H, W, f) == 1
    if c['wide']:
        monkeypatch.setenv('SGDFR_WSPLIT_WIDE_NOW', '2')
    worst = {}
    if f == 2 and cin in (16, 64, 256):
        i = _inputs('int', c)
        ref = R.plain3_ref(i['x'], i['wp64'], i['s'], i['d'], i['noise'], i['noise_w'], i['bias'], c['act'], batch=B, **EX)[0]
        for arith in Q.ARITHS:
            y = _wsplit(F_, c, i, arith)
            assert _eq(y, ref), (Q.case_id(c), arith, 'exact', float((y.double() - ref).abs().max()))
    i = _inputs('real', c)
    for arith in Q.ARITHS:
        ref, bound = Q.wsplit_reference(c, i, arith)
        y, part, xs_out = _wsplit(F_, c, i, arith, rgb=(i['rgb_w'], i['rgb_s']), s_next=i['s_next'])
        r = _ratio(y, ref, bound)
        assert r <= 1.0, (Q.case_id(c), arith, r)
        worst[arith] = r
        x_ref, x_bound = Q.handover_reference(ref, bound, i['s_next'], arith)
        rx = _ratio(Q.decode_xs(xs_out, B, cout, H, W, arith), x_ref, x_bound)
        r_ref, r_bound = Q.rgb_reference(ref, bound, i['rgb_w'], i['rgb_s'])
        rr = _ratio(part.double().view(B, cout // 128, 3, H, W).sum(1), r_ref, r_bound)
        assert rx <= 1.0 and rr <= 1.0, (Q.case_id(c), arith, 'xs_out', rx, 'rgb_part', rr)
        worst['xs_out ' + arith], worst['rgb ' + arith] = rx, rr
    if c['wide']:
        i = _inputs('loud', c)
        word = F_.new_saturation_word(torch.device(DEV))
        with F_.saturation_sink(word):
            y = _wsplit(F_, c, i, 'fp16f8')
        assert int(word.item()) == 0
        worst['fp16f8'] = _ratio(y, *Q.wsplit_reference(c, i, 'fp16f8'))
        assert worst['fp16f8'] <= 1.0, (Q.case_id(c), worst)
    _say(Q.case_id(c) + (' wide' if c['wide'] else ''), **worst)


# ------------------------------------------------------------------ the producers

PRODUCER_SHAPES = [(1, 16, 1, 1), (3, 16, 5, 7), (2, 8, 15, 15), (1, 24, 3, 250), (2, 16, 2, 701), (1, 16, 8, 128), (3, 16, 4, 4), (1, 16, 16, 32)]


@pytest.mark.parametrize('arith', Q.ARITHS)
def test_to_split_and_planes_to_split_forms(arith):
    """to_split and planes_to_split at the odd shapes of the conv cases: decoded == x s (gt d) on exact operands, within the form's step
    on real ones."""
    F_ = _F()
    worst = 0.0
    for B, C, H, W in PRODUCER_SHAPES:
        key = 'prod.%d.%d.%d.%d' % (B, C, H, W)
        for kind in ('int', 'real'):
            if kind == 'int':
                x = R.int_tensor(5, key + 'x', (B * C, H * W), -8, 8).view(B, C, H, W)
                g = R.int_tensor(5, key + 'g', (B * C, 4 * (H + 1) * (W + 1)), -8, 8).view(B, C, 4, H + 1, W + 1)
                s = R.choice_tensor(5, key + 's', (B, C), (0.5, 1.0, 2.0))
            else:
                x, g = S.counter_tensor(5, key + 'x', (B, C, H, W)), S.counter_tensor(5, key + 'g', (B, C, 4, H + 1, W + 1))
                s = S.counter_tensor(5, key + 's', (B, C), 1.0, 0.3)
            x, g, s = x.to(DEV), g.to(DEV), s.to(DEV)
            want = x.double() * s.double()[:, :, None, None]
            got = Q.decode_xs(F_.to_split(x, s, arith), B, C, H, W, arith)
            wantg = g.double() * s.double()[:, :, None, None, None]
            gotg = Q.decode_split_planes(F_.planes_to_split(g, s, arith), B, C, H, W, arith)
            got1 = Q.decode_split_planes(F_.planes_to_split(g, None, arith), B, C, H, W, arith)
            if kind == 'int':
                assert Q.split_fits(want, arith) and torch.equal(got, want) and torch.equal(gotg, wantg) and torch.equal(got1, g.double()), (key, arith)
            for a, b in ((got, want), (gotg, wantg), (got1, g.double())):
                r = _ratio(a, b, Q.split_step(b, arith))
                assert r <= 1.0, (key, arith, kind, r)
                worst = max(worst, r)
    _say('to_split / planes_to_split ' + arith, worst=worst)


@pytest.mark.parametrize('f', [2, 4])
@pytest.mark.parametrize('arith', Q.ARITHS)
def test_to_wsplit_form_and_its_row_border(arith, f):
    """V = B^T (x s) per tile, d_j zero outside the row: the first and last tile of every row are the point (a kernel that read the
    neighbour row's value there would differ in V_0 / V_{f+1} of those tiles, which are checked on their own)."""
    F_ = _F()
    worst = 0.0
    for B, C, H, W in ((1, 16, 16, 16), (3, 8, 5, 32), (2, 24, 3, 96), (1, 16, 1, 20), (2, 16, 7, 12)):
        key = 'wprod.%d.%d.%d.%d' % (B, C, H, W)
        for kind in ('int', 'real'):
            if kind == 'int':
                x = R.int_tensor(5, key + 'x', (B * C * H, W), -8, 8, nonzero=True).view(B, C, H, W)
                s = R.choice_tensor(5, key + 's', (B, C), (0.5, 1.0, 2.0))
            else:
                x, s = S.counter_tensor(5, key + 'x', (B, C, H, W)), S.counter_tensor(5, key + 's', (B, C), 1.0, 0.3)
            x, s = x.to(DEV), s.to(DEV)
            xs = x.double() * s.double()[:, :, None, None]
            want = Q.ws_input_ref(xs, f)
            got = Q.decode_ws(F_.to_wsplit(x, s, arith, f=f), B, C, H, W, f, arith)
            if kind == 'int':
                assert Q.split_fits(want, arith) and torch.equal(got, want), (key, arith, f)
                assert torch.equal(got[:, :, 0, :, 0], want[:, :, 0, :, 0]) and torch.equal(got[:, :, f + 1, :, -1], want[:, :, f + 1, :, -1])
            # beside the form's step, the transform's own fp32 roundings on sums of magnitude |B^T| |x s|: s * shift and x * that (2), up
            # to 3 adds / fmas, slack 1
            mag = torch.einsum('tj,bchwj->bcthw', Q.WS_BT[f].abs().to(DEV), R._pad(xs.abs(), 0, 0, 1, 1).unfold(3, f + 2, f))
            r = _ratio(got, want, Q.split_step(want, arith) + 6 * Q.U * mag)
            assert r <= 1.0, (key, arith, f, kind, r)
            worst = max(worst, r)
    _say('to_wsplit F(%d,3) %s' % (f, arith), worst=worst)


# ------------------------------------------------------------------ the refused side of every boundary

def test_first_refused_shapes_return_the_librarys_error():
    """The first shape beyond each boundary of tests/test_cpu_split_edges.py: a clean error from the entry point, no launch."""
    F_ = _F()
    lib = F_.N.load()

    def tensors(B, cin, cout, H, W, planes=False):
        x = torch.zeros((B, cin, 4, H + 1, W + 1) if planes else (B, cin, H, W), device=DEV)
        w = torch.zeros(1, cin if planes else cout, cout if planes else cin, 3, 3, device=DEV)
        return x, w, torch.ones(B, cin, device=DEV), torch.ones(B, cout, device=DEV)
    for mode, shapes in ((P3, Q.PLAIN_REFUSED), (U3, Q.UP_REFUSED)):
        for B, cin, cout, H, W in shapes:
            assert lib.sgdfr_modconv2d_split_supported(B, cin, cout, H, W, mode) == 0
            if cin % 16 or cout % 32:
                continue                                            # (the pack itself refuses such channels: below)
            x, w, s, d = tensors(B, cin, cout, H, W)
            with pytest.raises(RuntimeError, match='not supported'):
                F_.modconv_split(x, F_.prepack_split(w, 'fp16x3'), s, d, cout, mode=mode, arith='fp16x3')
    for B, cin, cout, H, W in Q.DOWN_REFUSED:
        assert lib.sgdfr_modconv2d_split_supported(B, cin, cout, H, W, D3) == 0
        if cin % 16 or cout % 64:
            continue
        g, w, dd, _ = tensors(B, cin, cout, H, W, planes=True)
        with pytest.raises(RuntimeError, match='not supported'):
            F_.modconv_split(F_.planes_to_split(g, dd, 'fp16x3'), F_.prepack_split(w, 'fp16x3', adjoint='down'), None, None, cout, mode=D3,
                             arith='fp16x3', x_split=(B, cin, H, W), batch=B)
    for B, cin, cout, H, W in Q.UP_XIN_REFUSED:                    # accepted with an fp32 input, refused pre-split
        assert lib.sgdfr_modconv2d_split_xin_supported(B, cin, cout, H, W, U3) == 0 and not F_.xin_ok(B, cin, cout, H, W, U3)
        x, w, s, d = tensors(B, cin, cout, H, W)
        with _no_splitk(F_), pytest.raises(RuntimeError, match='not built for tiling plan|LDS request'):
            F_.modconv_split(F_.to_split(x, s, 'fp16x3'), F_.prepack_split(w, 'fp16x3'), None, d, cout, mode=U3, arith='fp16x3',
                             x_split=(B, cin, H, W), batch=B)
    with pytest.raises(RuntimeError, match='prepack_split'):
        F_.prepack_split(torch.zeros(1, 48, 16, 3, 3, device=DEV), 'fp16x3')
    with pytest.raises(RuntimeError, match='prepack_split'):
        F_.prepack_split(torch.zeros(1, 64, 24, 3, 3, device=DEV), 'fp16x3')
    for B, cin, cout, H, W, f in Q.WSPLIT_REFUSED:
        assert lib.sgdfr_modconv2d_wsplit_supported(B, cin, cout, H, W, f) == 0
        if cin % 16 or cout % 128 or W % f:
            continue
        x, w, s, d = tensors(B, cin, cout, H, W)
        with pytest.raises(RuntimeError, match='not supported'):
            F_.modconv_wsplit(F_.to_wsplit(x, s, 'fp16x3', f=f), (B, cin, H, W), F_.prepack_wsplit(w, 'fp16x3', f=f), d, cout, arith='fp16x3', f=f)
    # fp16f8 where split_f8_ok says no
    x, w, s, d = tensors(1, 16, 64, 4, 4)
    assert lib.sgdfr_modconv2d_split_f8_ok(1, 16, 64, 4, 4, U3) == 0
    with pytest.raises(RuntimeError, match='FP16F8'):
        F_.modconv_split(F_.to_split(x, s, 'fp16f8'), F_.prepack_split(w, 'fp16f8'), None, d, 64, mode=U3, arith='fp16f8', x_split=(1, 16, 4, 4), batch=1)

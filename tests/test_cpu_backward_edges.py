"""Self-checks of the reference machinery of tests/test_gpu_backward_edges.py (tests/backward_refs.py), on the CPU: every fp64
reference is torch autograd of the forward expression it is the adjoint of, every exact case keeps its sums below 2^24 (and fits the
split forms), and the case lists cross every chunk, path, tile and grid edge from both sides."""
import pytest
import torch

import backward_refs as R
import conv_refs as CR
from util import O, S  # noqa: F401  (puts the repository root on sys.path)


def _close(a, b, tol=1e-12):
    return a.shape == b.shape and float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('B,C,H,W', [(2, 3, 1, 1), (1, 2, 2, 5), (2, 2, 5, 2), (1, 3, 4, 4), (2, 1, 3, 7)])
def test_blur_adjoint_ref_is_the_gradient_of_the_blur(B, C, H, W):
    for fir in R.real_firs() + R.exact_firs():
        i = R.blur_inputs('real', B, C, H, W)
        t = i['planes'].double().requires_grad_(True)
        y, _ = CR.blur_ref(t, fir)
        y.backward(i['g'].double())
        ref = R.blur_adjoint_ref(i['g'], fir, i['planes'])
        out = CR.planes_outside(H, W)
        assert ref['gt'].shape == (B, C, 4, H + 1, W + 1) and bool((ref['gt'][:, :, out] == 0).all())
        assert bool((ref['b_gt'][:, :, out] == 0).all())
        want = t.grad.clone()
        want[:, :, out] = 0             # (the forward reads its padding entries; their gradient is not part of dL/dT)
        assert _close(ref['gt'], want)
        assert _close(ref['asum'], (want * i['planes'].double()).sum((2, 3, 4)))
        assert bool((ref['gt'].abs() <= ref['b_gt'] / (16 * R.U) * (1 + 1e-12)).all())
        assert 'asum' not in R.blur_adjoint_ref(i['g'], fir)


@pytest.mark.parametrize('noise', ['none', 'shared', 'per'])
@pytest.mark.parametrize('bias', [True, False])
def test_act_grad_ref_is_the_gradient_of_the_fused_activation(noise, bias):
    B, C, HW = 3, 4, 37
    i = R.act_inputs('real', B, C, HW, noise, bias)
    y = S.counter_tensor(5, 'cpu.ag.y', (B, C, 1, HW)).double().requires_grad_(True)
    nw = (i['noise_w'] if noise != 'none' else torch.zeros(1)).double().requires_grad_(True)
    b = (i['bias'] if bias else torch.zeros(C)).double().requires_grad_(True)
    nz = i['noise'].double() if noise != 'none' else torch.zeros(1, 1, 1, HW, dtype=torch.float64)
    out = O.fused_leaky_relu(y + nw * nz, b, 0.2, 2 ** 0.5)
    assert bool((out != 0).all())
    out.backward(i['g'].double())
    sl, gn = float(R.F32(0.2)), float(R.F32(2 ** 0.5))       # the reference takes slope and gain at their fp32 values
    ref = R.act_grad_ref(i['g'], out.detach(), i['noise'], i['noise_w'], i['bias'], want_y=True)
    tol = 1e-7
    assert _close(ref['g_pre'], y.grad, tol)
    assert _close(ref['sums'][..., 0].sum(0), b.grad, tol)
    assert _close(ref['sums'][..., 1].sum().reshape(1), nw.grad, tol)
    assert _close(ref['sums'][..., 2], (ref['g_pre'] * y.detach()).sum((2, 3)), tol)
    assert abs(sl - 0.2) < 1e-8 and abs(gn - 2 ** 0.5) < 1e-7
    off = R.act_grad_ref(i['g'], out.detach(), i['noise'], i['noise_w'], i['bias'], want_y=False)
    assert bool((off['sums'][..., 2] == 0).all()) and torch.equal(off['sums'][..., :2], ref['sums'][..., :2])


def test_act_grad_ref_takes_the_slope_at_zero():
    g = torch.tensor([3.0, 3.0, 3.0]).view(1, 1, 1, 3)
    out = torch.tensor([1.0, 0.0, -1.0]).view(1, 1, 1, 3)
    ref = R.act_grad_ref(g, out, None, None, torch.tensor([5.0]), slope=0.25, gain=2.0, want_y=True)
    assert ref['g_pre'].view(-1).tolist() == [6.0, 1.5, 1.5]
    assert float(ref['sums'][0, 0, 2]) == 6.0 * (0.5 - 5) + 1.5 * (0 - 5) + 1.5 * (-2 - 5)
    for kind in ('exact', 'real'):
        assert bool((R.act_inputs(kind, 2, 3, 65)['out'] == 0).any()) and bool((R.join_inputs(kind, 2, 4, 65)['out'] == 0).any())


def test_reduction_refs_are_autograd_of_their_forward():
    B, C, HW = 3, 5, 19
    i = R.reduce_inputs('real', 'scale', B, C, HW)
    x, s = i['x'].double().requires_grad_(True), i['s'].double().requires_grad_(True)
    (x * s[:, :, None, None]).backward(i['gu'].double())
    ref = R.scale_reduce_ref(i['gu'], i['x'], i['s'])
    assert _close(ref['dx'], x.grad) and _close(ref['r'], s.grad)
    ib = R.reduce_inputs('real', 'scale', B, C, HW, bcast=True)
    assert torch.equal(R.scale_reduce_ref(ib['gu'], ib['x'], ib['s'])['r'], R.scale_reduce_ref(ib['gu'], ib['x'].repeat(B, 1, 1, 1), ib['s'])['r'])
    for cin in (1, 3, 4, 64):
        i = R.reduce_inputs('real', 'torgb', B, cin, HW)
        x, s, w = (i[k].double().requires_grad_(True) for k in ('x', 's', 'w_rgb'))
        y, _ = CR.torgb_ref(x, w, s)
        y.backward(i['g'].double())
        ref = R.torgb_bwd_ref(i['x'], i['g'], i['w_rgb'], i['s'])
        sc = R.wscale32(cin)
        assert _close(ref['dx'], x.grad) and ref['r'].shape == (B, 3, cin)
        assert _close((ref['r'] * w.detach() * sc).sum(1), s.grad)
        assert _close((ref['r'] * s.detach()[:, None, :] * sc).sum(0), w.grad)


@pytest.mark.parametrize('terms', R.TERM_SUBSETS, ids='+'.join)
def test_grad_join_ref_is_the_composition_of_the_three(terms):
    B, C, HW = 2, 8, 21
    for kind in ('exact', 'real'):
        i = R.join_inputs(kind, B, C, HW, terms, noise='per')
        kw = dict(slope=R.SLOPE, gain=R.GAIN) if kind == 'exact' else {}
        ref = R.grad_join_ref(want_y=True, **i, **kw)
        g = torch.zeros(B, C, 1, HW, dtype=torch.float64)
        if 'gu' in terms:
            sr = R.scale_reduce_ref(i['gu'], i['out'], i['s_next'])
            g = g + sr['dx']
            assert _close(ref['r_next'], sr['r'])
        if 'rgb' in terms:
            tb = R.torgb_bwd_ref(i['out'], i['g_rgb'], i['w_rgb'], i['s_rgb'])
            g = g + tb['dx']
            assert _close(ref['r_rgb'], tb['r'])
        if 'add' in terms:
            g = g + i['g_add'].double()
        act = R.act_grad_ref(g, i['out'], i['noise'], i['noise_w'], i['bias'], want_y=True, **kw)
        assert _close(ref['g_pre'], act['g_pre']) and _close(ref['sums'], act['sums'])
        assert ('r_next' in ref) == ('gu' in terms) and ('r_rgb' in ref) == ('rgb' in terms)
        assert bool((ref['b_pre'] >= act['b_pre'] * (1 - 1e-12)).all())         # the sum of |terms| bounds |their sum|


def test_prepack_t_ref_is_flip_and_permute():
    for cout, cin, k in ((3, 5, 3), (4, 2, 1), (2, 7, 3)):
        w = S.counter_tensor(7, 'cpu.pt.%d' % cin, (cout, cin, k, k))
        assert torch.equal(R.prepack_t_ref(w, 0), w.double().reshape(cout, cin, k * k).permute(0, 2, 1))
        assert torch.equal(R.prepack_t_ref(w, 1), w.double().flip(-1, -2).reshape(cout, cin, k * k).permute(0, 2, 1))
    for cin in (4, 16, 64):
        assert R.wscale32(cin) * R.wscale32(cin) * cin == 1.0


@pytest.mark.parametrize('arith', ['bf16x3', 'fp16x3'])
def test_split_decoders_invert_the_layouts(arith):
    B, C, H, W = 2, 16, 2, 3
    dt = torch.float16 if arith == 'fp16x3' else torch.bfloat16
    xsc = 16.0 if arith == 'fp16x3' else 1.0
    v = R.ints(3, 'cpu.dec', (B, C, 4, H + 1, W + 1), -300, 300).double() / 2
    hi = (v / xsc).to(dt)
    lo = (v / xsc - hi.double()).to(dt)
    assert torch.equal((hi.double() + lo.double()) * xsc, v) and R.split_fits(v, arith)
    G, RP = C // 8, (H + 1) * (W + 1)

    def lay(t):          # [B,C,4,RP] -> [B, ph G + c/8, RP, 8]
        return t.reshape(B, G, 8, 4, RP).permute(0, 3, 1, 4, 2).reshape(B, 4 * G, RP, 8)
    xs = torch.stack([lay(hi), lay(lo)], 2).contiguous().view(torch.int16)
    assert torch.equal(R.decode_split_planes(xs, B, C, H, W, arith), v)
    x4 = v[:, :, 0]                                                         # the plain form of one [B,C,H+1,W+1] map
    h4, l4 = (x4 / xsc).to(dt), (x4 / xsc - (x4 / xsc).to(dt).double()).to(dt)
    lay4 = lambda t: t.reshape(B, G, 8, RP).permute(0, 1, 3, 2)             # noqa: E731
    xs4 = torch.stack([lay4(h4), lay4(l4)], 2).contiguous().view(torch.int16)
    assert torch.equal(R.decode_split(xs4, (B, C, H + 1, W + 1), arith), x4)
    assert not R.split_fits(torch.tensor([2.0 ** 17 + 1.0]), 'bf16x3') and R.split_fits(torch.tensor([2.0 ** 17 + 4.0]), 'bf16x3')
    assert not R.split_fits(torch.tensor([2.0 ** 23 + 1.0]), 'fp16x3') and not R.split_fits(torch.tensor([2.0 ** -22]), 'fp16x3')


def test_every_exact_case_meets_its_condition():
    for B, C, HW, *_ in R.ACT_CASES:
        assert R.act_exact_condition(HW)
    n_exact = 0
    for c in R.JOIN_CASES:
        if c['exact']:
            assert R.join_exact_condition(c['C'], c['HW']), R.join_id(c)
            n_exact += 1
        assert c['exact'] or c['real'], R.join_id(c)
    assert n_exact >= len(R.JOIN_CASES) // 2
    assert not R.join_exact_condition(5, 64) and not R.join_exact_condition(16, 8192)
    for B, C, HW, _ in R.SCALE_CASES:
        assert R.reduce_exact_condition(HW)
    assert any(R.reduce_exact_condition(HW, cin) for _, cin, HW in R.TORGB_BWD_CASES)
    assert {cin for _, cin, HW in R.TORGB_BWD_CASES if R.reduce_exact_condition(HW, cin)} >= {1, 4, 64}
    shapes = ([(H, W) for H in R.BLUR_ADJ_H for W in R.BLUR_ADJ_W] + [R.BLUR_ADJ_STRIDE[2:]] + [(H, W) for H in R.SPLIT_H for W in R.SPLIT_W] +
              [c[2:] for c in R.SPLIT_STRIDE])
    for fir in R.exact_firs():
        for H, W in shapes:
            assert R.blur_exact_condition(H, W, fir), (H, W)
    assert not R.blur_exact_condition(64, 64, R.exact_firs()[0]) and not R.blur_exact_condition(1, 1, R.real_firs()[1])


@pytest.mark.parametrize('arith', ['bf16x3', 'fp16x3'])
def test_exact_blur_values_fit_the_split_forms(arith):
    for fir in R.exact_firs():
        for H, W in ((1, 1), (5, 33), (4, 64)):
            i = R.blur_inputs('exact', 2, 8, H, W)
            ref = R.blur_adjoint_ref(i['g'], fir)['gt']
            assert R.split_fits(ref * i['d'].double()[:, :, None, None, None], arith) and R.split_fits(ref, arith)


def test_the_case_lists_cross_every_edge_from_both_sides():
    hw = set(R.CHUNK_HW)
    assert {R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 63, 64, 65, 1} <= hw and max(hw) > 2 * R.CHUNK
    assert {R.chunks_of(v) for v in hw} == {1, 2, 3}
    waves = {R.waves_of(*c) for c in R.CHUNK_CASES}
    assert {1, 5, 7} <= waves and any(w % 4 == 0 for w in waves) and any(w % 4 for w in waves)
    for cases in (R.SCALE_CASES, R.TORGB_BWD_CASES, R.ACT_CASES):
        assert {c[2] for c in cases} >= hw
    assert {c['HW'] for c in R.JOIN_CHUNK_CASES} >= hw
    # act_grad_reduce: every noise kind, bias kind and want_y
    assert {c[3:] for c in R.ACT_CASES} >= {(n, b, w) for n in ('none', 'shared', 'per') for b in (True, False) for w in (True, False)}
    # grad_join: the seven subsets on a scalar and a float4 shape, with and without the workspace
    for path, want_hw in (('scalar', 2049), ('vec4', 2052)):
        for w in (False, True):
            got = {c['terms'] for c in R.JOIN_SUBSET_CASES if c['HW'] == want_hw and c['work'] == w}
            assert got == set(R.TERM_SUBSETS)
        assert all(R.join_path(c) in (path, 'rgb') for c in R.JOIN_SUBSET_CASES if c['HW'] == want_hw)
    assert {R.join_path(c) for c in R.JOIN_SUBSET_CASES} == {'scalar', 'vec4', 'rgb'}
    paths = {}
    for c in R.JOIN_PATH_CASES:
        paths.setdefault(R.join_path(c), []).append(c)
    assert set(paths) == {'rgb', 'vec4', 'scalar'}
    rgb = paths['rgb']
    assert R.join_path(R.J(2, 4, 1020)) == 'vec4' and R.join_path(R.J(2, 4, 1024)) == 'rgb'          # HW >= 1024 from both sides
    assert {1020, 1024} <= {c['HW'] for c in R.JOIN_PATH_CASES}
    assert {c['HW'] for c in rgb} >= {1024, 1028, 2048, 2052, 4096}
    assert {c['C'] % R.GJ_CPW for c in rgb} == {0, 1, 2, 3} and {c['C'] for c in rgb} >= {4, 5, 6, 7, 8, 16}
    assert {c['C'] for c in rgb if c['exact']} == {4, 16}
    assert any(c['HW'] % 256 for c in rgb) and any(c['HW'] % R.CHUNK % 256 == 4 for c in rgb)       # a last float4 row of one lane
    assert any('gu' not in c['terms'] for c in rgb) and any(c['noise'] == 'per' for c in rgb) and any(c['noise'] == 'none' for c in rgb)
    assert any(not c['want_y'] for c in rgb) and any(c['work'] for c in rgb)
    # what must leave the rgb path: g_add, a view one float into its storage, HW % 4 != 0
    left = [c for c in R.JOIN_PATH_CASES if 'rgb' in c['terms'] and c['HW'] >= 1024 and R.join_path(c) != 'rgb']
    assert any('add' in c['terms'] and not c['off'] and R.join_path(c) == 'vec4' for c in left)
    assert {c['off'] for c in left if c['off']} == {'gu', 'g_rgb', 'g_add'} and all(R.join_path(c) == 'scalar' for c in left if c['off'])
    assert any(c['HW'] % 4 and R.join_path(c) == 'scalar' for c in left)
    assert R.grad_join_path(1024, 1023, [0, 0, 0], True, False) == 'scalar' and R.grad_join_path(1024, 1024, [0, 0, 0], True, False) == 'rgb'
    # prepack_t: one block, its edge, and the grid cap
    n = sorted(co * ci * k * k for co, ci, k in R.PREPACK_T_CASES)
    assert n[0] < 256 and 256 in n and any(256 < v <= R.PREPACK_GRID_CAP * 256 for v in n)
    assert {(k, R.prepack_strides(co, ci, k)) for co, ci, k in R.PREPACK_T_CASES} == {(1, False), (3, False), (1, True), (3, True)}
    assert {ci for co, ci, k in R.PREPACK_T_CASES if k == 1} >= {4, 16, 64}
    # blur_adjoint: H != W, partial tail waves, a wave across two planes, the grid cap
    assert any(H != W for H in R.BLUR_ADJ_H for W in R.BLUR_ADJ_W)
    strips = {R.adjoint_strips(b * c, H, W) % 64 for H in R.BLUR_ADJ_H for W in R.BLUR_ADJ_W for b, c in R.BLUR_ADJ_PLANES}
    assert 0 in strips and len(strips) > 4
    assert {(H + 1) % R.ADJ_QV for H in R.BLUR_ADJ_H} == {0, 1, 2, 3}
    assert (1, 3) in R.BLUR_ADJ_PLANES and R.adjoint_strips(1, 2, 2) == 3                            # three planes in one wave
    B, C, H, W = R.BLUR_ADJ_STRIDE
    assert R.adjoint_strides(B * C, H, W) and R.adjoint_strips(B * C, H, W) == 2113800 and R.adjoint_tail(B * C, H, W) == (8, True)
    assert not any(R.adjoint_strides(3, H, W) for H in R.BLUR_ADJ_H for W in R.BLUR_ADJ_W)
    # blur_adjoint_split: QC 32 | 64, the column-W rule on and off, a second tile of two columns, the grid cap at both QC
    plans = {W: R.split_plan(2, 8, 4, W) for W in R.SPLIT_W}
    assert {(p['QC'], p['extra']) for p in plans.values()} == {(32, True), (32, False), (64, True), (64, False)}
    assert plans[63]['QC'] == 32 and plans[64]['QC'] == 64 and plans[32]['extra'] and not plans[33]['extra']
    assert plans[65]['col_tiles'] == 2 and plans[65]['last'] == 2 and plans[96]['col_tiles'] == 2 and plans[128]['col_tiles'] == 2
    assert plans[31]['col_tiles'] == 1 and plans[33]['col_tiles'] == 2 and plans[33]['last'] == 2 and plans[63]['col_tiles'] == 2
    assert {(H + 1 + 3) // 4 for H in R.SPLIT_H} == {1, 2}
    assert {R.split_plan(*c)['QC'] for c in R.SPLIT_STRIDE} == {32, 64} and all(R.split_plan(*c)['strides'] for c in R.SPLIT_STRIDE)
    assert not any(R.split_plan(3, 24, H, W)['strides'] for H in R.SPLIT_H for W in R.SPLIT_W)

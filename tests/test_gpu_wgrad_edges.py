"""GPU: the conv weight-gradient kernels of csrc/wgrad.hip at their plan, edge and finish seams, against the float64 restatement
(tests/wgrad_restatement.py) within bounds derived from the arithmetic, not measured.  The shapes are wgrad_restatement.CASES; what
they cover between them is asserted on the CPU (tests/test_cpu_wgrad_plan.py).

Four paths: 'parts+oik' (functional.wgrad's default on a shape the MFMA plan takes), 'parts+gather' (SGDFR_WGRAD_OIK=0), 'atomic'
(sgdfr_modconv_wgrad_f32 + sgdfr_modconv_wgrad_finish_f32 called directly on such a shape) and 'direct' (functional.wgrad on a shape
the plan refuses).  Each runs the argument variants
    'nodq' dq = None, d given           'nod'   d = None                    'dq'  dq given
    'a'    a given, contiguous          'astr'  a a column view (a_stride = 3)
    'x1'   x with one row, B > 1 (x_bstride = 0), with dq
and prints max(err / bound) per case."""
import pytest
import torch

from util import S
import wgrad_restatement as R

pytestmark = pytest.mark.gpu

SEED = 41
VARIANTS = ('nodq', 'nod', 'dq', 'a', 'astr', 'x1')
MFMA_CASES = [c for c in R.CASES if R.plan(*c) is not None]
UP_CASES = [c for c in R.CASES if c[5]]

_INPUTS, _REFS = {}, {}


def inputs(case):
    """CPU fp32 tensors of a case, keyed per case (cached: the references are computed from the same objects)."""
    if case not in _INPUTS:
        B, Cin, Cout, H, W, up = case
        key = 'wge.' + R.case_id(case) + '.'
        t = {'x': S.counter_tensor(SEED, key + 'x', (B, Cin, H, W)),
             's': S.counter_tensor(SEED, key + 's', (B, Cin), 1.0, 0.3),
             'd': S.counter_tensor(SEED, key + 'd', (B, Cout)).abs() * 0.5 + 0.25,
             'w': S.counter_tensor(SEED, key + 'w', (1, Cout, Cin, 3, 3)),
             'dq': S.counter_tensor(SEED, key + 'dq', (Cout, Cin)),
             'awide': S.counter_tensor(SEED, key + 'a', (B, Cout, 3))}
        if up:      # the plane entries outside the (2H+1) x (2W+1) image are zero here, 1e30 in `g_out`
            g = S.counter_tensor(SEED, key + 'g', (B, Cout, 4, H + 1, W + 1))
            out = R.outside_mask(H, W)
            t['g'] = g.masked_fill(out, 0.0)
            t['g_out'] = g.masked_fill(out, 1e30)
        else:
            t['g'] = S.counter_tensor(SEED, key + 'g', (B, Cout, H, W))
        _INPUTS[case] = t
    return _INPUTS[case]


def reference(case, variant):
    """(finish64 result, bound) of a variant, float64 on the CPU; the two contractions are computed once per operand set."""
    t = inputs(case)
    B, Cin, Cout, H, W, up = case
    ops = 'nod' if variant == 'nod' else 'x1' if variant == 'x1' else 'full'
    if (case, ops) not in _REFS:
        d = None if ops == 'nod' else t['d']
        x = t['x'][:1] if ops == 'x1' else t['x']
        _REFS[(case, ops)] = (R.dwc64(t['g'], d, x, t['s'], up), R.absdwc64(t['g'], d, x, t['s'], up))
    dwc, absdwc = _REFS[(case, ops)]
    p = R.plan(*case)
    K = 1 if p is None else p['K']
    if variant in ('nodq', 'nod'):
        return R.finish64(dwc, t['w'], None), R.bound64(B, H, W, K, absdwc)
    if variant in ('dq', 'x1'):
        return R.finish64(dwc, t['w'], t['dq']), R.bound64(B, H, W, K, absdwc, t['w'], t['dq'])
    a = t['awide'][:, :, 1]
    dq = R.dq64(a, t['d'], t['s'])
    return R.finish64(dwc, t['w'], dq), R.bound64(B, H, W, K, absdwc, t['w'], dq, R.absdq64(a, t['d'], t['s']))


def guarded(t):
    """A contiguous device copy of `t` in the middle of a buffer that holds 1e30 for one batch row on either side: a kernel that
    walks one image, row or column past its operand (a chunk range not clamped to the last chunk, a wrong edge test) reads the
    guard, inside the allocation, and the result is no longer finite."""
    pad = t[0].numel() + 64
    buf = torch.full((t.numel() + 2 * pad,), 1e30, device='cuda')
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def device_args(case, variant, g_key='g'):
    from stylegan_directions_face_reenactment_amd import functional as F_
    t = inputs(case)
    dev = {k: t[k].cuda() for k in ('w', 'dq', 'awide')}
    dev.update({k: guarded(t[k]) for k in ('s', 'd', g_key)})
    x = guarded(t['x'][:1] if variant == 'x1' else t['x'])
    kw = {'g': dev[g_key], 'd': None if variant == 'nod' else dev['d'], 'x': x, 's': dev['s'], 'weight': dev['w'],
          'wp': F_.prepack(dev['w'])[0], 'dq': dev['dq'] if variant in ('dq', 'x1') else None, 'a': None}
    if variant == 'a':
        kw['a'] = dev['awide'][:, :, 1].contiguous()
    elif variant == 'astr':
        kw['a'] = dev['awide'][:, :, 1]
        assert kw['a'].stride(1) == 3
    return kw


def run_functional(case, variant, g_key='g'):
    """functional.wgrad: parts + oik finish (or + gather finish under SGDFR_WGRAD_OIK=0) on an MFMA shape, else the direct kernel."""
    from stylegan_directions_face_reenactment_amd import functional as F_
    kw = device_args(case, variant, g_key)
    return F_.wgrad(kw['g'], kw['d'], kw['x'], kw['s'], case[2], bool(case[5]), wp=kw['wp'], dq=kw['dq'], weight=kw['weight'], a=kw['a'])


def run_atomic(case, variant, g_key='g'):
    """The C entries directly: sgdfr_modconv_wgrad_f32 (atomic combine on an MFMA shape) then sgdfr_modconv_wgrad_finish_f32."""
    from stylegan_directions_face_reenactment_amd import _native as N, functional as F_
    B, Cin, Cout, H, W, up = case
    kw = device_args(case, variant, g_key)
    dq = kw['dq'] if kw['a'] is None else F_.demod_dq(kw['a'], kw['d'], kw['s'])
    xb = 0 if (kw['x'].shape[0] == 1 and B != 1) else Cin * H * W
    dwp = torch.full((Cin, 9, Cout), float('nan'), device='cuda')           # the entry zeroes it itself
    dw = torch.empty(1, Cout, Cin, 3, 3, device='cuda')
    N.call('sgdfr_modconv_wgrad_f32', N.ptr(kw['g']), N.ptr(kw['d']), N.ptr(kw['x']), xb, N.ptr(kw['s']), N.ptr(dwp), B, Cin, Cout, H, W,
           N.MODE_UP3 if up else N.MODE_PLAIN3, N.stream())
    N.call('sgdfr_modconv_wgrad_finish_f32', N.ptr(dwp), N.ptr(kw['wp']), N.ptr(dq), N.ptr(dw), Cout, Cin, N.stream())
    return dw


def variants_of(case):
    return [v for v in VARIANTS if not (v == 'x1' and case[0] == 1)]


def check(case, path, run):
    """Every variant of a case on one path against the restatement: |err| <= bound elementwise (a zero bound asks for an exact zero).
    The bound (wgrad_restatement.bound64): m = B*H*W + K + 4 roundings on the |d*g| x |x*s| contraction, seven on the demodulation
    term, (B + 6) u on a dq formed in fp32; u = 2^-24."""
    worst = {}
    for variant in variants_of(case):
        want, bound = reference(case, variant)
        got = run(case, variant).double().cpu()[0]
        assert got.shape == want.shape and bool(torch.isfinite(got).all())
        err = (got - want).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
        worst[variant] = float(ratio.max())
    print('%s %s: max err / bound %.3f (%s)' % (path, R.case_id(case), max(worst.values()),
                                               ' '.join('%s %.3f' % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, (path, case, worst)


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_default_path_against_the_restatement(case):
    check(case, 'direct' if R.plan(*case) is None else 'parts+oik', run_functional)


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_gather_finish_against_the_restatement(case, monkeypatch):
    """SGDFR_WGRAD_OIK=0 is read per call: the same calls then finish through wgrad_finish_parts_kernel."""
    monkeypatch.setenv('SGDFR_WGRAD_OIK', '0')
    check(case, 'direct' if R.plan(*case) is None else 'parts+gather', run_functional)


@pytest.mark.parametrize('case', MFMA_CASES, ids=R.case_id)
def test_atomic_form_against_the_restatement(case):
    check(case, 'atomic', run_atomic)


def same_bits(a, b):
    """Equal values at every element: +0 and -0 are equal, a NaN equals nothing."""
    return torch.equal(a, b)


@pytest.mark.parametrize('case', MFMA_CASES, ids=R.case_id)
def test_bit_equalities_of_the_parts_path(case, monkeypatch):
    """What the comments of csrc/wgrad.hip claim: the slices are added in fixed order (the same bits twice); the oik finish that
    forms dq from (a, d, s) uses sgdfr_demod_dq_f32's expression and order (the same bits as given that kernel's dq); and with at
    most four slices each of the four slice groups of the oik finish holds at most one, so both finishes add the same values in the
    same order."""
    from stylegan_directions_face_reenactment_amd import functional as F_
    K = R.plan(*case)['K']
    oik = {v: run_functional(case, v) for v in ('dq', 'astr', 'nod')}
    for v in oik:
        assert same_bits(run_functional(case, v), oik[v]), ('oik twice', v)
    kw = device_args(case, 'astr')
    dq = F_.demod_dq(kw['a'], kw['d'], kw['s'])
    given = F_.wgrad(kw['g'], kw['d'], kw['x'], kw['s'], case[2], bool(case[5]), wp=kw['wp'], dq=dq, weight=kw['weight'])
    assert same_bits(oik['astr'], given), 'a form against demod_dq'
    assert same_bits(run_functional(case, 'a'), oik['astr']), 'a contiguous against a strided'
    monkeypatch.setenv('SGDFR_WGRAD_OIK', '0')
    gather = {v: run_functional(case, v) for v in oik}
    for v in oik:
        assert same_bits(run_functional(case, v), gather[v]), ('gather twice', v)
        if K <= 4:
            assert same_bits(gather[v], oik[v]), ('gather against oik', v, K)


@pytest.mark.parametrize('case', UP_CASES, ids=R.case_id)
def test_up_planes_outside_the_image_are_never_consumed(case, monkeypatch):
    """The kernel stages the last row of the odd-row planes and the last column of the odd-column planes but no tap reads them:
    1e30 there gives the bits of the zero-filled run, on every path."""
    for v in ('dq', 'nod'):
        assert same_bits(run_functional(case, v, 'g_out'), run_functional(case, v)), v
    if R.plan(*case) is not None:
        monkeypatch.setenv('SGDFR_WGRAD_OIK', '0')
        assert same_bits(run_functional(case, 'dq', 'g_out'), run_functional(case, 'dq'))
        # the atomic form adds in no fixed order: within the bound of the zero-filled reference instead
        want, bound = reference(case, 'dq')
        got = run_atomic(case, 'dq', 'g_out').double().cpu()[0]
        assert bool(((got - want).abs() <= bound).all())


def test_refusals():
    from stylegan_directions_face_reenactment_amd import _native as N
    z = torch.zeros(4096, device='cuda')
    p, st = N.ptr(z), N.stream()
    with pytest.raises(RuntimeError, match='shape needs the direct kernel'):
        N.call('sgdfr_modconv_wgrad_parts_f32', p, p, p, 8 * 4 * 6, p, p, 2, 8, 8, 4, 6, N.MODE_PLAIN3, st)
    with pytest.raises(RuntimeError, match='shape needs the direct kernel'):
        N.call('sgdfr_modconv_wgrad_parts_f32', p, p, p, 6 * 3 * 5, p, p, 2, 6, 10, 3, 5, N.MODE_UP3, st)
    for entry in ('sgdfr_modconv_wgrad_parts_f32', 'sgdfr_modconv_wgrad_f32'):
        for mode in (N.MODE_DOWN3, 3, -1):
            with pytest.raises(RuntimeError, match='mode must be PLAIN3 or UP3, got %d' % mode):
                N.call(entry, p, p, p, 8 * 4 * 4, p, p, 1, 8, 8, 4, 4, mode, st)
    with pytest.raises(RuntimeError, match=r'give dq OR \(a, d, s\), not both'):
        N.call('sgdfr_modconv_wgrad_finish_parts_oik_f32', p, 1, p, p, p, 1, p, p, 1, p, 8, 8, st)
    for d, s, B, stride in ((None, p, 1, 1), (p, None, 1, 1), (p, p, 0, 1), (p, p, 1, 0)):
        with pytest.raises(RuntimeError, match='a needs d, s, B and a_stride >= 1'):
            N.call('sgdfr_modconv_wgrad_finish_parts_oik_f32', p, 1, p, None, p, stride, d, s, B, p, 8, 8, st)
    with pytest.raises(RuntimeError, match='wgrad_finish_parts_oik: null pointer'):
        N.call('sgdfr_modconv_wgrad_finish_parts_oik_f32', p, 1, None, p, None, 1, None, None, 1, p, 8, 8, st)
    torch.cuda.synchronize()
    assert float(z.abs().max()) == 0.0          # refused before any launch

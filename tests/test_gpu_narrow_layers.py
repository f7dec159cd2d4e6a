"""The generator backward on the 32- and 16-channel layers of the 512^2 and 1024^2 generators, at test size (tests/narrow_cases.py;
the routes are checked and printed on the CPU by tests/test_cpu_narrow_routes.py): every per-layer case through StyledConv, and two
narrow generators through autograd.SynthesisFn and the per-layer Functions, against torch autograd of the fp64 oracle -- with the
project's own bars (tests/test_gpu_backward.py, tests/test_gpu_generator.py) -- and one PTI step sequence eager against captured.
Every per-layer test also asserts that the forward and dL/dx launches that ran are the ones the route table names.

FP32_LIMITED lists the comparisons that take the rule of tests/test_gpu_pool_loss.py instead of the project bar -- 8 x the deviation
of the oracle itself run in fp32 on the same inputs -- which is allowed only where that deviation alone exceeds the project bar."""
import copy

import pytest
import torch

import narrow_cases as NC
from util import O, S, SEED, maxabs

IMG_TOL = 2e-4          # the bar of tests/test_gpu_generator.py


@pytest.fixture(autouse=True, params=['fp16x3', 'fp32'])
def _both_arithmetics(request):
    from stylegan_directions_face_reenactment_amd import functional as F_
    with F_.precision(request.param):
        yield


pytestmark = pytest.mark.gpu

# (test, tensor) -> reason.  Empty: every comparison below holds the project bar as measured on an MI355X (figures in DESIGN.md).
FP32_LIMITED = {}


def _rel(a, b):
    return maxabs(a, b) / max(float(b.detach().abs().max()), 1e-12)


def _tol():
    from stylegan_directions_face_reenactment_amd import functional as F_
    return 2e-4 if F_.PRECISION == 'fp16x3' else 5e-3


def _check(test, name, err, bar, dev32):
    """err <= bar, or for a comparison listed in FP32_LIMITED <= 8 x dev32() (the fp32 oracle's own relative deviation from the fp64
    one, which must itself exceed the bar).  Prints the figure first; a miss also prints the fp32 oracle's deviation."""
    print('  %-28s %-34s %.2e  (bar %.0e)' % (test, name, err, bar))
    if (test, name) in FP32_LIMITED:
        dev = dev32()
        print('  %-28s %-34s fp32 oracle deviates %.2e: bar 8 x that' % (test, name, dev))
        assert dev > bar, (test, name, 'is listed in FP32_LIMITED, but the fp32 oracle is within the bar: %.2e' % dev)
        bar = 8 * dev
    elif err > bar:
        print('  %-28s %-34s MISS; the fp32 oracle deviates %.2e from the fp64 one' % (test, name, dev32()))
    assert err <= bar, (test, name, err, bar)


# ------------------------------------------------------------------ per layer

LAYER_GRADS = ('conv.modulation.weight', 'conv.modulation.bias', 'noise.weight', 'activate.bias')
_LAYER = {}


def _layer_case(case):
    """The inputs of one case and the fp64 autograd results, computed once for both arithmetics: dx, dstyle and the small gradients
    under the upstream gradient g; dL/dW under g masked where the output is within 1e-5 of the leaky ReLU's kink
    (test_conv_weight_gradient); the same from the oracle in fp32 on demand (dev32)."""
    if case in _LAYER:
        return _LAYER[case]
    from stylegan_directions_face_reenactment_amd.model import StyledConv
    cin, cout, h, up, B = case
    key = 'nl.%d.%d.%d.%d.%d' % (cin, cout, h, up, B)
    m = StyledConv(cin, cout, 3, 64, upsample=up)
    sd = {k: S.counter_tensor(27, key + k, tuple(v.shape)) for k, v in m.state_dict().items() if 'kernel' not in k}
    sd['conv.modulation.bias'] = sd['conv.modulation.bias'] * 0.1 + 1.0
    sd['noise.weight'] = sd['noise.weight'] * 0.1 + 0.1
    if up:
        sd['conv.blur.kernel'] = m.conv.blur.kernel
    r = 2 * h if up else h
    c = dict(sd=sd, x=S.counter_tensor(27, key + 'x', (B, cin, h, h)), st=S.counter_tensor(27, key + 's', (B, 64)),
             nz=S.counter_tensor(27, key + 'n', (1, 1, r, r)), g=S.counter_tensor(27, key + 'g', (B, cout, r, r)))

    def oracle(dtype, gm=None):
        P = {'L.' + k: v.to(dtype).requires_grad_('kernel' not in k) for k, v in sd.items()}
        xr, sr = c['x'].to(dtype).requires_grad_(True), c['st'].to(dtype).requires_grad_(True)
        yo = O.styled_conv(P, 'L', xr, sr, c['nz'].to(dtype), upsample=up)
        if gm is None:
            gm = c['g'] * (yo.detach().abs() > 1e-5).float()
        (yo * c['g'].to(dtype)).sum().backward(retain_graph=True)
        out = {'dx': xr.grad.clone(), 'dstyle': sr.grad.clone()}
        out.update({k: P['L.' + k].grad.clone() for k in LAYER_GRADS})
        P['L.conv.weight'].grad = None
        (yo * gm.to(dtype)).sum().backward()
        out['conv.weight'] = P['L.conv.weight'].grad.clone()
        return out, gm

    c['ref'], c['gm'] = oracle(torch.float64)

    def dev32(name):
        if 'ref32' not in c:
            c['ref32'] = oracle(torch.float32, c['gm'])[0]
        return _rel(c['ref32'][name], c['ref'][name])
    c['dev32'] = dev32
    _LAYER[case] = c
    return c


def _layer_run(m, c, g, timer=None):
    """One forward + backward of the StyledConv on the device; timer: a timing.LaunchTimer that collects the conv launches of both
    (autograd runs the backward on its own thread: the collector is entered there by a hook on the output and left by one on x)."""
    from stylegan_directions_face_reenactment_amd import timing
    m.zero_grad()
    xh, sh = c['x'].cuda().requires_grad_(True), c['st'].cuda().requires_grad_(True)
    if timer is None:
        out = m(xh, sh, noise=c['nz'].cuda())
    else:
        with timing.collect(timer):
            out = m(xh, sh, noise=c['nz'].cuda())
        scope = timing.collect(timer)

        def enter(_):
            scope.__enter__()

        def leave(_):
            scope.__exit__()
        out.register_hook(enter)
        xh.register_hook(leave)
    (out * g.cuda()).sum().backward()
    return xh.grad, sh.grad


@pytest.mark.parametrize('case', NC.PER_LAYER_CASES, ids=NC.case_id)
def test_narrow_layer_gradients_and_routes(case):
    """One StyledConv of a narrow shape: every gradient against fp64 autograd of O.styled_conv, and the launches against the table."""
    from stylegan_directions_face_reenactment_amd import functional as F_, timing
    from stylegan_directions_face_reenactment_amd.model import StyledConv
    cin, cout, h, up, B = case
    c = _layer_case(case)
    ref = c['ref']
    m = StyledConv(cin, cout, 3, 64, upsample=up)
    m.load_state_dict(c['sd'])
    m = m.cuda()
    ariths = ('fp16x3', 'bf16x3') if F_.PRECISION == 'fp16x3' else (None,)
    for arith in ariths:
        test = '%s [%s%s]' % (NC.case_id(case), F_.PRECISION, '/' + arith if arith else '')
        route = NC.layer_route(B, cin, cout, h, up, F_.PRECISION)
        timer = timing.LaunchTimer()
        with F_.using(F_.config().replace(backward_arith=arith) if arith else F_.config()):
            dx, ds = _layer_run(m, c, c['g'], timer)
            got = {'dx': dx, 'dstyle': ds}
            got.update({k: dict(m.named_parameters())[k].grad.clone() for k in LAYER_GRADS})
            _layer_run(m, c, c['gm'])
            got['conv.weight'] = m.conv.weight.grad.clone()
        torch.cuda.synchronize()
        descs = [d for _, _, _, d in timer.conv]
        print('  %-28s launches %s; table: forward %s, dL/dx %s' % (test, descs, NC.route_class(route)[1], route['dx']))
        assert NC.launches_of(descs) == (route['fwd'], route['dx']), (descs, route)
        if route['fwd'] == 'split':
            assert ('K/%d' % route['ksplit'] in descs[0]) == (route['ksplit'] > 1), (descs, route)
        assert got['conv.weight'].shape == (1, cout, cin, 3, 3)
        for name, bar in (('dx', 2e-5), ('dstyle', 5e-5)) + tuple((k, 5e-5) for k in LAYER_GRADS) + (('conv.weight', 1e-4),):
            _check(test, name, _rel(got[name], ref[name]), bar, lambda name=name: c['dev32'](name))
    assert F_.split_saturation_count(reset=True) == 0


# ------------------------------------------------------------------ the narrow generators

_GEN = {}


def _trainable(k):
    return not (k.startswith('style.') or k.startswith('noises.') or k.endswith('.kernel'))


def _gen_case(name):
    """Latents, truncation latent, target, and the fp64 oracle's image, loss L = mean((img - target)^2), dL/dW+ and every parameter
    gradient of a narrow generator, computed once for the module; the fp32 oracle's on demand."""
    if name in _GEN:
        return _GEN[name]
    spec = NC.NARROW[name]
    B, size = spec['B'], spec['size']
    state = NC.narrow_state(name)
    n_latent = 2 * (size.bit_length() - 1) - 2
    c = dict(B=B, size=size, w=S.synthetic_latents(51, B, n_latent=n_latent, key='nw.w' + name), tr=S.counter_tensor(51, 'nw.t', (1, 512)),
             target=torch.tanh(S.counter_tensor(51, 'nw.g' + name, (B, 3, size, size))))

    def oracle(dtype):
        P = {k: v.to(dtype).requires_grad_(_trainable(k)) for k, v in state.items()}
        wr = c['w'].to(dtype).requires_grad_(True)
        img, _ = O.generator_forward(P, [wr], input_is_latent=True, truncation=0.7, truncation_latent=c['tr'].to(dtype))
        loss = ((img - c['target'].to(dtype)) ** 2).mean()
        loss.backward()
        grads = {k: v.grad for k, v in P.items() if v.grad is not None}
        grads['W+'] = wr.grad
        return img.detach(), float(loss.detach()), grads
    c['img'], c['loss'], c['grads'] = oracle(torch.float64)

    def dev32(k):
        if 'grads32' not in c:
            c['img32'], _, c['grads32'] = oracle(torch.float32)
        if k == 'image':
            return maxabs(c['img32'], c['img'])
        if k.endswith('noise.weight'):
            return abs(float(c['grads32'][k]) - float(c['grads'][k])) / _nz_scale(c)
        return _rel(c['grads32'][k], c['grads'][k])
    c['dev32'] = dev32
    _GEN[name] = c
    return c


def _nz_scale(c):
    return max(float(g.abs().max()) for k, g in c['grads'].items() if k.endswith('noise.weight'))


def _hip_narrow(name):
    return NC.narrow_generator(name).cuda()


def _grad_run(G, c, fused):
    G.fused_backward = fused
    G.zero_grad()
    wh = c['w'].cuda().requires_grad_(True)
    img, _ = G([wh], input_is_latent=True, truncation=0.7, truncation_latent=c['tr'].cuda())
    assert (type(img.grad_fn).__name__ == 'SynthesisFnBackward') == fused
    loss = ((img - c['target'].cuda()) ** 2).mean()
    loss.backward()
    grads = {k: p.grad.clone() for k, p in G.named_parameters() if p.grad is not None}
    grads['W+'] = wh.grad.clone()
    return img.detach(), float(loss), grads


def _against_oracle(test, c, grads, keys):
    tol = _tol()
    nz = _nz_scale(c)
    for k in keys:
        if k.endswith('noise.weight'):          # (one scalar each: on the scale of the largest of them, test_gpu_backward.py)
            err, bar = abs(float(grads[k]) - float(c['grads'][k])) / nz, 10 * tol
        else:
            err, bar = _rel(grads[k], c['grads'][k]), tol
        _check(test, k, err, bar, lambda k=k: c['dev32'](k))


def test_n256_image_and_every_gradient():
    """N256 (64 channels up to 64^2, 32 at 128^2, 16 at 256^2), B = 2: the image under no_grad, from the whole-synthesis Function and from
    the per-layer Functions against the fp64 oracle; dL/dW+ and every parameter gradient of the fused path against fp64 autograd and
    against the per-layer path; nothing saturates."""
    from stylegan_directions_face_reenactment_amd import functional as F_
    test = 'N256 [%s]' % F_.PRECISION
    c = _gen_case('N256')
    G = _hip_narrow('N256')
    with torch.no_grad():
        img0, _ = G([c['w'].cuda()], input_is_latent=True, truncation=0.7, truncation_latent=c['tr'].cuda())
    _check(test, 'image, no_grad', maxabs(img0, c['img']), IMG_TOL, lambda: c['dev32']('image'))
    G.train()
    img_f, loss_f, fused_g = _grad_run(G, c, True)
    img_l, loss_l, layer_g = _grad_run(G, c, False)
    _check(test, 'image, fused Function', maxabs(img_f, c['img']), IMG_TOL, lambda: c['dev32']('image'))
    _check(test, 'image, per-layer Functions', maxabs(img_l, c['img']), IMG_TOL, lambda: c['dev32']('image'))
    print('  %-28s loss %.6f / %.6f, oracle %.6f' % (test, loss_f, loss_l, c['loss']))
    assert set(fused_g) == set(layer_g) == set(c['grads']) and len(fused_g) == 1 + 1 + 5 * 13 + 4 * 7
    _against_oracle(test + ' fused', c, fused_g, sorted(fused_g))
    # fused against per-layer: the bars of test_fused_backward_parameter_gradients_match_the_per_layer_functions
    pairs = [(_rel(fused_g[k], layer_g[k]), k) for k in fused_g if float(layer_g[k].abs().max()) > 0]
    worst = max(p for p in pairs if not p[1].endswith('noise.weight'))
    worst_nz = max(p for p in pairs if p[1].endswith('noise.weight'))
    print('  %-28s fused vs per-layer: worst rel %.2e (%s), noise strengths %.2e (%s), %d tensors' % ((test,) + worst + worst_nz + (len(pairs),)))
    assert worst[0] <= 1e-3, worst
    assert worst_nz[0] <= 1e-2, worst_nz
    assert G.saturated_pairs() == 0


N1024_KEYS = ('W+', 'conv1.conv.weight', 'convs.14.conv.weight', 'convs.15.conv.weight', 'convs.7.conv.modulation.weight',
              'to_rgbs.7.conv.weight', 'to_rgbs.7.bias', 'input.input')


def test_n1024_index_maps_of_17_layers():
    """N1024 (16 channels everywhere, 17 layers, 9 ToRGBs, 18 latent rows), B = 1: the fused path's image, dL/dW+ (every latent row) and the
    gradients at both ends of the parameter list against the fp64 oracle."""
    from stylegan_directions_face_reenactment_amd import functional as F_
    test = 'N1024 [%s]' % F_.PRECISION
    c = _gen_case('N1024')
    G = _hip_narrow('N1024').train()
    assert G.n_latent == 18 and len(G.convs) == 16 and len(G.to_rgbs) == 8
    img, loss, grads = _grad_run(G, c, True)
    _check(test, 'image, fused Function', maxabs(img, c['img']), IMG_TOL, lambda: c['dev32']('image'))
    print('  %-28s loss %.6f, oracle %.6f' % (test, loss, c['loss']))
    assert set(grads) == set(c['grads'])
    _against_oracle(test, c, grads, N1024_KEYS)
    rows = (grads['W+'].cpu().double() - c['grads']['W+']).abs().amax((0, 2)) / float(c['grads']['W+'].abs().max())
    print('  %-28s dL/dW+ per latent row: %s' % (test, ' '.join('%.1e' % float(v) for v in rows)))
    assert float(c['grads']['W+'].abs().amax((0, 2)).min()) > 0          # every row carries a gradient: a swapped row would show
    assert G.saturated_pairs() == 0


def test_pti_steps_on_n256_graph_replay_matches_eager():
    """finetune.optimize_g on N256 -- convs[4..11] are trained: the 64 -> 32, 32 -> 32, 32 -> 16 and 16 -> 16 layers among them -- 6 steps
    eager and as 3 warm-up steps + 3 replays of the captured step: same weights within the tolerances of
    test_pti_driver_graph_replay_matches_eager_steps, the loss falls, nothing else moves."""
    from stylegan_directions_face_reenactment_amd import finetune, functional as F_
    c = _gen_case('N256')
    G0 = _hip_narrow('N256')
    w, trunc = c['w'][:1].cuda(), c['tr'].cuda()
    with torch.no_grad():
        base, _ = G0([w], input_is_latent=True, truncation=0.7, truncation_latent=trunc)
    target = (base + 0.3 * S.counter_tensor(SEED, 'npti.d', tuple(base.shape)).cuda()).clamp(-1, 1)
    runs = {}
    for graph in (False, True):
        G = copy.deepcopy(G0)
        first = finetune.l2_loss_fn(G([w], input_is_latent=True, truncation=0.7, truncation_latent=trunc)[0], target, 100).item()
        G, loss = finetune.optimize_g(G, w, target, trunc, opt_steps=6, lr=1e-3, graph=graph)
        print('  N256 PTI [%s] graph=%s: loss %.6f -> %.6f' % (F_.PRECISION, graph, first, loss.item()))
        assert loss.item() < first
        runs[graph] = (G, loss.item())
    Ge, Gg = runs[False][0], runs[True][0]
    assert abs(runs[False][1] - runs[True][1]) <= 2e-3 * abs(runs[False][1])
    worst = 0.0
    for (k, a), (_, b), (_, c0) in zip(Ge.state_dict().items(), Gg.state_dict().items(), G0.state_dict().items()):
        moved = k.startswith('convs.') and 4 <= int(k.split('.')[1]) <= 11 and 'kernel' not in k
        if moved:
            worst = max(worst, float(((a - b).abs() / (2e-4 + 2e-3 * b.abs())).max()))
            assert torch.allclose(a, b, rtol=2e-3, atol=2e-4), k
            assert not torch.equal(a, c0), k
        else:
            assert torch.equal(a, c0) and torch.equal(b, c0), k
    print('  N256 PTI [%s]: eager vs replayed weights, worst |a - b| / (2e-4 + 2e-3 |b|) = %.2e, losses %.6f / %.6f'
          % (F_.PRECISION, worst, runs[False][1], runs[True][1]))

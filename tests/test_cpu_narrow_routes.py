"""Which launches the 32- and 16-channel layers of the 512^2 and 1024^2 generators take, forward and backward, and that small cases
take the same ones (tests/narrow_cases.py): the route function against the restated host rules of tests/split_refs.py, the route table
of the six real generators, of the per-layer cases and of the two narrow generators of tests/test_gpu_narrow_layers.py (printed: run
with -s), the coverage of every narrow route by a per-layer case and by a layer of N256, the effect of the `cin % 64` guard of
autograd._conv_input_grad, Generator(channels=...) itself, and the oracle on a narrow state against torch's fp64 convolutions."""
import pytest
import torch
import torch.nn.functional as TF

import narrow_cases as NC
import split_refs as Q
from util import O, S

PRECISIONS = ('fp16x3', 'fp32')


def _table(precision):
    """[(label, source, route)]: source 'real' | 'case' | the narrow generator's name."""
    rows = []
    for size, cm in NC.REAL_GENERATORS:
        for B in (1, 2):
            for name, cin, cout, h, up in NC.generator_layers(size, NC.reference_channels(cm)):
                rows.append(('G%d cm%d %s' % (size, cm, name), 'real', NC.layer_route(B, cin, cout, h, up, precision)))
    for c in NC.PER_LAYER_CASES:
        rows.append((NC.case_id(c), 'case', NC.layer_route(c[4], c[0], c[1], c[2], c[3], precision)))
    for n, spec in NC.NARROW.items():
        for name, cin, cout, h, up in NC.generator_layers(spec['size'], spec['channels']):
            rows.append(('%s %s' % (n, name), n, NC.layer_route(spec['B'], cin, cout, h, up, precision)))
    return rows


def test_route_function_agrees_with_the_restated_host_rules():
    """Where tests/split_refs.py restates a rule (environment at its defaults) the route function, which asks the library, says the same:
    the forward plan, its geometry class, the half tile, the K slices; split_supported of the dL/dx convs; cout tiles of a fused ToRGB."""
    n = 0
    for label, _, r in _table('fp16x3'):
        B, cin, cout, h, up = r['B'], r['cin'], r['cout'], r['h'], r['kind'] == 'up'
        mode = Q.UP3 if up else Q.PLAIN3
        g = Q.split_plan(B, cin, cout, h, h, mode)
        assert (r['fwd'] == 'split') == (g is not None), label
        if g is not None:
            assert (r['plan'], r['geometry'], r['half']) == (g['plan'].cfg, g['kind'], g['half']), label
            assert r['ksplit'] == Q.ksplit_hint(B, cin, cout, h, h, mode), label
            n += 1
        if up:
            assert (r['dx'] == 'split down3') == bool(Q.split_supported(B, cout, cin, h, h, Q.DOWN3)), label
        else:
            assert (r['dx'] == 'split3') == bool(cin % 64 == 0 and Q.split_supported(B, cout, cin, h, h, Q.PLAIN3)), label
            assert r['rgb'] == (g is not None and r['ksplit'] == 1), label
    assert n > 100
    for label, _, r in _table('fp32'):
        assert r['fwd'] in ('direct', 'wino') and r['dx'] in ('plain3', 'wino3', 'down3') and not r['rgb'], label


@pytest.mark.parametrize('precision', PRECISIONS)
def test_every_narrow_route_of_the_real_generators_is_reached_by_a_small_case(precision, capsys):
    rows = _table(precision)
    real = {}
    for label, src, r in rows:
        if src == 'real' and NC.is_narrow(r['cin'], r['cout']):
            real.setdefault(NC.route_class(r), []).append('%s B%d' % (label, r['B']))
    by_case = {NC.route_class(r) for _, src, r in rows if src == 'case'}
    by_n256 = {NC.route_class(r) for _, src, r in rows if src == 'N256'}
    with capsys.disabled():
        print('\n---- routes under precision %s (narrow real layers, every case, every layer of N256 and N1024)' % precision)
        print('%-22s %-20s | %-28s | %-11s | %-9s | ToRGB' % ('layer', '', 'forward', 'dL/dx', 'dL/dW'))
        for label, src, r in rows:
            if src != 'real' or NC.is_narrow(r['cin'], r['cout']):
                print(NC.format_route(label, r))
        for cls, who in sorted(real.items()):
            print('narrow class %s: %d real layers; per-layer case %s, N256 %s' % (cls, len(who), cls in by_case, cls in by_n256))
    assert real, 'the real generators have narrow layers'
    # fp16x3: up 64->32, plain 32->32, up 32->16, plain 16->16 are one class each over both multipliers and batches; fp32: up / plain
    assert len(real) == (4 if precision == 'fp16x3' else 2)
    for cls, who in real.items():
        assert cls in by_case, (cls, who)
        assert cls in by_n256, (cls, who)
    # ... and by a per-layer case with the real layer's K slices too (all narrow real layers run unsliced)
    sliced = {(NC.route_class(r), r['ksplit'] > 1) for _, src, r in rows if src == 'real' and NC.is_narrow(r['cin'], r['cout'])}
    assert sliced <= {(NC.route_class(r), r['ksplit'] > 1) for _, src, r in rows if src == 'case'}
    # the plans of the issue's table, by name
    if precision == 'fp16x3':
        want = {('plain', 'split cfg%d patch half' % Q.PLAIN_NARROW.cfg, 'plain3', 'sliced', 'rgb fused'),
                ('up', 'split cfg%d flat half' % Q.UP_NARROW.cfg, 'down3', 'sliced', '-'),
                ('up', 'direct', 'down3', 'sliced', '-'), ('plain', 'direct', 'plain3', 'sliced', 'rgb apart')}
        assert set(real) == want
        # every geometry class of the half tile is reached by a per-layer case
        assert {r['geometry'] for _, src, r in rows if src == 'case' and r['half'] and r['cin'] == 32} == {'images', 'rows', 'patch'}


def test_the_guard_keeps_half_tile_gradients_off_the_split_kernels():
    """A plain layer with cin % 64 == 32 (its dL/dx conv would need a half cout tile, which only the forward pack pads): forward on the
    half tile, dL/dx never on modconv_split -- over the table and a sweep; with cin % 64 == 0 and the same cout the split route is on."""
    from stylegan_directions_face_reenactment_amd import functional as F_
    seen = 0
    shapes = [(r['B'], r['cin'], r['cout'], r['h']) for _, _, r in _table('fp16x3') if r['kind'] == 'plain']
    shapes += [(B, cin, cout, h) for B in (1, 2, 5) for cin in (32, 96, 160) for cout in (32, 64, 96, 128) for h in (4, 8, 16, 32, 64, 128)]
    for B, cin, cout, h in shapes:
        if cin % 64 != 32:
            continue
        r = NC.layer_route(B, cin, cout, h, False)
        assert r['dx'] != 'split3', (B, cin, cout, h)
        if cout == cin:
            assert r['fwd'] == 'split' and r['half'], (B, cin, cout, h)
        with F_.precision('fp16x3'):
            seen += int(F_.split_ok(B, cout, cin, h, h))          # the query alone WOULD have admitted the dL/dx conv
    assert seen > 20
    assert NC.layer_route(1, 64, 32, 16, False)['dx'] == 'split3' and NC.layer_route(1, 64, 32, 16, False)['half']


def test_generator_channels_argument():
    from stylegan_directions_face_reenactment_amd.model import Generator
    ref = Generator(32, 64, 2, channel_multiplier=1)
    same = Generator(32, 64, 2, channel_multiplier=1, channels=None)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in same.state_dict().items()}
    G = Generator(32, 64, 2, channels={4: 48, 8: 32, 16: 16, 32: 8, 64: 999})
    assert list(G.state_dict()) == list(ref.state_dict())                      # the key set and its order do not change
    assert G.channels == {4: 48, 8: 32, 16: 16, 32: 8} and G.n_latent == 8 and G.num_layers == 7
    assert tuple(G.input.input.shape) == (1, 48, 4, 4) and tuple(G.convs[0].conv.weight.shape) == (1, 32, 48, 3, 3)
    assert tuple(G.convs[5].conv.weight.shape) == (1, 8, 8, 3, 3) and tuple(G.to_rgbs[2].conv.weight.shape) == (1, 3, 8, 1, 1)
    for bad, err in (({4: 8, 8: 8, 32: 8}, ValueError), ({4: 8, 8: 8, 16: 0, 32: 8}, ValueError), ({4: 8, 8: 8, 16: 8.0, 32: 8}, ValueError),
                     ({4: 8, 8: True, 16: 8, 32: 8}, ValueError), ([8, 8, 8, 8], TypeError), ({4: 8, 8: 8, 16: -16, 32: 8}, ValueError)):
        with pytest.raises(err):
            Generator(32, 64, 2, channels=bad)
    with pytest.raises(TypeError):
        Generator(32, 64, 2, 1, [1, 3, 3, 1], 0.01, {4: 8, 8: 8, 16: 8, 32: 8})          # keyword only
    for name, spec in NC.NARROW.items():
        Gn = NC.narrow_generator(name)
        lay = NC.generator_layers(spec['size'], spec['channels'])
        mods = [Gn.conv1] + list(Gn.convs)
        assert len(lay) == len(mods) == Gn.num_layers and Gn.n_latent == {'N256': 14, 'N1024': 18}[name]
        for (_, cin, cout, _, up), m in zip(lay, mods):
            assert (m.conv.in_channel, m.conv.out_channel, m.conv.upsample) == (cin, cout, up)
        assert set(NC.narrow_state(name)) == set(O.template_state(spec['size'], NC.STYLE_DIM, NC.N_MLP, 1))


def _blur(t, dtype=torch.float64):
    fir = O.make_fir([1, 3, 3, 1], gain=4.0, dtype=dtype)
    C = t.shape[1]
    return TF.conv2d(t, fir.flip(0, 1)[None, None].repeat(C, 1, 1, 1), padding=1, groups=C)


@pytest.mark.parametrize('prefix,cin,cout,up,h', [('convs.9', 32, 32, False, 11), ('convs.10', 32, 16, True, 9)])
def test_oracle_on_a_narrow_state_is_torchs_fp64_convolution(prefix, cin, cout, up, h):
    """O.styled_conv reads every shape from the state: on N256's 32 -> 32 and 32 -> 16 (up) layers it equals the shared-weight form
    d * conv(x s, W / sqrt(9 Cin)) (+ blur) + noise + bias, leaky ReLU, written with torch.nn.functional in fp64."""
    P = O.cast_state(NC.narrow_state('N256'), torch.float64)
    w = P[prefix + '.conv.weight']
    assert tuple(w.shape) == (1, cout, cin, 3, 3)
    B = 2
    x = S.counter_tensor(7, 'nr.x' + prefix, (B, cin, h, h)).double()
    style = S.counter_tensor(7, 'nr.s' + prefix, (B, NC.STYLE_DIM)).double()
    r = 2 * h if up else h
    nz = S.counter_tensor(7, 'nr.n' + prefix, (1, 1, r, r)).double()
    got = O.styled_conv(P, prefix, x, style, nz, upsample=up)
    s = TF.linear(style, P[prefix + '.conv.modulation.weight'] / NC.STYLE_DIM ** 0.5, P[prefix + '.conv.modulation.bias'])
    wc = w[0] / (9 * cin) ** 0.5
    d = torch.rsqrt(torch.einsum('bi,oi->bo', s * s, (wc * wc).sum((2, 3))) + 1e-8)
    xs = x * s[:, :, None, None]
    if up:
        y = _blur(TF.conv_transpose2d(xs, wc.transpose(0, 1).contiguous(), stride=2))
    else:
        y = TF.conv2d(xs, wc, padding=1)
    y = y * d[:, :, None, None] + P[prefix + '.noise.weight'] * nz + P[prefix + '.activate.bias'][None, :, None, None]
    want = torch.where(y > 0, y, 0.2 * y) * 2 ** 0.5
    assert got.shape == (B, cout, r, r)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_oracle_runs_the_narrow_generator_from_its_state():
    """generator_forward on N256's state: 14 latent rows, 13 layers, the image at 256^2; the last layer is the 16-channel one."""
    P = O.cast_state(NC.narrow_state('N256'), torch.float64)
    w = S.synthetic_latents(7, 1, n_latent=14, key='nr.w').double()
    img, _, layers = O.generator_forward(P, [w], input_is_latent=True, return_layers=True)
    assert img.shape == (1, 3, 256, 256) and bool(torch.isfinite(img).all())
    assert layers['convs.11'].shape == (1, 16, 256, 256) and layers['convs.9'].shape == (1, 32, 128, 128) and layers['conv1'].shape == (1, 64, 4, 4)

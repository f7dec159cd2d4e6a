"""The narrow layers of the 512^2 and 1024^2 generators (32 and 16 channels) at test size: the case lists, two narrow generators and
the route function, shared by tests/test_cpu_narrow_routes.py (which checks and prints the route table) and
tests/test_gpu_narrow_layers.py (which compares the gradients of every case with fp64 autograd of the oracle and asserts that the
launches that ran are the ones the table names).

A route is what the dispatchers of functional.modconv3x3 / autograd._conv_input_grad / functional.wgrad / autograd.SynthesisFn decide
for one StyledConv from its shape alone.  layer_route asks the library's host queries through the dispatchers' own predicates
(functional.split_ok, wino_ok, rgb_fusable, sgdfr_modconv2d_split_plan_info, sgdfr_modconv_wgrad_ksplit); the one predicate that is
an inline expression of the dispatcher (`cin % 64 == 0` in autograd._conv_input_grad) is restated here once, in dx_route -- the GPU
module reads the launches that really ran, so a restatement that drifts from the dispatcher fails there."""
from util import O, S, SEED  # noqa: F401  (puts the repository root on sys.path)

STYLE_DIM, N_MLP = 512, 8

# ------------------------------------------------------------------ per-layer cases (cin, cout, h of the INPUT, up, B)

PER_LAYER_CASES = [
    (32, 32, 8, False, 1), (32, 32, 8, False, 3),           # 8 images per 512-pixel tile (B = 1, 3: one ragged tile)
    (32, 32, 16, False, 1), (32, 32, 16, False, 3),         # 2 images per tile
    (32, 32, 64, False, 1), (32, 32, 64, False, 3),         # whole rows
    (32, 32, 128, False, 1), (32, 32, 128, False, 3),       # 64-wide patches: the geometry of the real 512^2 and 1024^2 layers
    (64, 32, 32, True, 1), (64, 32, 32, True, 3),           # up 64->32: half cout tile forward, exact DOWN3 backward
    (64, 32, 64, True, 1), (64, 32, 64, True, 3),
    (64, 32, 128, True, 3),                                 # added from the route table: 196 tiles, so no K slices, as in the real layers
    (32, 16, 64, True, 1),                                  # no split plan at all: the direct kernels
    (16, 16, 128, False, 1),                                # ... with W > 64
    (96, 96, 16, False, 1),                                 # a half tile behind a full one; 96 % 64 != 0 keeps dL/dx off the split kernels
    (64, 32, 16, False, 1),                                 # cin % 64 == 0: dL/dx (a 32 -> 64 conv) does run on the split kernels
]


def case_id(c):
    return '%s%dto%d-%d-B%d' % ('up' if c[3] else 'plain', c[0], c[1], c[2], c[4])


# ------------------------------------------------------------------ generators

def reference_channels(cm):
    """The reference's table (libs/gan/StyleGAN2/model.py:389-399)."""
    return {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * cm, 128: 128 * cm, 256: 64 * cm, 512: 32 * cm, 1024: 16 * cm}


REAL_GENERATORS = [(size, cm) for size in (256, 512, 1024) for cm in (1, 2)]

NARROW = {
    # the narrow routes, with patch geometry at 128^2 and 256^2
    'N256': dict(size=256, channels={4: 64, 8: 64, 16: 64, 32: 64, 64: 64, 128: 32, 256: 16}, B=2),
    # the index maps of 17 layers and 9 ToRGBs
    'N1024': dict(size=1024, channels={2 ** i: 16 for i in range(2, 11)}, B=1),
}


def generator_layers(size, channels):
    """[(name, cin, cout, h of the input, up)] of the StyledConvs in execution order."""
    out = [('conv1', channels[4], channels[4], 4, False)]
    cin, r, j = channels[4], 8, 0
    while r <= size:
        cout = channels[r]
        out.append(('convs.%d' % (2 * j), cin, cout, r // 2, True))
        out.append(('convs.%d' % (2 * j + 1), cout, cout, r, False))
        cin, r, j = cout, r * 2, j + 1
    return out


def narrow_generator(name):
    """The narrow generator `name` on the CPU, in eval mode, with its synthetic state loaded (narrow_state)."""
    from stylegan_directions_face_reenactment_amd.model import Generator
    spec = NARROW[name]
    G = Generator(spec['size'], STYLE_DIM, N_MLP, channel_multiplier=1, channels=spec['channels'])
    G.load_state_dict(narrow_state(name, G), strict=True)
    return G.eval()


_STATES = {}


def narrow_state(name, G=None):
    """synthetic_state_dict over the module's own state_dict() shapes (the oracle reads every shape from the state); cached."""
    if name not in _STATES:
        if G is None:
            from stylegan_directions_face_reenactment_amd.model import Generator
            spec = NARROW[name]
            G = Generator(spec['size'], STYLE_DIM, N_MLP, channel_multiplier=1, channels=spec['channels'])
        _STATES[name] = S.synthetic_state_dict(G.state_dict(), seed=SEED)
    return _STATES[name]


# ------------------------------------------------------------------ routes

def _lib():
    from stylegan_directions_face_reenactment_amd import _native
    return _native.load()


def dx_route(F_, B, cin, cout, h, up):
    """autograd._conv_input_grad's choice for dL/d(x s) of a layer cin -> cout on an h x h input, under the ambient Config."""
    from stylegan_directions_face_reenactment_amd import _native as N
    if up:
        split_down = F_.config().precision != 'fp32' and F_.split_ok(B, cout, cin, h, h, N.MODE_DOWN3)
        return 'split down3' if split_down else 'down3'
    if cin % 64 == 0 and F_.split_ok(B, cout, cin, h, h):         # (the guard: the dispatcher's inline expression, restated)
        return 'split3'
    if F_.wino_ok(B, cout, cin, h, h):
        return 'wino3'
    return 'plain3'


GEOMETRY = ('images', 'rows', 'patch', 'flat')


def layer_route(B, cin, cout, h, up, precision='fp16x3'):
    """dict(kind, fwd, plan, geometry, half, ksplit, dx, wgrad, wgrad_k, rgb) of one StyledConv on an h x h input:
    fwd 'split' | 'wino' | 'direct' (modconv3x3's order); for 'split' the plan's cfg number, its geometry class, the half cout tile and
    the K slices (plan_info's word and ksplit_hint); dx: dx_route; wgrad 'sliced' (sgdfr_modconv_wgrad_ksplit > 0) | 'direct';
    rgb (plain layers): SynthesisFn's with-grad forward fuses the ToRGB that reads the layer."""
    from stylegan_directions_face_reenactment_amd import functional as F_, _native as N
    lib = _lib()
    mode = N.MODE_UP3 if up else N.MODE_PLAIN3
    r = dict(kind='up' if up else 'plain', B=B, cin=cin, cout=cout, h=h, precision=precision, plan=None, geometry=None, half=False,
             ksplit=1, rgb=False)
    with F_.precision(precision):
        if F_.split_ok(B, cin, cout, h, h, mode):
            word = lib.sgdfr_modconv2d_split_plan_info(B, cin, cout, h, h, mode, 0)
            assert word >= 0
            simgs = (word >> 8) & 0xfff
            r.update(fwd='split', plan=word & 15, half=bool((word >> 20) & 1),
                     geometry='flat' if up else ('patch' if h > 64 else ('rows' if simgs == 1 else 'images')))
            if F_.config().use_splitk:
                r['ksplit'] = lib.sgdfr_modconv2d_split_ksplit_hint(B, cin, cout, h, h, mode)
        elif not up and F_.wino_ok(B, cin, cout, h, h):
            r['fwd'] = 'wino'
        else:
            r['fwd'] = 'direct'
        r['dx'] = dx_route(F_, B, cin, cout, h, up)
        r['wgrad_k'] = lib.sgdfr_modconv_wgrad_ksplit(B, cin, cout, h, h, mode)
        r['wgrad'] = 'sliced' if r['wgrad_k'] > 0 else 'direct'
        if not up:
            r['rgb'] = bool(F_.config().precision != 'fp32' and F_.rgb_fusable(B, cin, cout, h, h))
    return r


def route_class(r):
    """What a small case has to share with a real layer to stand for it: the kind of layer, the forward kernel family with its plan,
    geometry class and half tile, the dL/dx route, the form of the weight gradient, and whether ToRGB fuses.  (The K slices of the
    forward are not part of it: they follow the tile COUNT, which N256 at B = 2 does not have -- its up 64 -> 32 layer runs K/2, the real
    ones unsliced.  The per-layer cases do reach the unsliced launch; tests/test_cpu_narrow_routes.py asks that of them.)"""
    fwd = r['fwd'] if r['fwd'] != 'split' else 'split cfg%d %s%s' % (r['plan'], r['geometry'], ' half' if r['half'] else '')
    return (r['kind'], fwd, r['dx'], r['wgrad'], 'rgb fused' if r['rgb'] else ('rgb apart' if r['kind'] == 'plain' else '-'))


def is_narrow(cin, cout):
    return cin < 64 or cout < 64


def format_route(name, r):
    fwd = route_class(r)[1] + (' K/%d' % r['ksplit'] if r['ksplit'] > 1 else '')
    return '%-22s B%d %3d->%-3d @%-4d %-5s | %-28s | %-11s | %-9s | %s' % (
        name, r['B'], r['cin'], r['cout'], r['h'], r['kind'], fwd, r['dx'], r['wgrad'] + ('(%d)' % r['wgrad_k'] if r['wgrad_k'] else ''),
        route_class(r)[4])


def launches_of(descs):
    """(forward family, dL/dx route) from the descriptions functional attaches to its conv launches (timing.LaunchTimer.conv) of one
    StyledConv forward + backward."""
    fwd = dx = None
    for d in descs:
        if d.startswith('bwd '):
            assert dx is None, descs
            dx = next(k for k in ('split down3', 'split3', 'wino3', 'plain3', 'down3') if d.startswith('bwd ' + k + ' '))
        else:
            assert fwd is None, descs
            fwd = 'split' if d.startswith('split mode') else 'wino' if d.startswith('wino3 ') else 'direct'
            assert fwd != 'direct' or d.startswith('plain3 ') or d.startswith('up3 '), d
    return fwd, dx

"""GPU: the e4e encoder on the HIP kernels with more heads than its input side gives (encoder.encode / run_debug of
Encoder4Editing(50, 'ir_se', 512 / 1024, input_size=...)) against the fp64 restatement on the CPU (tests/e4e_restatement.py, pinned
by test_cpu_e4e_styles to the fixture written from the reference's own module) and against the fixture kat24.  Never against another
run of the HIP code, except where two HIP runs must agree.

Bar: every tap and W+ within 8 x the reference's own max |fp32 - fp64| on that tensor (dev_* of the fixture), the bar of
test_gpu_e4e_hip.  Every test prints the figures it asserts on.
"""
import copy

import pytest
import torch

from util import S, golden
import e4e_restatement as R
import e4e_styles_cases as C

pytestmark = pytest.mark.gpu

BAR = 8.0


@pytest.fixture(scope='module')
def kat():
    return golden(C.KAT)


@pytest.fixture(scope='module')
def encoders():
    """Cases d and e: the module on the device, its state, the images and the fp64 taps of the restatement on the CPU."""
    out = {}
    for name in ('d', 'e'):
        enc, state = C.make_encoder(S, name)
        x = C.fixture_inputs(S, name)
        with torch.no_grad():
            taps64 = R.forward(state, x.double())
        out[name] = (copy.deepcopy(enc).cuda(), state, x, taps64)
    return out


def _ratio(got, want, dev):
    return float((got.double().cpu() - want).abs().max()) / dev


@pytest.mark.parametrize('name', ['d', 'e'])
def test_taps_and_codes_against_the_fp64_restatement(kat, encoders, name):
    """d: input 32, 18 heads, 11 of them on p1: 88 R^2 floats per row of parked head maps, head convs on 1x1 inputs.  e: input 80,
    16 heads: 5 / 10 / 20 maps, 72 R^2, pixel counts that are no multiple of the 64-pixel tile."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _, x, taps64 = encoders[name]
    r = E.run_debug(enc, x.cuda())
    torch.cuda.synchronize()
    got = dict(r['debug'], w=r['w'])
    assert list(got) == list(R.TAPS)
    figures = []
    for k in R.TAPS:
        dev = float(kat['dev_%s_%s' % (k, name)])
        assert tuple(got[k].shape) == tuple(taps64[k].shape), k
        ratio = _ratio(got[k], taps64[k], dev)
        figures.append((k, ratio))
        print('case %s tap %-8s %-18s max |HIP - fp64| = %.2f x the reference fp32 deviation %.3e   bar %.0f x' % (
            name, k, tuple(got[k].shape), ratio, dev, BAR))
    e_fix = _ratio(r['w'], torch.from_numpy(kat['w_' + name]), float(kat['dev_w_' + name]))
    print('case %s W+ against the fixture: %.2f x' % (name, e_fix))
    first = next(((k, v) for k, v in figures + [('w (fixture)', e_fix)] if not v <= BAR), None)
    assert first is None, 'first tensor beyond the bar: %s at %.2f x' % first
    assert tuple(r['w'].shape) == (C.CASES[name][0], C.heads(name), 512)
    assert torch.equal(E.encode(enc, x.cuda()), r['w'])                   # the debug taps change nothing


@pytest.mark.parametrize('name', ['d', 'e'])
def test_two_runs_are_bitwise_equal(encoders, name):
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _, x, _ = encoders[name]
    xc = x.cuda()
    one, two = E.run_debug(enc, xc), E.run_debug(enc, xc)
    assert torch.equal(one['w'], two['w'])
    assert all(torch.equal(one['debug'][k], two['debug'][k]) for k in one['debug'])


def test_rows_are_independent_across_batch_sizes(kat, encoders):
    """B = 1 and 2 from the rows of case d, permuted: each row stays within the bar against fp64."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _, x, taps64 = encoders['d']
    dev = float(kat['dev_w_d'])
    for rows in ([1], [0], [1, 0]):
        ratio = _ratio(E.encode(enc, x[rows].cuda()), taps64['w'][rows], dev)
        print('B = %d rows %s: W+ at %.2f x the reference fp32 deviation   bar %.0f x' % (len(rows), rows, ratio, BAR))
        assert ratio <= BAR


def test_codes_of_18_heads_on_the_256_crop_against_the_reference_fixture(kat):
    """Case f: the 1024 generator's encoder on a 256 x 256 input against the reference's fp64 codes; no CPU recomputation at this
    size.  The module's own planned forward (MIOpen) on the device meets the same bar."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _ = C.make_encoder(S, 'f')
    enc = copy.deepcopy(enc).cuda()
    want = torch.from_numpy(kat['w_f'])
    xc = C.fixture_inputs(S, 'f').cuda()
    dev = float(kat['dev_w_f'])
    w = E.encode(enc, xc)
    with torch.no_grad():
        stock = enc(xc)
    ratio, ratio_stock = _ratio(w, want, dev), _ratio(stock, want, dev)
    print('case f W+ %s max |HIP - reference| = %.2f x, max |planned forward - reference| = %.2f x the reference fp32 deviation %.3e   '
          'bar %.0f x' % (tuple(w.shape), ratio, ratio_stock, dev, BAR))
    assert tuple(w.shape) == tuple(stock.shape) == (1, 18, 512) and not w.requires_grad
    assert ratio <= BAR and ratio_stock <= BAR


def test_invert_images_with_16_latents():
    """reenact.invert_images with the 16 heads of case e's encoder: refused by the 256 generator (14 latents), rendered by the 512
    generator (16), the codes encode's bit for bit."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    from stylegan_directions_face_reenactment_amd.reenact import invert_images
    from util import hip_generator
    enc, _ = C.make_encoder(S, 'e')                              # 16 heads: the 512 generator's count
    enc = copy.deepcopy(enc).cuda()
    xc = C.fixture_inputs(S, 'e')[:1].cuda()
    with pytest.raises(RuntimeError, match='gives 16 latents, the generator takes 14'):
        invert_images(enc, hip_generator(256, 1), xc)
    G = hip_generator(512, 1)
    assert G.n_latent == 16
    w, frames = invert_images(enc, G, xc)
    assert torch.equal(w, E.encode(enc, xc)) and tuple(frames.shape) == (1, 3, 512, 512) and bool(torch.isfinite(frames).all())

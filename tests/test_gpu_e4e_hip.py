"""GPU: the e4e encoder on the HIP kernels of csrc/e4e.hip (encoder.encode / run_debug, reenact.invert_images) against the fp64
restatement on the CPU (tests/e4e_restatement.py, itself pinned by test_cpu_e4e_taps to the fixture written from the reference's own
module) and against the fixtures kat15 and kat6.  Never against another run of the HIP code, except where two HIP runs must agree.

Bar: every tap and W+ within 8 x the reference's own max |fp32 - fp64| on that tensor (dev_* of the fixture): the same fp32
accumulation in another order.  Every test prints the figures it asserts on.
"""
import copy

import pytest
import torch

from util import O, S, SEED, golden, hip_generator
from oracle import e4e_oracle as EO
import e4e_restatement as R
from test_cpu_e4e_taps import make_encoder

pytestmark = pytest.mark.gpu

BAR = 8.0


@pytest.fixture(scope='module')
def kat():
    return golden(R.KAT)


@pytest.fixture(scope='module')
def encoders():
    """Cases a and b: the module on the device, its state, the images and the fp64 taps of the restatement on the CPU."""
    out = {}
    for name in ('a', 'b'):
        enc, state = make_encoder(name)
        x = R.fixture_inputs(S, name)
        with torch.no_grad():
            taps64 = R.forward(state, x.double())
        out[name] = (copy.deepcopy(enc).cuda(), state, x, taps64)       # .cuda() after a CPU load
    return out


def _ratio(got, want, dev):
    return float((got.double().cpu() - want).abs().max()) / dev


@pytest.mark.parametrize('name', ['a', 'b'])
def test_taps_and_codes_against_the_fp64_restatement(kat, encoders, name):
    """a: R = 64, 10 heads, head convs on 1x1 inputs (the centre tap alone).  b: R = 96: 6x6, 12x12 and 24x24 taps, 3x3 maps in the
    stride-2 convs, pixel counts that are no multiple of the 64-pixel tile, 6 -> 12 and 12 -> 24 bilinear resamples."""
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
    assert torch.equal(E.encode(enc, x.cuda()), r['w'])                   # the debug taps change nothing


def test_codes_at_256_against_the_reference_fixture(kat):
    """Case c: B = 2 at R = 256 against kat6's w256 (the reference's fp32 codes), 14 heads; no CPU recomputation at this size."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _ = make_encoder('c')
    enc = enc.cuda()
    want = torch.from_numpy(golden('kat6_e4e.npz')['w256']).double()
    w = E.encode(enc, R.fixture_inputs(S, 'c').cuda())
    dev = float(kat['dev_w_c'])
    ratio = _ratio(w, want, dev)
    print('case c W+ %s max |HIP - reference| = %.2f x the reference fp32 deviation %.3e   bar %.0f x' % (tuple(w.shape), ratio, dev, BAR))
    assert tuple(w.shape) == (2, 14, 512) and ratio <= BAR


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return sum('e4e_conv_kernel' in n for n in names), sum('e4e_finish_kernel' in n for n in names)


def test_rows_are_independent_across_batch_sizes_and_plans(kat, encoders):
    """B = 1, 2 and 3 from the rows of case a, permuted: each row stays within the bar against fp64.  The split-K plan follows the
    row count: unit 0's first conv has 64 output tiles per row and runs whole from 192 tiles on, so B = 3 slices one conv fewer."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _, x, taps64 = encoders['a']
    dev = float(kat['dev_w_a'])
    counts = {}
    for rows in ([2], [1, 0], [1, 2, 0]):
        B = len(rows)
        xb = x[rows].cuda()
        ratio = _ratio(E.encode(enc, xb), taps64['w'][rows], dev)
        counts[B] = _launches(lambda: E.encode(enc, xb))
        print('B = %d rows %s: W+ at %.2f x the reference fp32 deviation   bar %.0f x; %d convs, %d of them sliced over K' % (
            B, rows, ratio, BAR, counts[B][0], counts[B][1]))
        assert ratio <= BAR
    # stem, 24 x (conv1, conv2), 3 shortcut convs, 2 lateral convs, 4 + 5 + 6 head depths, the EqualLinears
    assert all(c[0] == 1 + 48 + 3 + 2 + 15 + 1 for c in counts.values()), counts
    assert counts[1][1] >= counts[2][1] >= counts[3][1] > 0 and counts[1][1] > counts[3][1], counts


def test_two_runs_are_bitwise_equal(encoders):
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _, x, _ = encoders['b']
    xc = x.cuda()
    one, two = E.run_debug(enc, xc), E.run_debug(enc, xc)
    assert torch.equal(one['w'], two['w'])
    assert all(torch.equal(one['debug'][k], two['debug'][k]) for k in one['debug'])


def test_graph_capture_replays_the_eager_result(encoders):
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, _, x, _ = encoders['a']
    xc = x.cuda()
    eager = E.encode(enc, xc)                   # the pack exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.encode(enc, xc)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and float(eager.abs().max()) > 0.1


def test_pack_follows_the_weights(kat, encoders):
    """styles[0].linear.bias += 1 in place rebuilds the pack and moves every row of W+ by 1; a state loaded on the device does too."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, state, x, taps64 = encoders['a']
    e = copy.deepcopy(enc)
    assert e._pack is None
    xc = x.cuda()
    base = E.encode(e, xc)
    p0 = E.packed(e)
    E.encode(e, xc)
    assert E.packed(e) is p0                                  # no change, no rebuild
    with torch.no_grad():
        e.styles[0].linear.bias.add_(1.0)                     # bumps the version counter
    moved = E.encode(e, xc)
    assert E.packed(e) is not p0
    dev = float(kat['dev_w_a'])
    shift = float(((moved.double() - base.double()) - 1.0).abs().max())
    ratio = _ratio(moved, taps64['w'] + 1.0, dev)
    print('W+ moved by 1 +- %.3e (%.2f x dev_w); against fp64 + 1: %.2f x   bar %.0f x' % (shift, shift / dev, ratio, BAR))
    assert shift <= BAR * dev and ratio <= BAR
    e.load_state_dict(state, strict=True)                     # back to the fixture's weights, loaded onto the device module
    assert e._pack is None
    assert torch.equal(E.encode(e, xc), base)


def test_hip_path_agrees_with_the_miopen_forward(encoders):
    from stylegan_directions_face_reenactment_amd import encoder as E
    for name in ('a', 'b'):
        enc, _, x, _ = encoders[name]
        with torch.no_grad():
            stock = enc(x.cuda())
        w = E.encode(enc, x.cuda())
        top = float(stock.abs().max())
        err = float((w - stock).abs().max())
        print('case %s: max |encode - enc(x)| %.3e   bar 1e-3 max|w| = %.3e' % (name, err, 1e-3 * top))
        assert not w.requires_grad and err <= 1e-3 * top


def test_invert_images_end_to_end(encoders):
    """reenact.invert_images at R = 64 (10 latents, the 64 x 64 generator): the codes are encode's bit for bit, the frames within
    1e-3 of the CPU oracle's generator on the CPU oracle's encoder codes."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    from stylegan_directions_face_reenactment_amd.reenact import images_to_uint8, invert_images
    enc, state, x, _ = encoders['a']
    G = hip_generator(64, 1)
    trunc = S.counter_tensor(7, 'e4e.invert.t', (1, 512))
    xc = x.cuda()
    w, frames = invert_images(enc, G, xc, truncation=0.7, trunc=trunc.cuda())
    assert torch.equal(w, E.encode(enc, xc)) and tuple(frames.shape) == (3, 3, 64, 64)
    PG = {k: v.cpu() for k, v in G.state_dict().items()}
    with torch.no_grad():
        w_cpu = EO.encoder_forward(state, x)
        ref = O.generate_image(PG, w_cpu, 0.7, trunc, input_is_latent=True)
    err = float((frames.cpu().double() - ref.double()).abs().max())
    print('inverted frames: max |HIP - oracle| %.3e   bar 1e-3' % err)
    assert err <= 1e-3
    _, u8 = invert_images(enc, G, xc, truncation=0.7, trunc=trunc.cuda(), as_uint8=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (3, 64, 64, 3)
    # a second generator call may pick another verified arithmetic: the same frame up to one grey level at a rounding edge
    assert int((u8.int() - images_to_uint8(frames).int()).abs().max()) <= 1
    with pytest.raises(RuntimeError, match='truncation latent'):
        invert_images(enc, G, xc, truncation=0.7)

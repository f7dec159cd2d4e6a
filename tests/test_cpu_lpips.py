"""CPU: LPIPS-alex -- the fp64 restatement of the tests (lpips_restatement.py) against the reference's own LPIPS code
(tests/golden/kat9_lpips.npz, scripts/make_golden_lpips.py), and the host contract of lpips.LPIPS: state-dict formats, rejected
network types, frozen weights, pickling, the C ABI."""
import copy
import pickle

import numpy as np
import pytest
import torch

from util import S, golden, t
import lpips_restatement as R


def _kat():
    return golden('kat9_lpips.npz')


def test_restatement_matches_the_reference_lpips():
    g = _kat()
    sd = S.synthetic_lpips_state(int(g['seed']))
    for name in ('a', 'b'):
        x, y = t(g['x_' + name]), t(g['y_' + name])
        xr = x.double().requires_grad_(True)
        loss = R.lpips(sd, xr, y)
        loss.backward()
        ref = float(g['loss_' + name])
        assert abs(loss.item() - ref) <= 1e-12 * abs(ref), (loss.item(), ref)
        dref = t(g['dx_' + name])
        assert float((xr.grad - dref).abs().max() / dref.abs().max()) <= 1e-10


def test_restatement_with_its_own_masks_is_the_plain_restatement():
    """taps(fixed=own activations) gives the same loss and gradient as plain ReLU / max-pool: the mask injection the GPU tests
    use to pin the fp64 gradient to the HIP forward's choices changes nothing when the choices agree."""
    g = _kat()
    sd = S.synthetic_lpips_state(int(g['seed']))
    x, y = t(g['x_b']), t(g['y_b'])
    own = [a.detach() for a in R.taps(sd, x)]
    x1, x2 = x.double().requires_grad_(True), x.double().requires_grad_(True)
    l1, l2 = R.lpips(sd, x1, y), R.lpips(sd, x2, y, fixed=own)
    l1.backward()
    l2.backward()
    assert abs(float(l1) - float(l2)) <= 1e-14
    assert torch.allclose(x1.grad, x2.grad, rtol=0, atol=1e-15)


def _module():
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    return LPIPS()


def test_state_dict_keys_match_the_reference():
    m = _module()
    keys = list(m.state_dict().keys())
    want = ['net.mean', 'net.std'] + ['net.layers.%d.%s' % (i, p) for i in (0, 3, 6, 8, 10) for p in ('weight', 'bias')] + \
        ['lin.%d.1.weight' % i for i in range(5)]
    assert keys == want
    assert all(not p.requires_grad for p in m.parameters())
    assert tuple(m.net.layers[0].weight.shape) == (64, 3, 11, 11) and tuple(m.lin[2][1].weight.shape) == (1, 384, 1, 1)


def test_state_dict_round_trips_in_all_three_formats():
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    sd = S.synthetic_lpips_state(5)
    m = LPIPS()
    m.load_state_dict(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # torchvision alexnet (features.N.*, classifier.* ignored) + PerceptualSimilarity alex.pth (linN.model.1.weight)
    tv = {k.replace('net.layers.', 'features.'): v for k, v in sd.items() if k.startswith('net.layers.')}
    tv['classifier.1.weight'] = torch.zeros(4096, 9216)
    ps = {'lin%d.model.1.weight' % i: sd['lin.%d.1.weight' % i] for i in range(5)}
    m2 = LPIPS()
    m2.load_state_dict(tv)
    m2.load_state_dict(ps)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    m3 = LPIPS()
    m3.load_state_dict({**tv, **ps})
    assert all(torch.equal(v, sd[k]) for k, v in m3.state_dict().items())
    # the renamed alex.pth of lpips/utils.py:get_state_dict ('0.1.weight' ...)
    m4 = LPIPS()
    m4.load_state_dict({'%d.1.weight' % i: sd['lin.%d.1.weight' % i] for i in range(5)})
    assert all(torch.equal(m4.lin[i][1].weight, sd['lin.%d.1.weight' % i]) for i in range(5))
    with pytest.raises(RuntimeError):
        LPIPS().load_state_dict({k: v for k, v in ps.items() if not k.startswith('lin4')})


def test_rejected_network_types_and_versions():
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    for net in ('squeeze', 'vgg', 'resnet'):
        with pytest.raises(NotImplementedError):
            LPIPS(net_type=net)
    with pytest.raises(NotImplementedError):
        LPIPS(version='0.0')


def test_trainable_weights_are_refused_before_any_launch():
    m = _module()
    m.lin[0][1].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='requires_grad'):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))


def test_module_deepcopies_and_pickles():
    m = _module()
    m.load_state_dict(S.synthetic_lpips_state(2))
    m2 = pickle.loads(pickle.dumps(m))
    m3 = copy.deepcopy(m)
    for a, b, c in zip(m.state_dict().values(), m2.state_dict().values(), m3.state_dict().values()):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not any(isinstance(v, type(np)) for v in vars(m).values())


def test_native_symbols_and_error_paths():
    from stylegan_directions_face_reenactment_amd import _native
    for name in ('sgdfr_lpips_prepack_f32', 'sgdfr_lpips_features_f32', 'sgdfr_lpips_distance_f32', 'sgdfr_lpips_backward_f32'):
        assert name in _native.SIGNATURES
    assert _native.ABI_VERSION == 23
    lib = _native.load()
    assert lib.sgdfr_lpips_pack_elems() >= 2 * 2469696            # forward + input-gradient weights
    assert lib.sgdfr_lpips_feature_elems(1, 256, 256) == 64 * 63 * 63 + 192 * 31 * 31 + (384 + 256 + 256) * 15 * 15
    assert lib.sgdfr_lpips_workspace_bytes(1, 30, 256) < 0        # too small for the network
    assert lib.sgdfr_lpips_feature_elems(1, 256, 30) < 0
    rc = lib.sgdfr_lpips_features_f32(None, 1, None, 0, 30, 30, None, None, None, 0, None)
    assert rc != 0 and b'unsupported image size' in lib.sgdfr_last_error()
    rc = lib.sgdfr_lpips_distance_f32(None, 1, None, 1, 0, 0, 1, 64, 64, None, None, None, 0, None)
    assert rc != 0 and b'null' in lib.sgdfr_last_error()
    one = ctypes_ptr(1)
    rc = lib.sgdfr_lpips_backward_f32(one, one, 1, one, 1, 1, 0, 1, 64, 64, one, one, one, 1 << 30, None)
    assert rc != 0 and b'outside' in lib.sgdfr_last_error()
    rc = lib.sgdfr_lpips_distance_f32(one, 1, one, 1, 0, 0, 1, 64, 64, one, one, one, 16, None)
    assert rc != 0 and b'workspace' in lib.sgdfr_last_error()


def ctypes_ptr(v):
    import ctypes
    return ctypes.c_void_p(v)


def test_pti_loss_is_opt_in():
    from stylegan_directions_face_reenactment_amd import finetune
    import inspect
    assert inspect.signature(finetune.optimize_g).parameters['loss_fn'].default is None
    assert hasattr(finetune, 'PtiLoss')

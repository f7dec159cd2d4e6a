"""CPU: the ArcFace identity loss -- the fp64 restatement of the tests (idloss_restatement.py) against the reference's own IDLoss
(tests/golden/kat10_idloss.npz, scripts/make_golden_idloss.py), and the host contract of id_loss.IDLoss: the reference's keys and
checkpoint formats, the BatchNorm folding, refused configurations, pickling, the C ABI and the opt-in compat mount."""
import copy
import ctypes
import pickle
import sys

import pytest
import torch
import torch.nn.functional as F

from util import S, golden, t
import idloss_restatement as R

CASES = {'crop': ((1, 3, 256, 256), True), 'nocrop': ((2, 3, 120, 112), False)}


def _kat():
    return golden('kat10_idloss.npz')


def _inputs(g, name):
    seed, (shape, _) = int(g['seed']), CASES[name]
    x = S.counter_tensor(seed, str(g['x_key_' + name]), shape, 0.0, 0.5).clamp(-1, 1)
    y = S.counter_tensor(seed, str(g['y_key_' + name]), shape, 0.0, 0.5).clamp(-1, 1)
    return x, y


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_restatement_matches_the_reference_id_loss():
    g = _kat()
    sd = S.synthetic_arcface_state(int(g['seed']))
    for name, (_, crop) in CASES.items():
        x, y = _inputs(g, name)
        xr = x.double().requires_grad_(True)
        loss = R.id_loss(sd, xr, y, crop)
        loss.backward()
        ref = float(g['loss_' + name])
        assert 0.05 <= ref <= 1.5
        assert abs(loss.item() - ref) <= 1e-12 * abs(ref), (loss.item(), ref)
        assert _rel(R.backbone(sd, x, crop)['e'], t(g['ex_' + name])) <= 1e-6
        assert _rel(R.backbone(sd, y, crop)['e'], t(g['ey_' + name])) <= 1e-6
        dx = xr.grad[:, :, 35:223, 32:220] if crop else xr.grad
        assert _rel(dx, t(g['dx_' + name])) <= 1e-6


def test_backbone_keys_and_shapes_are_the_reference_s():
    from stylegan_directions_face_reenactment_amd.id_loss import Backbone
    m = Backbone(112, 50, 'ir_se', 0.6)
    got = ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in m.state_dict().items()]
    assert got == [str(k) for k in _kat()['keys']]
    assert all(not p.requires_grad for p in m.parameters())


def test_checkpoint_formats_load_strictly(tmp_path):
    from stylegan_directions_face_reenactment_amd.id_loss import IDLoss
    sd = S.synthetic_arcface_state(3)
    path = str(tmp_path / 'model_ir_se50.pth')
    torch.save(sd, path)
    m = IDLoss(path)                                             # the reference's constructor: torch.load(pretrained_model_path)
    assert not m.facenet.training
    for k, v in m.facenet.state_dict().items():
        assert torch.equal(v, sd[k]), k
    m2 = IDLoss()
    m2.load_state_dict({'facenet.' + k: v for k, v in sd.items()})   # an IDLoss state dict
    assert all(torch.equal(v, sd[k]) for k, v in m2.facenet.state_dict().items())
    m3 = IDLoss()
    m3.load_state_dict(m2.state_dict())
    with pytest.raises(RuntimeError):
        IDLoss().load_state_dict({k: v for k, v in sd.items() if not k.startswith('output_layer.3')})


def test_folded_weights_equal_the_unfolded_math_in_fp64():
    from stylegan_directions_face_reenactment_amd.id_loss import Backbone
    sd = S.synthetic_arcface_state(4)
    m = Backbone()
    m.load_state_dict(sd)
    f = m.folded(torch.float64)
    assert len(f) == 245
    P = {k: v.double() for k, v in sd.items()}

    def bn(a, pre):
        return F.batch_norm(a, P[pre + '.running_mean'], P[pre + '.running_var'], P[pre + '.weight'], P[pre + '.bias'], False, 0.0, 1e-5)

    a = S.counter_tensor(4, 'fold.a', (2, 3, 9, 9)).double()
    assert torch.allclose(F.conv2d(a, f[0], f[1], padding=1), bn(F.conv2d(a, P['input_layer.0.weight'], padding=1), 'input_layer.1'),
                          rtol=0, atol=1e-12)
    u = 3                                                         # a unit with a shortcut conv: 64 -> 128, stride 2
    s1, t1, w1, a1, w2, b2, f1, f2, wsc, bsc = f[3 + 10 * u:3 + 10 * (u + 1)]
    pre = 'body.%d.' % u
    z = S.counter_tensor(4, 'fold.z', (2, 64, 8, 8)).double()
    assert torch.allclose(z * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1), bn(z, pre + 'res_layer.0'), rtol=0, atol=1e-12)
    c = S.counter_tensor(4, 'fold.c', (2, 128, 8, 8)).double()
    assert torch.allclose(F.conv2d(c, w2, b2, stride=2, padding=1),
                          bn(F.conv2d(c, P[pre + 'res_layer.3.weight'], stride=2, padding=1), pre + 'res_layer.4'), rtol=0, atol=1e-12)
    assert torch.allclose(F.conv2d(z, wsc.view(128, 64, 1, 1), bsc, stride=2),
                          bn(F.conv2d(z, P[pre + 'shortcut_layer.0.weight'], stride=2), pre + 'shortcut_layer.1'), rtol=0, atol=1e-12)
    assert f[3 + 10 * 1 + 8] is None and f[3 + 10 * 1 + 9] is None      # identity shortcut
    h = S.counter_tensor(4, 'fold.h', (3, 512, 7, 7)).double()
    v = F.linear(bn(h, 'output_layer.0').flatten(1), P['output_layer.3.weight'], P['output_layer.3.bias'])
    v = F.batch_norm(v, P['output_layer.4.running_mean'], P['output_layer.4.running_var'], P['output_layer.4.weight'],
                     P['output_layer.4.bias'], False, 0.0, 1e-5)
    assert torch.allclose(F.linear(h.flatten(1), f[-2], f[-1]), v, rtol=0, atol=1e-10)


def test_unsupported_configurations_are_refused():
    from stylegan_directions_face_reenactment_amd.id_loss import Backbone
    for kw in ({'num_layers': 100}, {'num_layers': 152}, {'mode': 'ir'}, {'input_size': 224}, {'affine': False}):
        with pytest.raises(NotImplementedError):
            Backbone(**kw)


def test_trainable_or_train_mode_modules_are_refused_before_any_launch():
    from stylegan_directions_face_reenactment_amd.id_loss import IDLoss
    x = torch.zeros(1, 3, 256, 256)                               # a CPU tensor: a launch would fail differently
    m = IDLoss()
    m.facenet.body[0].res_layer[1].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='requires_grad'):
        m(x, x)
    m = IDLoss()
    m.facenet.train()
    with pytest.raises(RuntimeError, match='eval'):
        m(x, x)
    with pytest.raises(RuntimeError, match='eval'):
        m.target(x)


def test_module_deepcopies_and_pickles():
    from stylegan_directions_face_reenactment_amd.id_loss import IDLoss
    m = IDLoss()
    m.load_state_dict(S.synthetic_arcface_state(2))
    for m2 in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert m2.facenet._pack is None
        for a, b in zip(m.state_dict().values(), m2.state_dict().values()):
            assert torch.equal(a, b)


def test_native_symbols_and_error_paths():
    from stylegan_directions_face_reenactment_amd import _native
    for name in ('sgdfr_idloss_prepack_f32', 'sgdfr_idloss_forward_f32', 'sgdfr_idloss_backward_f32'):
        assert name in _native.SIGNATURES
    assert _native.ABI_VERSION == 23 and _native.IDLOSS_PARAMS == 245
    lib = _native.load()
    assert lib.sgdfr_idloss_pack_elems() >= 2 * 43_000_000           # forward + input-gradient weights (349 MB)
    assert lib.sgdfr_idloss_saved_elems(2) == 2 * lib.sgdfr_idloss_saved_elems(1) > 0
    assert lib.sgdfr_idloss_saved_elems(0) < 0
    # the workspace does not depend on the window: 30 rows are fine without the crop (AdaptiveAvgPool2d takes any size) ...
    assert lib.sgdfr_idloss_workspace_bytes(1, 30, 256) == lib.sgdfr_idloss_workspace_bytes(1, 256, 256) > 0
    assert lib.sgdfr_idloss_workspace_bytes(1, 0, 256) < 0 and lib.sgdfr_idloss_workspace_bytes(1, 256, 8193) < 0
    assert lib.sgdfr_idloss_workspace_bytes(0, 256, 256) < 0
    one = ctypes.c_void_p(1)
    # ... while the crop window [35:223] of 30 rows is empty: refused by the forward and the backward, by name
    rc = lib.sgdfr_idloss_forward_f32(one, 1, None, 0, 30, 256, 1, one, one, None, one, 1 << 40, None)
    assert rc != 0 and b'unsupported image size 30x256 (crop=1)' in lib.sgdfr_last_error()
    rc = lib.sgdfr_idloss_backward_f32(one, one, 1, 256, 32, 1, one, one, one, 1 << 40, None)
    assert rc != 0 and b'unsupported image size 256x32 (crop=1)' in lib.sgdfr_last_error()
    rc = lib.sgdfr_idloss_forward_f32(one, 1, None, 0, 30, 256, 0, None, one, None, one, 1 << 40, None)
    assert rc != 0 and b'null' in lib.sgdfr_last_error()              # crop=0: past the size check, stopped by the null pack
    rc = lib.sgdfr_idloss_forward_f32(one, 1, None, 0, 256, 256, 1, None, one, None, one, 1 << 40, None)
    assert rc != 0 and b'null' in lib.sgdfr_last_error()
    rc = lib.sgdfr_idloss_forward_f32(one, 1, one, 2, 256, 256, 1, one, one, None, one, 1 << 40, None)   # rows_y > rows_x
    assert rc != 0 and b'bad inputs' in lib.sgdfr_last_error()
    rc = lib.sgdfr_idloss_forward_f32(one, 1, None, 0, 256, 256, 1, one, one, None, one, 16, None)
    assert rc != 0 and b'workspace' in lib.sgdfr_last_error()
    rc = lib.sgdfr_idloss_backward_f32(one, None, 1, 256, 256, 1, one, one, one, 1 << 40, None)
    assert rc != 0 and b'null' in lib.sgdfr_last_error()
    rc = lib.sgdfr_idloss_backward_f32(one, one, 1, 256, 256, 2, one, one, one, 1 << 40, None)
    assert rc != 0 and b'unsupported' in lib.sgdfr_last_error()
    params = (ctypes.c_void_p * _native.IDLOSS_PARAMS)()
    rc = lib.sgdfr_idloss_prepack_f32(params, one, None)
    assert rc != 0 and b'parameter 0 is null' in lib.sgdfr_last_error()


def test_the_mount_is_opt_in(tmp_path, capsys):
    from stylegan_directions_face_reenactment_amd import compat
    assert compat.ID_LOSS_ALIAS not in compat.ALIASES
    saved = {k: sys.modules.get(k) for k in ('libs', 'libs.criteria', compat.ID_LOSS_ALIAS)}
    try:
        sys.modules.pop(compat.ID_LOSS_ALIAS, None)
        compat.install()
        assert compat.ID_LOSS_ALIAS not in sys.modules
        compat.install_id_loss(str(tmp_path / 'missing.pth'))
        from libs.criteria import id_loss
        with pytest.raises(SystemExit):                           # id_loss.py:12-14: print and exit
            id_loss.IDLoss()
        assert 'does not exist' in capsys.readouterr().out
        path = str(tmp_path / 'model_ir_se50.pth')
        torch.save(S.synthetic_arcface_state(1), path)
        m = id_loss.IDLoss(path)
        assert m.facenet.input_layer[2].weight.shape == (64,)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v

"""CPU: the landmark head without a GPU -- the fp64 restatement (tests/fan_restatement.py) against the fixture kat13 written from the
reference's own FAN(4), get_preds_fromhm and transform (scripts/make_golden_fan.py), the module's key list, the decode and crop
restatements on hand-made inputs, the refused configurations, pickling, the C ABI of csrc/fan.hip and the synthetic state's scale."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import S, golden
import fan_restatement as R

from stylegan_directions_face_reenactment_amd import landmarks as L

KAT = 'kat13_fan.npz'


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def state(kat):
    return S.synthetic_fan_state(int(kat['seed']))


def check_against_fixture(kat, name, taps, dec, bar_heatmaps, bar_taps=None, label='restatement'):
    """Shared with the GPU tests: the last heatmaps against the stored full maps, top-2 values and 3 x 3 neighbourhoods within
    `bar_heatmaps`; each tap's checksums within bar_taps[tap]; arg-max, pts, pts_img and boxes exactly.  Prints every figure."""
    hm = taps['heatmaps'][-1].detach().double().cpu()
    B = hm.shape[0]
    full = [int(j) for j in kat['full']]
    e_full = float((hm[0, full] - torch.from_numpy(kat['heatmaps_full_' + name])).abs().max())
    flat = hm.reshape(B, R.POINTS, -1)
    idx = torch.from_numpy(kat['argmax_' + name])
    top2 = torch.from_numpy(kat['top2_' + name])
    e_top = float((flat.gather(2, idx.unsqueeze(2)).squeeze(2) - top2[..., 0]).abs().max())
    nbh = torch.from_numpy(kat['nbh_' + name])
    e_nbh = 0.0
    for b in range(B):
        for j in range(R.POINTS):
            py, px = int(idx[b, j]) // 64, int(idx[b, j]) % 64
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= py + dy < 64 and 0 <= px + dx < 64:
                        e_nbh = max(e_nbh, abs(float(hm[b, j, py + dy, px + dx]) - float(nbh[b, j, dy + 1, dx + 1])))
    print('%s case %s: heatmaps full %.3e, maxima %.3e, neighbourhoods %.3e   bar %.3e' % (label, name, e_full, e_top, e_nbh, bar_heatmaps))
    fails = []
    if max(e_full, e_top, e_nbh) > bar_heatmaps:
        fails.append(('heatmaps', max(e_full, e_top, e_nbh), bar_heatmaps))
    if bar_taps is not None:
        for tap, t in R.tap_list(taps):
            err = float(np.abs(R.tap_checksum(t.detach().cpu()) - kat['tap_%s_%s' % (tap, name)]).max())
            print('%s case %s: tap %-10s %.3e   bar %.3e' % (label, name, tap, err, bar_taps[tap]))
            if err > bar_taps[tap]:
                fails.append((tap, err, bar_taps[tap]))
    assert not fails, fails
    assert torch.equal(dec['idx'].cpu(), idx)
    assert np.array_equal(dec['pts'].cpu().numpy(), kat['pts_' + name])
    assert np.array_equal(dec['pts_img'].cpu().numpy(), kat['pts_img_' + name])
    assert np.array_equal(dec['boxes'].cpu().numpy(), kat['boxes_' + name])


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_matches_reference_fixture(kat, state, name):
    """Both forms of the fp64 restatement (unfolded, and folded as the kernels compute) against the reference's fp64 run: heatmaps
    and tap checksums to fp64 rounding of the heatmaps' maximum (1e-9 of it), pts / pts_img / boxes exactly."""
    x, faces = R.fixture_inputs(S, int(kat['seed']), name)
    assert np.array_equal(faces.numpy(), kat['faces_' + name])
    assert R.windows(faces) == kat['window_' + name].tolist()
    c, s = R.centre_scale(faces)
    assert np.array_equal(c.numpy(), kat['centre_' + name]) and np.array_equal(s.numpy(), kat['scale_' + name])
    crop = R.crop(x.double(), faces)
    bar = 1e-9 * float(kat['heatmaps_max_' + name])
    with torch.no_grad():
        for label, fn in (('unfolded', R.network), ('folded', R.network_folded)):
            taps = fn(state, crop)
            tb = {tap: 1e-9 * max(1.0, float(np.abs(kat['tap_%s_%s' % (tap, name)]).max())) for tap, _ in R.tap_list(taps)}
            check_against_fixture(kat, name, taps, R.decode(taps['heatmaps'][-1], faces), bar, tb, label)


def test_key_list_and_shapes_match_the_reference_module(kat, state):
    fan = L.FAN(4)
    ours = ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in fan.state_dict().items()]
    assert ours == [str(k) for k in kat['keys']]
    assert len(ours) == 1129
    fan.load_state_dict(state, strict=True)
    back = fan.state_dict()
    assert all(torch.equal(back[k], state[k]) for k in state)
    n_params = sum(p.numel() for p in fan.parameters())
    assert 23.7e6 < n_params < 23.9e6, n_params
    convs = [m for m in fan.modules() if isinstance(m, torch.nn.Conv2d)]
    bns = [m for m in fan.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert (len(convs), len(bns)) == (194, 184)
    assert not any(p.requires_grad for p in fan.parameters())


def test_decode_restatement_on_handmade_heatmaps():
    """Border maxima, zero neighbour differences and ties against a literal transcription of the loop."""
    hm, faces = R.handmade_heatmaps()
    d = R.decode(hm, faces)
    c, s = R.centre_scale(faces)
    kinds = set()
    for b in range(hm.shape[0]):
        for j in range(R.POINTS):
            m = hm[b, j]
            top = float(m.max())
            first = next(i for i, v in enumerate(m.reshape(-1).tolist()) if v == top)
            assert int(d['idx'][b, j]) == first
            px, py = first % 64, first // 64
            fx, fy = float(px + 1), float(py + 1)
            inner = 0 < px < 63 and 0 < py < 63
            if inner:
                dx, dy = float(m[py, px + 1] - m[py, px - 1]), float(m[py + 1, px] - m[py - 1, px])
                fx += 0.25 * ((dx > 0) - (dx < 0))
                fy += 0.25 * ((dy > 0) - (dy < 0))
                kinds.add(('inner', (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)))
            else:
                kinds.add(('border', px in (0, 63), py in (0, 63)))
            if int((m == top).sum()) > 1:
                kinds.add('tie')
            fx, fy = fx - 0.5, fy - 0.5
            assert d['pts'][b, j].tolist() == [4 * fx, 4 * fy]
            want = R.inv_transform(torch.tensor([fx, fy]), c[b], s[b], 64.0)
            assert d['pts_img'][b, j].tolist() == [float(want[0]), float(want[1])]
        assert d['boxes'][b].tolist() == [float(d['pts_img'][b, :, 0].min()), float(d['pts_img'][b, :, 1].min()),
                                          float(d['pts_img'][b, :, 0].max()), float(d['pts_img'][b, :, 1].max())]
    assert 'tie' in kinds and ('inner', 0, -1) in kinds and ('inner', 1, 0) in kinds and ('inner', -1, 1) in kinds
    assert ('border', False, True) in kinds and ('border', True, False) in kinds and ('border', True, True) in kinds
    # transform truncates toward zero, as .int() does: a point left of the image's origin
    far = R.inv_transform(torch.tensor([-30.0, 0.5]), torch.tensor([20.0, 20.0]), torch.tensor(1.0), 64.0)
    pre = R.inv_transform_float(torch.tensor([-30.0, 0.5]), torch.tensor([20.0, 20.0]), torch.tensor(1.0), 64.0)
    assert float(pre[0]) < -1 and int(far[0]) == int(np.trunc(float(pre[0]))) > float(pre[0])


@pytest.mark.parametrize('name', list(R.CASES))
def test_crop_restatement_equals_interpolate_of_the_clipped_window(kat, name):
    """R.crop against the window built pixel by pixel from crop_torch's own slice arithmetic, then F.interpolate."""
    x, faces = R.fixture_inputs(S, int(kat['seed']), name)
    x = x.double()
    B, _, H, W = x.shape
    mine = R.crop(x, faces)
    sizes = []
    for b in range(B):
        l1x, l1y, l2x, l2y = kat['window_' + name][b].tolist()
        win = torch.zeros(3, l2y - l1y, l2x - l1x, dtype=torch.float64)
        new_x, new_y = (max(1, -l1x + 1), min(l2x, W) - l1x), (max(1, -l1y + 1), min(l2y, H) - l1y)
        old_x, old_y = (max(1, l1x + 1), min(l2x, W)), (max(1, l1y + 1), min(l2y, H))
        win[:, new_y[0] - 1:new_y[1], new_x[0] - 1:new_x[1]] = x[b, :, old_y[0] - 1:old_y[1], old_x[0] - 1:old_x[1]]
        want = F.interpolate(win[None], size=(256, 256), mode='bilinear', align_corners=False) / 255.0
        assert float((mine[b:b + 1] - want).abs().max()) == 0.0
        sizes.append(win.shape[1:])
        padded = int((win.abs().sum(0) == 0).sum())
        print('case %s row %d: window %s of image %dx%d, %d zero pixels' % (name, b, tuple(win.shape[1:]), H, W, padded))
        if name == 'a':
            assert l1x < 0 and l1y < 0 and l2x > W and l2y > H and padded > 0          # padding and clipping both active
    if name == 'b':
        assert max(sizes[0]) > 256 > max(sizes[1])                                     # one scaled down, one scaled up
    g = R.crop(R.to_gan(x), faces, input_range='gan')
    assert float((g - mine).abs().max()) <= 1e-6                                       # the range map's twin


def test_refused_configurations_raise_before_any_launch():
    for n in (1, 2, 3, 5):
        with pytest.raises(NotImplementedError):
            L.FAN(n)
    fan = L.FAN(4)
    assert not any(p.requires_grad for p in fan.parameters())
    x, faces = torch.zeros(2, 3, 64, 64), torch.tensor([[10.0, 10.0, 50.0, 50.0]] * 2)
    with pytest.raises(RuntimeError, match='eval mode'):
        L.get_landmarks(fan, x, faces)                     # a fresh module is in training mode
    fan.eval()
    fan.l3.weight.requires_grad = True
    with pytest.raises(RuntimeError, match='no gradient for the weights'):
        L.get_landmarks(fan, x, faces)
    fan.l3.weight.requires_grad = False
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.get_landmarks(fan, x, faces)
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.get_landmarks(fan, x, faces.tolist(), input_range='gan')
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.kpt68_boxes(torch.zeros(2, 68, 2))
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.crop(x, faces)
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.decode(torch.zeros(2, 68, 64, 64), faces)
    with pytest.raises(RuntimeError, match='no CPU path'):
        fan(torch.zeros(1, 3, 256, 256))
    for bad in (torch.zeros(2, 1, 64, 64), torch.zeros(3, 64, 64), torch.zeros(2, 3, 64)):
        with pytest.raises(ValueError, match='images'):
            L.get_landmarks(fan, bad, faces)
    for bad in (torch.zeros(2, 3), torch.zeros(3, 4), torch.zeros(2, 6), torch.zeros(8), [[1.0, 2.0, 3.0]] * 2):
        with pytest.raises(ValueError, match='face boxes'):
            L.get_landmarks(fan, x, bad)
    L._faces(torch.zeros(2, 5), x)                         # a score column is accepted
    for bad in ('256', 'GAN', None, 1):
        with pytest.raises(ValueError, match='input_range'):
            L.get_landmarks(fan, x, faces, input_range=bad)
    with pytest.raises(ValueError, match='points'):
        L.kpt68_boxes(torch.zeros(2, 67, 2))
    with pytest.raises(ValueError, match='heatmaps'):
        L.decode(torch.zeros(2, 68, 32, 32), faces)
    with pytest.raises(ValueError, match='crops'):
        fan(torch.zeros(1, 3, 224, 224))
    fan.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        fan(torch.zeros(1, 3, 256, 256))


def test_deepcopy_and_pickle_drop_the_pack():
    fan = L.FAN(4).eval()
    fan._pack = ('key', torch.zeros(1), [])
    f2 = pickle.loads(pickle.dumps(fan))
    assert f2._pack is None and not f2.training
    f3 = copy.deepcopy(fan)
    assert f3._pack is None
    assert list(f2.state_dict().keys()) == list(fan.state_dict().keys())
    fan.load_state_dict(fan.state_dict())
    assert fan._pack is None
    fan._pack = ('key', torch.zeros(1), [])
    fan.double().float()
    assert fan._pack is None


def test_native_symbols_and_sizes():
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()
    header = open(_native.os.path.join(_native._HERE, '..', 'include', 'sgdfr.h')).read()
    names = ('sgdfr_fan_pack_elems', 'sgdfr_fan_prepack_f32', 'sgdfr_fan_workspace_bytes', 'sgdfr_fan_debug_elems', 'sgdfr_fan_forward_f32',
             'sgdfr_fan_crop_f32', 'sgdfr_fan_decode_f32', 'sgdfr_fan_network_f32', 'sgdfr_fan_boxes_f32')
    for name in names:
        assert hasattr(lib, name), name
        assert name + '(' in header, name
    fan = L.FAN(4)
    folded = fan.folded()
    assert _native.FAN_PARAMS == 735 == len(folded)
    assert sum(v is None for v in folded) == 3 * 57                          # 57 of the 59 blocks have no projection
    n_folded = sum(v.numel() for v in folded if v is not None)
    assert n_folded <= lib.sgdfr_fan_pack_elems() < n_folded + 64 * len(folded)      # every tensor once, 64-float alignment
    for rows in (1, 3):
        v = L.debug_views(torch.zeros(lib.sgdfr_fan_debug_elems(rows)), rows)        # asserts the total
        assert len(v['hg']) == len(v['heatmaps']) == 4 and tuple(v['stem'].shape) == (rows, 64, 128, 128)
    assert lib.sgdfr_fan_debug_elems(0) == -1 and lib.sgdfr_fan_workspace_bytes(1, 0, 256) == -1 and lib.sgdfr_fan_workspace_bytes(0, 9, 9) == -1
    assert lib.sgdfr_fan_workspace_bytes(2, 256, 256) > lib.sgdfr_fan_workspace_bytes(1, 256, 256) > 0
    p8 = ctypes.c_void_p(8)
    rc = lib.sgdfr_fan_forward_f32(None, None, 1, 256, 256, 0, None, None, None, None, None, None, None, 0, None)
    assert rc != 0 and b'null pointer' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_forward_f32(p8, p8, 0, 256, 256, 0, p8, p8, p8, p8, p8, None, p8, 1 << 40, None)
    assert rc != 0 and b'unsupported size' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_forward_f32(p8, p8, 1, 256, 256, 7, p8, p8, p8, p8, p8, None, p8, 1 << 40, None)
    assert rc != 0 and b'input_range' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_forward_f32(p8, p8, 1, 256, 256, 0, p8, p8, p8, p8, p8, None, p8, 16, None)
    assert rc != 0 and b'workspace' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_network_f32(None, 1, None, None, None, None, 0, None)
    assert rc != 0 and b'null pointer' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_network_f32(p8, -1, p8, p8, None, p8, 1 << 40, None)
    assert rc != 0 and b'unsupported size' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_crop_f32(None, None, 1, 64, 64, 0, None, None)
    assert rc != 0 and b'null pointer' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_crop_f32(p8, p8, 0, 64, 64, 0, p8, None)
    assert rc != 0 and b'unsupported size' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_decode_f32(None, None, 1, None, None, None, None)
    assert rc != 0 and b'null pointer' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_decode_f32(p8, p8, 0, p8, p8, None, None)
    assert rc != 0 and b'unsupported size' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_boxes_f32(None, 1, None, None)
    assert rc != 0 and b'null pointer' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_boxes_f32(p8, 0, p8, None)
    assert rc != 0 and b'unsupported size' in lib.sgdfr_last_error()
    arr = (ctypes.c_void_p * _native.FAN_PARAMS)()
    rc = lib.sgdfr_fan_prepack_f32(arr, p8, None)
    assert rc != 0 and b'parameter 0 is null' in lib.sgdfr_last_error()
    rc = lib.sgdfr_fan_prepack_f32(None, None, None)
    assert rc != 0 and b'null pointer' in lib.sgdfr_last_error()


def test_synthetic_state_keeps_activations_in_range(kat, state):
    """fp32 on the CPU, one 256^2 crop: every debug tap stays within 1e-2 ... 1e2 (rms above 1e-2, largest magnitude below 1e2)."""
    crop = S.counter_tensor(7, 'fan.scale.crop', (1, 3, 256, 256), 0.5, 0.25).clamp(0, 1)
    with torch.no_grad():
        taps = R.network(state, crop)
    for tap, t in R.tap_list(taps):
        rms, top = float(t.pow(2).mean().sqrt()), float(t.abs().max())
        print('tap %-10s rms %.3f max %.2f' % (tap, rms, top))
        assert 1e-2 <= rms <= 1e2 and top <= 1e2, (tap, rms, top)
    again = S.synthetic_fan_state(int(kat['seed']))
    assert torch.equal(again['m2.b2_plus_1.conv2.weight'], state['m2.b2_plus_1.conv2.weight'])

"""CPU: flip_input, the Gaussian draw and the 3D landmark type without a GPU -- the restatement (tests/fan3d_restatement.py) against
the fixture kat21 written from the reference's own flip, draw_gaussian and ResNetDepth (scripts/make_golden_fan3d.py): the flip sum
and the drawn maps bit for bit, the network taps in fp64 to fp64 rounding in both forms, the assembly of pts_img3, the module's key
list, ResNetDepth.folded() against the unfolded modules, the refused configurations and the size queries of the C ABI."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import S, golden
import fan_restatement as R
import fan3d_restatement as R3

from stylegan_directions_face_reenactment_amd import _native as N, landmarks as L

KAT = 'kat21_fan3d.npz'
CASES = ('a', 'b', 'c')
MODES = ('plain', 'flip')


@pytest.fixture(scope='module')
def kat():
    return golden(KAT)


@pytest.fixture(scope='module')
def state(kat):
    return S.synthetic_fan_depth_state(int(kat['depth_seed']))


def test_flip_add_restatement_equals_the_reference_sum_bit_for_bit(kat):
    hm2 = S.counter_tensor(int(kat['seed']), 'fan3d.flip.hm2', (2, 68, 64, 64))
    out = R3.flip_add(hm2)
    assert tuple(out.shape) == (1, 68, 64, 64) and out.dtype == torch.float32
    bad = (int((out[0, :, ::8, ::8].numpy() != kat['flipadd_sub']).sum()), int((out[0].double().sum(2).numpy() != kat['flipadd_rowsum']).sum()),
           int((out[0].double().sum(1).numpy() != kat['flipadd_colsum']).sum()))
    print('flip sum: %d sampled values, %d row sums and %d column sums differ' % bad)
    assert bad == (0, 0, 0)
    assert sorted(R3.PAIRS) == list(range(68)) and all(R3.PAIRS[R3.PAIRS[c]] == c for c in range(68))      # an involution


def test_draw_restatement_equals_draw_gaussian_bit_for_bit(kat):
    R3.check_maps(kat, 'edge', R3.draw(R3.edge_points()), 'restatement')
    count = kat['draw_count_edge']
    n = len(R3.EDGE)
    # the branches of the injected list, row 0: x = -3 and 0 draw nothing, 262 draws one column, 263 nothing; y = -3 draws 3 rows
    assert count[0, 0] == 0 and count[0, 1] == 0 and count[0, n - 1] == 0 and kat['draw_box_edge'][0, n - 2].tolist()[1:] == [255, 13, 1]
    assert kat['draw_box_edge'][0, n].tolist() == [0, 83, 3, 13] and count[0, 8] == 169
    for name in CASES:
        for mode in MODES:
            tag = '%s_%s' % (mode, name)
            R3.check_maps(kat, tag, R3.draw(torch.from_numpy(kat['pts_' + tag])), 'restatement')
    g = R3.gaussian13()
    assert float(g[6, 6]) == 1.0 and torch.equal(g, g.t()) and torch.equal(g, g.flip(0))


@pytest.mark.parametrize('name', CASES)
def test_depth_restatement_matches_reference_fixture(kat, state, name):
    """Both forms of the fp64 restatement against the reference's fp64 run on the reference's own drawn maps: tap checksums and
    depths to fp64 rounding (1e-9 of the tap's size), then pts_img3: x and y exactly, z to the same rounding."""
    x, faces = R3.case_inputs(S, int(kat['seed']), name)
    assert np.array_equal(faces.numpy(), kat['faces_' + name])
    assert np.array_equal(R3.z_factor(faces).numpy(), kat['zfac_' + name])
    crop = R.crop(x.double(), faces)
    for mode in MODES:
        tag = '%s_%s' % (mode, name)
        maps = R3.draw(torch.from_numpy(kat['pts_' + tag])).double()
        with torch.no_grad():
            for label, fn in (('unfolded', R3.depth_network), ('folded', R3.depth_network_folded)):
                if mode == 'flip' and label == 'unfolded':
                    continue
                taps = fn(state, crop, maps)
                for tap, t in R3.tap_list(taps):
                    key = 'tap_%s_%s' % (tap, tag)
                    if key not in kat.files:
                        continue
                    want = kat[key]
                    err, bar = float(np.abs(R3.tap_checksum(t) - want).max()), 1e-9 * max(1.0, float(np.abs(want).max()))
                    print('%s case %s: tap %-7s %.3e   bar %.3e' % (label, tag, tap, err, bar))
                    assert err <= bar
                want = torch.from_numpy(kat['depth_' + tag])
                err = float((taps['depth'] - want).abs().max())
                assert err <= 1e-9 * float(want.abs().max()), err
                assert 1.0 < float(want.abs().max()) < 200.0 and float(want.abs().median()) > 1.0       # depths of order 1 to 100
                p3 = torch.from_numpy(kat['pts_img3_' + tag])
                zf = torch.from_numpy(kat['zfac_' + name]).double().view(-1, 1)
                assert torch.equal(p3[..., :2].float(), torch.from_numpy(kat['pts_img_' + tag]))
                ez = float((taps['depth'] * zf - p3[..., 2]).abs().max())
                print('%s case %s: z against the fixture %.3e' % (label, tag, ez))
                assert ez <= 1e-9 * float(p3[..., 2].abs().max())
        got = R3.assemble(torch.from_numpy(kat['pts_img_' + tag]), taps['depth'], faces)
        assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0], 68, 3)
        assert float((got.double() - p3).abs().max()) <= 2.0 ** -22 * float(p3[..., 2].abs().max())
    if name == 'c':
        assert float(kat['zfac_c'].max() / kat['zfac_c'].min()) > 1.9                                   # the scales differ


def test_key_list_and_shapes_match_the_reference_module(kat, state):
    net = L.ResNetDepth()
    ours = ['%s:%s' % (k, ','.join(map(str, v.shape))) for k, v in net.state_dict().items()]
    assert ours == [str(k) for k in kat['depth_keys']] and len(ours) == 932
    assert list(state.keys()) == [k.split(':')[0] for k in ours]
    # the reference's checkpoint carries a 'module.' prefix that landmarks_estimation.py:136-138 strips
    wrapped = {'module.' + k: v for k, v in state.items()}
    net.load_state_dict({k.replace('module.', ''): v for k, v in wrapped.items()}, strict=True)
    back = net.state_dict()
    assert all(torch.equal(back[k], state[k]) for k in state)
    n_params = sum(p.numel() for p in net.parameters())
    assert 58.4e6 < n_params < 58.6e6, n_params
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert (len(convs), len(bns), len(net.bottlenecks())) == (155, 155, 50)
    assert not any(p.requires_grad for p in net.parameters())
    assert len(net.folded()) == N.FANDEPTH_PARAMS == 312


def test_folded_weights_against_the_unfolded_modules_in_fp64(kat, state):
    """A forward written on ResNetDepth.folded(float64)'s 312 tensors in the order the prepack takes them against the unfolded
    restatement."""
    net = L.ResNetDepth()
    net.load_state_dict(state, strict=True)
    net.eval()
    P = iter(net.folded(torch.float64))
    x, faces = R3.case_inputs(S, int(kat['seed']), 'a')
    crop = R.crop(x.double(), faces)
    maps = R3.draw(torch.from_numpy(kat['pts_plain_a'])).double()
    with torch.no_grad():
        want = R3.depth_network(state, crop, maps)['depth']
        h = F.max_pool2d(torch.relu(F.conv2d(torch.cat([crop, maps], 1), next(P), next(P), stride=2, padding=3)), 3, stride=2, padding=1)
        for _, stride, ds in R3.blocks():
            w1, b1, w2, b2, w3, b3 = (next(P) for _ in range(6))
            res = F.conv2d(h, next(P), next(P), stride=stride) if ds else h
            o = torch.relu(F.conv2d(torch.relu(F.conv2d(h, w1, b1)), w2, b2, stride=stride, padding=1))
            h = torch.relu(F.conv2d(o, w3, b3) + res)
        got = F.linear(F.avg_pool2d(h, 7).flatten(1), next(P), next(P))
    assert next(P, None) is None
    err = float((got - want).abs().max())
    print('folded against unfolded: depth differs by %.3e of %.3e' % (err, float(want.abs().max())))
    assert err <= 1e-9 * float(want.abs().max())
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in net.folded())


def test_refused_configurations_and_size_queries():
    net = L.ResNetDepth()
    net.train()
    with pytest.raises(RuntimeError, match='eval mode only'):
        net.check()
    net.eval()
    net.check()
    net.fc.bias.requires_grad_(True)
    with pytest.raises(RuntimeError, match='forward only'):
        net.check()
    c = copy.deepcopy(net)
    assert c._pack is None
    lib = N.load()
    assert lib.sgdfr_abi_version() == 23
    folded = sum(t.numel() for t in net.folded())           # filters + one bias per channel: the BatchNorm scales are folded away
    assert folded <= lib.sgdfr_fandepth_pack_elems() <= folded + 64 * N.FANDEPTH_PARAMS      # each tensor padded to 64 floats
    for rows in (0, -1, 257):
        assert lib.sgdfr_fandepth_workspace_bytes(rows) == -1 and lib.sgdfr_fandepth_debug_elems(rows) == -1
    assert lib.sgdfr_fandepth_debug_elems(2) == 2 * (64 * 128 * 128 + 64 * 64 * 64 + 256 * 64 * 64 + 512 * 32 * 32 + 1024 * 16 * 16
                                                     + 2048 * 8 * 8 + 2048)
    assert lib.sgdfr_fandepth_workspace_bytes(2) > lib.sgdfr_fandepth_workspace_bytes(1) > 0
    # a flip call runs the network on 2B rows: the row limit halves, with the existing error
    assert lib.sgdfr_fan_workspace_bytes(256, 64, 64) > 0 and lib.sgdfr_fan_workspace_bytes(2 * 129, 64, 64) == -1
    with pytest.raises(ValueError, match='expected .2B,68,64,64. heatmaps'):
        L.flip_add(torch.zeros(3, 68, 64, 64))
    with pytest.raises(ValueError, match='expected .B,68,2. points'):
        L.draw(torch.zeros(1, 67, 2))
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.draw(torch.zeros(1, 68, 2))
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.flip_add(torch.zeros(2, 68, 64, 64))

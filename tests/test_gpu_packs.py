"""The shared pack cache (packs.PackedWeights) on the device, for each of the seven heads on synthetic weights: prepack launches only,
no forward pass.  What the network computes from a pack is the business of each head's own tests.

A prepack writes the pack's entries and leaves the padding between them (every entry starts at a multiple of 64 floats) as the
allocator handed it over, so two packs of the same weights agree only where they are written.  The packs of this test are therefore
allocated full of NaN, and compared as bit patterns: equal where written, and the same places left unwritten."""
import pytest
import torch

from util import SEED

pytestmark = pytest.mark.gpu


def _backbone(S):
    from stylegan_directions_face_reenactment_amd.id_loss import Backbone
    return Backbone(), S.synthetic_arcface_state(SEED)


def _resnet_encoder(S):
    from stylegan_directions_face_reenactment_amd.deca import ResnetEncoder
    return ResnetEncoder(), S.synthetic_deca_encoder_state(SEED)


def _fan(S):
    from stylegan_directions_face_reenactment_amd.landmarks import FAN
    return FAN(4), S.synthetic_fan_state(SEED)


def _s3fd(S):
    from stylegan_directions_face_reenactment_amd.face_detector import S3FD
    return S3FD(), S.synthetic_s3fd_state(SEED)


def _flame(S):
    from stylegan_directions_face_reenactment_amd.flame import FLAME
    return FLAME(), S.synthetic_flame_state(SEED)


def _lpips(S):
    from stylegan_directions_face_reenactment_amd.lpips import LPIPS
    return LPIPS(), S.synthetic_lpips_state(SEED)


def _e4e(S):
    from stylegan_directions_face_reenactment_amd.encoder import Encoder4Editing
    enc = Encoder4Editing(50, 'ir_se', 32)
    return enc, S.synthetic_encoder_state(enc.state_dict(), SEED)


HEADS = {'Backbone': _backbone, 'ResnetEncoder': _resnet_encoder, 'FAN': _fan, 'S3FD': _s3fd, 'FLAME': _flame, 'LPIPS': _lpips,
         'Encoder4Editing': _e4e}


def _nan_empty(*size, **kw):
    return torch.full(size[0] if len(size) == 1 and not isinstance(size[0], int) else size, float('nan'), **kw)


@pytest.mark.parametrize('name', list(HEADS))
def test_pack_is_cached_follows_the_weights_and_leaves_with_the_device(name, monkeypatch):
    from stylegan_directions_face_reenactment_amd import synthetic as S
    m, state = HEADS[name](S)
    m.load_state_dict(state, strict=True)
    m = m.eval().cuda()
    assert m._pack is None
    monkeypatch.setattr(torch, 'empty', _nan_empty)                      # packed() allocates the pack with torch.empty
    p0 = m.packed()
    assert m.packed() is p0 and m._pack[1] is p0                         # no change, no rebuild
    assert p0.is_cuda and p0.dtype == torch.float32 and p0.dim() == 1
    written = int((~torch.isnan(p0)).sum())
    print('%s: pack of %d floats, %d written' % (name, p0.numel(), written))
    assert 0 < written <= p0.numel()
    weight = max((t for t in m.state_dict(keep_vars=True).values() if t.is_floating_point()), key=lambda t: t.numel())
    with torch.no_grad():
        weight.add_(0)                                                   # bumps the version counter, changes no value
    p1 = m.packed()
    assert p1 is not p0 and p1.data_ptr() != p0.data_ptr() and m.packed() is p1
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32))
    m.invalidate_packs()
    assert m._pack is None
    p2 = m.packed()
    assert p2 is not p1 and torch.equal(p2.view(torch.int32), p0.view(torch.int32))
    monkeypatch.undo()
    m = m.cpu()
    assert m._pack is None

"""GPU: the Reenactor on a generator above 256^2: the 512 generator (cm = 1, 16 latents) with Encoder4Editing(50, 'ir_se', 512) on the
256 x 256 alignment crop (16 heads on the HIP encoder), rendered through a session that pools to 256, and PTI with the pooled loss
(finetune.PooledPtiLoss).  The frames, the detector, FAN, DECA and the shift tables are those of tests/test_gpu_reenactor.py's Rig:
256 x 256 generated faces that the rig proves usable, so the source's usability does not depend on the new generator."""
import copy

import pytest
import torch

from util import S, SEED, hip_generator
from test_gpu_reenactor import D, Rig, bits

pytestmark = pytest.mark.gpu


class HiresRig:
    def __init__(self):
        from stylegan_directions_face_reenactment_amd.encoder import Encoder4Editing
        self.rig = Rig()
        self.G = hip_generator(512, 1)
        enc = Encoder4Editing(50, 'ir_se', 512).eval()
        enc.load_state_dict(S.synthetic_encoder_state(enc.state_dict(), seed=SEED + 512), strict=True)
        assert (enc.style_count, enc.input_size, self.G.n_latent) == (16, 256, 16)
        self.enc = enc.cuda()

    def reenactor(self, batch=2, lpips=None):
        from stylegan_directions_face_reenactment_amd.reenact import Reenactor
        g = self.rig
        return Reenactor(self.G, g.A, self.enc, g.det, g.fan, g.E, g.shifts, truncation=0.7, trunc=g.trunc, lpips=lpips, batch=batch)


@pytest.fixture(scope='module')
def hi():
    return HiresRig()


def test_reenact_on_the_512_generator_is_the_composition(hi):
    """optimize=False, 3 frames in chunks of 2 and 1: video bytes, ok and the shift vectors equal the sequence written out from
    public calls: preprocess_frames, invert_images (16 codes), shape_params, make_shift, ReenactmentSession(pool_to=256).video_frames.
    Before the head count was apart from the input side this construction raised in encode."""
    from stylegan_directions_face_reenactment_amd import reenact as RE
    from stylegan_directions_face_reenactment_amd.face_detector import detect_landmarks
    from stylegan_directions_face_reenactment_amd.train_step import shape_params
    g = hi.rig
    r = hi.reenactor(batch=2)
    assert r.pool_to == 256
    info = r.set_source(g.source, optimize=False)
    assert r.G_source is hi.G and info['loss'] is None
    assert tuple(info['source_code'].shape) == (1, 16, 512) and tuple(info['inverted'].shape) == (1, 3, 512, 512)
    faces = g.faces[:3].contiguous()
    video, ok, sv = r.reenact(faces)

    with torch.no_grad():
        crop, x, src_ok = RE.preprocess_frames(g.det, g.fan, g.source.unsqueeze(0))
        code, inverted = RE.invert_images(hi.enc, hi.G, x, 0.7, g.trunc)
        params_source, angles_source = shape_params(g.det, g.fan, g.E, x)
        xs, svs, oks = [], [], []
        for lo in range(0, 3, 2):
            _, xt, ok_t = RE.preprocess_frames(g.det, g.fan, faces[lo:lo + 2])
            _, boxes, has = detect_landmarks(g.det, g.fan, xt, input_range='gan')
            params_target, angles_target = shape_params(g.det, g.fan, g.E, xt, boxes=boxes, has_face=has)
            svs.append(g.shifts.make_shift(angles_source, angles_target, params_source, params_target))
            xs.append(xt)
            oks.append(ok_t & has)
        want_ok = torch.cat(oks)
        want_sv, _, _ = RE.hold_failed_rows(torch.cat(svs), want_ok, torch.zeros(D, device='cuda'), torch.zeros((), dtype=torch.bool, device='cuda'))
        sess = RE.ReenactmentSession(hi.G, g.A, code, 0.7, g.trunc, batch=2, shifts=g.shifts, pool_to=256)
        want = sess.video_frames(x, torch.cat(xs), want_sv, swap_rb=True)
        pooled = RE.video_frames_uint8(RE.ReenactmentSession(hi.G, g.A, code, 0.7, g.trunc, batch=2, shifts=g.shifts).render(want_sv), [], 256,
                                       swap_rb=True)
    print('hires reenact: source ok %s, target ok %s' % (src_ok.tolist(), want_ok.tolist()))
    assert bool(src_ok.all()) and want_ok.tolist() == [True] * 3
    assert torch.equal(info['crop'], crop) and bits(info['x'], x) and bits(info['source_code'], code) and bits(info['inverted'], inverted)
    assert torch.equal(ok, want_ok) and bits(sv, want_sv)
    assert video.shape == (3, 256, 768, 3) and video.dtype == torch.uint8 and torch.equal(video, want)
    # the reenacted panel is the unpooled render of a plain session through video_frames_uint8, up to one grey level where a second
    # generator call picks another verified arithmetic
    d = (video[:, :, 512:].int() - pooled.int()).abs()
    print('hires reenact: reenacted panel against render -> video_frames_uint8: max byte diff %d, %.4f %% differ' % (
        int(d.max()), 100 * float((d != 0).float().mean())))
    assert pooled.shape == (3, 256, 256, 3) and int(d.max()) <= 1 and float((d != 0).float().mean()) <= 0.01
    assert len({tuple(row) for row in sv.tolist()}) == 3 and not torch.equal(video[0, :, 512:], video[1, :, 512:])


def test_make_source_with_pooled_pti_on_the_512_generator(hi):
    """make_source(optimize=True, opt_steps=6) no longer raises for G.size = 512: the base G is bit-unchanged, the tuned copy is
    what finetune.optimize_g gives with a PooledPtiLoss built by hand, and the loss is below the first step's.  The generator
    backward accumulates weight gradients with fp32 atomics, so two PTI runs agree to the tolerance the suite holds two runs of the
    same steps to (test_pti_with_the_real_loss_graph_replay_matches_eager_steps: rtol 2e-3, atol 2e-4), not bit for bit."""
    from stylegan_directions_face_reenactment_amd import finetune
    g = hi.rig
    before = {k: v.detach().clone() for k, v in hi.G.state_dict().items()}
    r = hi.reenactor(batch=2, lpips=g.lpips)
    src = r.make_source(g.source, optimize=True, opt_steps=6)
    torch.cuda.synchronize()
    after = hi.G.state_dict()
    assert list(after) == list(before) and all(bits(after[k], before[k]) if before[k].dtype == torch.float32 else torch.equal(after[k], before[k])
                                                for k in before)
    assert src.G_source is not hi.G and not src.G_source.training and not any(p.grad is not None for p in src.G_source.parameters())
    assert tuple(src.inverted.shape) == (1, 3, 512, 512) and tuple(src.code.shape) == (1, 16, 512)      # the generator's own size
    # by hand
    loss_fn = finetune.PooledPtiLoss(g.lpips, src.x, 256)
    with torch.no_grad():
        img, _ = hi.G([src.code], input_is_latent=True, truncation=0.7, truncation_latent=g.trunc)
        first = float(loss_fn(img, src.x, 100))
    G2 = copy.deepcopy(hi.G)
    G2.invalidate_packs()
    G2, loss2 = finetune.optimize_g(G2, src.code, src.x, g.trunc, opt_steps=6, lr=3e-3, optimize_all=False, loss_fn=loss_fn, truncation=0.7)
    tuned, hand = src.G_source.state_dict(), G2.state_dict()
    changed = [k for k in before if not torch.equal(tuned[k], before[k])]
    worst = max(float((tuned[k].float() - hand[k].float()).abs().max()) for k in before)
    print('pooled PTI at 512, 6 steps: loss %.6g (first step %.6g, by hand %.6g); %d of %d tensors changed; max |tuned - by hand| %.3e' % (
        float(src.loss), first, float(loss2), len(changed), len(before), worst))
    assert src.loss.is_cuda and src.loss.dim() == 0 and float(src.loss) < first
    assert changed and all(k.startswith('convs.') for k in changed)
    assert abs(float(src.loss) - float(loss2)) <= 2e-3 * abs(float(loss2))
    for k in before:
        assert torch.allclose(tuned[k], hand[k], rtol=2e-3, atol=2e-4), k
    # the source renders: a session on the tuned copy, pooled to 256
    r.use_source(src)
    video, ok, _ = r.reenact(g.faces[:2].contiguous())
    assert video.shape == (2, 256, 768, 3) and ok.tolist() == [True, True] and r.session.G is src.G_source and r.session.pool_to == 256
    assert hi.G.saturated_pairs() == 0

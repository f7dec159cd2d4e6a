"""GPU: the reenactment pipeline (reenact.Reenactor), sessions that pool to 256 (ReenactmentSession(pool_to=...)) and the one launch
below them (sgdfr_video_frames_f32 through reenact.video_frames_uint8).  All networks carry synthetic weights, built the way each
head's own GPU test builds them.

Bars.  The fused frames are the existing kernels' arithmetic without the float intermediate: equal bytes.  A pooled session against
generic.generate_image row by row: IMG_TOL = 2e-4 (the bar of tests/test_gpu_generator.py), its video frames within one count and at
most 1 % of the bytes different (tests/test_gpu_sweeps.py).  Reenactor.reenact against the same sequence written out from
public calls with the same chunks: the same kernels on the same numbers, equal bytes.  Every test prints the figures it asserts on.
"""
import pytest
import torch

from util import S, SEED, composed, golden, hip_generator, maxabs

pytestmark = pytest.mark.gpu

IMG_TOL = 2e-4          # the bar of tests/test_gpu_generator.py
D = 15


# ------------------------------------------------------------------ the fused frames kernel
def frames_input(shape, key):
    x = S.counter_tensor(SEED, key, shape, 0.0, 0.9).clamp_(-1.5, 1.5)
    flat = x.view(-1)
    flat[0], flat[1], flat[2], flat[3], flat[4] = 1.0, -1.0, -0.0, 1.25, -1.5          # exactly +-1, -0.0, beyond +-1
    assert float(x.abs().max()) > 1.0
    return x.cuda()


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P,f', [(8, 1), (8, 2), (8, 4), (7, 1), (7, 2), (5, 4)])
def test_fused_video_frames_equal_pool_then_grid(P, f, B):
    from stylegan_directions_face_reenactment_amd.reenact import video_frames_uint8
    key = 'reen.vf.%d.%d.%d' % (P, f, B)
    x = frames_input((B, 3, P * f, P * f), key)
    per_row = [frames_input((B, 3, P, P), key + '.p%d' % k) for k in range(3)]
    one = frames_input((1, 3, P, P), key + '.one')                                      # batch stride 0 where B > 1
    layouts = [[], [per_row[0]], [one, per_row[1]], [per_row[0], None, one], [None, per_row[2], per_row[1]]]
    checked = 0
    for panels in layouts:
        K = len(panels) + 1
        for swap_rb in (False, True):
            fill = torch.arange(B * P * K * P * 3, device='cuda').mul_(37).remainder_(251).to(torch.uint8).view(B, P, K * P, 3)
            got = video_frames_uint8(x, panels, P, swap_rb=swap_rb, out=fill.clone())
            want = composed(x, panels, P, swap_rb, fill.clone())
            assert got.shape == (B, P, K * P, 3) and torch.equal(got, want), (len(panels), swap_rb)
            for k, p in enumerate(panels):
                if p is None:                                                           # a NULL panel keeps what `out` held
                    assert torch.equal(got[:, :, k * P:(k + 1) * P], fill[:, :, k * P:(k + 1) * P])
            if None not in panels:
                assert torch.equal(video_frames_uint8(x, panels, P, swap_rb=swap_rb), want)
            checked += 1
    # swap_rb reverses the channel order of every panel and nothing else
    a = video_frames_uint8(x, [one, per_row[1]], P, swap_rb=False)
    b = video_frames_uint8(x, [one, per_row[1]], P, swap_rb=True)
    assert torch.equal(a.flip(3), b) and not torch.equal(a, b)
    print('P=%d f=%d B=%d: %d layouts equal pool -> grid byte for byte' % (P, f, B, checked))


@pytest.mark.parametrize('P,f', [(8, 1), (8, 4)])
def test_fused_video_frames_from_a_view_off_16_bytes(P, f):
    """x offset by one float takes the dword path: the same bytes."""
    from stylegan_directions_face_reenactment_amd.reenact import video_frames_uint8
    x = frames_input((3, 3, P * f, P * f), 'reen.vf.off.%d' % f)
    left = [frames_input((1, 3, P, P), 'reen.vf.off.l'), frames_input((3, 3, P, P), 'reen.vf.off.r')]
    shifted = torch.empty(x.numel() + 1, device='cuda')[1:].view(x.shape).copy_(x)
    assert x.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    for swap_rb in (False, True):
        want = composed(x, left, P, swap_rb, None)
        assert torch.equal(video_frames_uint8(x, left, P, swap_rb=swap_rb), want)
        assert torch.equal(video_frames_uint8(shifted, left, P, swap_rb=swap_rb), want)


def test_video_frames_f32_entry_takes_stride_0_as_one_row_and_a_full_stride_as_one_per_row():
    """sgdfr_video_frames_f32 below the Python entry, which never sends stride 0 at B = 1: the C entry describes its float panels to
    the px kernels as tables of 1 row (stride 0) or B rows (stride 3 * P * P), whatever B is.  P = 7, f = 2: P * f = 14 takes the
    dword path and a panel starts 3 * P = 21 bytes into a line.  Equal bytes with pool_images -> grid_frames_uint8; the NULL panel's
    columns keep what `out` held."""
    import ctypes
    from stylegan_directions_face_reenactment_amd import _native as N
    P, f = 7, 2
    one, per_row = frames_input((1, 3, P, P), 'reen.vf.c.one'), frames_input((3, 3, P, P), 'reen.vf.c.rows')

    def entry(x, panels, strides, swap_rb, out):
        n = len(panels)
        ptrs = (ctypes.c_void_p * n)(*[None if p is None else p.data_ptr() for p in panels])
        N.call('sgdfr_video_frames_f32', N.ptr(x), x.shape[0], P, f, ptrs, (ctypes.c_int64 * n)(*strides), n, N.ptr(out), swap_rb, N.stream())
        return out

    fill = lambda B, K: torch.arange(B * P * K * P * 3, device='cuda').mul_(37).remainder_(251).to(torch.uint8).view(B, P, K * P, 3)
    x1, x3 = frames_input((1, 3, P * f, P * f), 'reen.vf.c.x1'), frames_input((3, 3, P * f, P * f), 'reen.vf.c.x3')
    for swap_rb in (0, 1):
        want = composed(x1, [one], P, swap_rb, None)
        for stride in (0, 3 * P * P):                                                   # B = 1: either stride is the panel's only row
            assert torch.equal(entry(x1, [one], [stride], swap_rb, fill(1, 2)), want), (stride, swap_rb)
        got = entry(x3, [one, per_row, None], [0, 3 * P * P, 0], swap_rb, fill(3, 4))
        assert torch.equal(got, composed(x3, [one, per_row, None], P, swap_rb, fill(3, 4)))
        assert torch.equal(got[:, :, 2 * P:3 * P], fill(3, 4)[:, :, 2 * P:3 * P])
        assert not torch.equal(got[0, :, P:2 * P], got[1, :, P:2 * P]) and torch.equal(got[0, :, :P], got[2, :, :P])


def test_fused_video_frames_python_entry_refuses_bad_shapes():
    from stylegan_directions_face_reenactment_amd.reenact import video_frames_uint8
    x = frames_input((2, 3, 8, 8), 'reen.vf.bad')
    with pytest.raises(RuntimeError, match='1, 2 or 4'):
        video_frames_uint8(frames_input((1, 3, 24, 24), 'reen.vf.f3'), [], 8)
    with pytest.raises(RuntimeError, match='left panels'):
        video_frames_uint8(x, [x[:, :, :4, :4]], 8)
    with pytest.raises(RuntimeError, match='up to 3'):
        video_frames_uint8(x, [x, x, x, x], 8)
    with pytest.raises(RuntimeError, match='skipped panel'):
        video_frames_uint8(x, [None], 8)
    with pytest.raises(RuntimeError, match='out must be'):
        video_frames_uint8(x, [x], 8, out=torch.empty(2, 8, 8, 3, dtype=torch.uint8, device='cuda'))


# ------------------------------------------------------------------ sessions that pool
def direction_matrix():
    from stylegan_directions_face_reenactment_amd.direction_matrix import DirectionMatrix
    A = DirectionMatrix(512, input_dim=D, out_dim=512, w_plus=True, num_layers=8, verbose=False)
    A.load_state_dict(S.synthetic_direction_state(SEED, num_layers=8))
    return A.cuda()


def byte_figures(got, want):
    d = (got.to(torch.int16) - want.to(torch.int16)).abs()
    return int(d.max()), float((d != 0).float().mean())


def test_pooled_session_on_a_512_generator():
    """f = 2, B = 3 in chunks of 2 and 1: render(pool_to=256) against generic.generate_image row by row, video_frames against the grid
    of those images, streaming against render; pool_to=None still hands back the generator's own size."""
    from stylegan_directions_face_reenactment_amd.generic import generate_image
    from stylegan_directions_face_reenactment_amd.reenact import ReenactmentSession, grid_frames_uint8, images_to_uint8
    G, A = hip_generator(512, 1), direction_matrix()
    w = S.synthetic_latents(SEED, 1, n_latent=G.n_latent, key='reen.512.w').cuda()
    trunc = S.counter_tensor(SEED, 'reen.512.trunc', (1, 512)).cuda()
    sv = S.counter_tensor(SEED, 'reen.512.sv', (3, D), 0.0, 2.0).cuda()
    src = S.counter_tensor(SEED, 'reen.512.src', (1, 3, 256, 256), 0.0, 0.5).clamp_(-1, 1).cuda()
    tgt = S.counter_tensor(SEED, 'reen.512.tgt', (3, 3, 256, 256), 0.0, 0.5).clamp_(-1, 1).cuda()
    with torch.no_grad():                                                 # run_inference.py:179-181, one row at a time
        loop = torch.cat([generate_image(G, w, 0.7, trunc, True, 8, shift_code=A(sv[i:i + 1]), input_is_latent=True) for i in range(3)])
        full = torch.cat([G([generate_shifted(G, A, w, sv[i:i + 1])], input_is_latent=True, truncation=0.7, truncation_latent=trunc)[0]
                          for i in range(3)])
    assert loop.shape == (3, 3, 256, 256) and full.shape == (3, 3, 512, 512)
    sess = ReenactmentSession(G, A, w, 0.7, trunc, batch=2, pool_to=256)
    images = sess.render(sv)
    err = maxabs(images, loop)
    print('pooled render vs generate_image row by row: max |diff| = %.3e (bar %.0e)' % (err, IMG_TOL))
    assert images.shape == (3, 3, 256, 256) and err <= IMG_TOL
    # uint8 frames and the video grid: within one count of the loop's, at most 1 % of the bytes different
    for name, got, want in (('render(as_uint8)', sess.render(sv, as_uint8=True), images_to_uint8(loop)),
                            ('video_frames', sess.video_frames(src, tgt, sv, swap_rb=True), grid_frames_uint8([src, tgt, loop], swap_rb=True))):
        worst, share = byte_figures(got, want)
        print('pooled %s vs the loop: max byte diff %d, %.4f %% of the bytes differ' % (name, worst, 100 * share))
        assert got.shape == want.shape and got.dtype == torch.uint8 and worst <= 1 and share <= 0.01
    video = sess.video_frames(src, tgt, sv, swap_rb=True)
    assert video.shape == (3, 256, 768, 3)
    assert torch.equal(video[:, :, :512], grid_frames_uint8([src, tgt], swap_rb=True))       # the left panels are the grid kernel's bytes
    # streaming hands back the chunks render concatenates
    stream = sess.streaming()
    outs = [stream.push(sv[:2]), stream.push(sv[2:]), stream.flush()]
    assert outs[0] is None and maxabs(torch.cat(outs[1:]), images) <= IMG_TOL and outs[1].shape == (2, 3, 256, 256)
    with pytest.raises(RuntimeError, match='pools to 256'):
        sess.video_frames(src[:, :, :128, :128].contiguous(), tgt, sv)
    # pool_to=None: what it returns today, images of the generator's own size
    plain = ReenactmentSession(G, A, w, 0.7, trunc, batch=2).render(sv)
    err = maxabs(plain, full)
    print('pool_to=None render vs G row by row: max |diff| = %.3e' % err)
    assert plain.shape == (3, 3, 512, 512) and err <= IMG_TOL
    assert G.saturated_pairs() == 0


def generate_shifted(G, A, w, sv):
    from stylegan_directions_face_reenactment_amd.generic import get_shifted_latent_code
    return get_shifted_latent_code(G, w, A(sv), input_is_latent=True, w_plus=True)


# ------------------------------------------------------------------ the pipeline
class Rig:
    """The networks of run_inference.py, built once for the module, and two sets of frames: five 96 x 128 noise frames (the synthetic
    detector finds a face in each, the alignment crop is valid for some) and 256 x 256 generated frames chosen so that every row is usable."""

    def __init__(self):
        import s3fd_restatement as R3
        from test_cpu_e4e_taps import make_encoder
        from stylegan_directions_face_reenactment_amd import deca as DE, face_detector as FD, landmarks as L
        from stylegan_directions_face_reenactment_amd.lpips import LPIPS
        from stylegan_directions_face_reenactment_amd.reenact import images_to_uint8, preprocess_frames
        from stylegan_directions_face_reenactment_amd.shift import ShiftVectors
        seed = int(golden('kat14_s3fd.npz')['seed'])
        self.G = hip_generator(256, 1)
        self.A = direction_matrix()
        self.det = FD.S3FD()
        self.det.load_state_dict(S.synthetic_s3fd_state(seed), strict=True)
        self.det = self.det.cuda()
        self.fan = L.FAN(4)
        self.fan.load_state_dict(S.synthetic_fan_state(20261208), strict=True)
        self.fan = self.fan.cuda().eval()
        self.E = DE.ResnetEncoder()
        self.E.load_state_dict(S.synthetic_deca_encoder_state(20261101))
        self.E = self.E.cuda().eval()
        self.enc = make_encoder('c')[0].cuda()
        self.lpips = LPIPS()
        self.lpips.load_state_dict(S.synthetic_lpips_state(SEED))
        self.lpips = self.lpips.cuda()
        self.shifts = ShiftVectors('voxceleb', D, 6.0, ranges=golden('kat8_shift.npz')['ranges_voxceleb'])
        self.trunc = S.counter_tensor(SEED, 'step.trunc', (1, 512)).cuda()
        x = R3.images(S, seed, 'reen.frames2', 5, 96, 128)
        self.small = x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
        # generated frames the synthetic detector, the alignment crop and the detector on the crop all accept (one host read, here)
        with torch.no_grad():
            z = torch.cat([S.synthetic_z(SEED, 6, key='step.zs'), S.synthetic_z(SEED, 6, key='step.zt')]).cuda()
            img, _ = self.G([z], truncation=0.7, truncation_latent=self.trunc)
            frames = images_to_uint8(img)
            _, x, ok = preprocess_frames(self.det, self.fan, frames)
            _, _, has = FD.detect_landmarks(self.det, self.fan, x, input_range='gan')
        good = (ok & has).nonzero().flatten().tolist()
        print('rig: usable generated frames %s of %d' % (good, frames.shape[0]))
        assert len(good) >= 7
        frames = frames[good[:7]]
        self.faces, self.source, self.source2 = frames[:5].contiguous(), frames[5].contiguous(), frames[6:7].contiguous()

    def reenactor(self, batch=2, lpips=None):
        from stylegan_directions_face_reenactment_amd.reenact import Reenactor
        return Reenactor(self.G, self.A, self.enc, self.det, self.fan, self.E, self.shifts, truncation=0.7, trunc=self.trunc,
                         lpips=lpips, batch=batch)


@pytest.fixture(scope='module')
def rig():
    return Rig()


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_reenact_is_the_composition(rig):
    """N = 5 frames of 96 x 128 in chunks of 2, 2 and 1, optimize=False: video bytes, ok and the shift vectors equal
    run_inference.py:169-195 written out from public calls with the same chunks."""
    from stylegan_directions_face_reenactment_amd import reenact as RE
    from stylegan_directions_face_reenactment_amd.face_detector import detect_landmarks
    from stylegan_directions_face_reenactment_amd.train_step import shape_params
    r = rig.reenactor(batch=2)
    info = r.set_source(rig.source, optimize=False)
    assert r.G_source is rig.G and info['loss'] is None and info['crop'].shape == (1, 256, 256, 3) and info['crop'].dtype == torch.uint8
    video, ok, sv = r.reenact(rig.small)

    # ---- the same sequence, written out
    with torch.no_grad():
        crop, x, src_ok = RE.preprocess_frames(rig.det, rig.fan, rig.source.unsqueeze(0))                    # load_source_data step 1
        code, inverted = RE.invert_images(rig.enc, rig.G, x, 0.7, rig.trunc)                                # step 2
        params_source, angles_source = shape_params(rig.det, rig.fan, rig.E, x)                             # run_inference.py:169
        xs, svs, oks = [], [], []
        for lo in range(0, 5, 2):
            _, xt, ok_t = RE.preprocess_frames(rig.det, rig.fan, rig.small[lo:lo + 2])                      # :173-174
            _, boxes, has = detect_landmarks(rig.det, rig.fan, xt, input_range='gan')
            params_target, angles_target = shape_params(rig.det, rig.fan, rig.E, xt, boxes=boxes, has_face=has)   # :175
            svs.append(rig.shifts.make_shift(angles_source, angles_target, params_source, params_target))  # :178
            xs.append(xt)
            oks.append(ok_t & has)
        want_ok = torch.cat(oks)
        want_sv, _, _ = RE.hold_failed_rows(torch.cat(svs), want_ok, torch.zeros(D, device='cuda'), torch.zeros((), dtype=torch.bool, device='cuda'))
        sess = RE.ReenactmentSession(rig.G, rig.A, code, 0.7, rig.trunc, batch=2, shifts=rig.shifts)
        want = sess.video_frames(x, torch.cat(xs), want_sv, swap_rb=True)                                   # :179-195
    print('reenact: source ok %s, target ok %s' % (src_ok.tolist(), want_ok.tolist()))
    assert bool(src_ok.all()) and torch.equal(info['crop'], crop) and bits(info['x'], x) and bits(info['source_code'], code)
    assert bits(info['inverted'], inverted) and bits(info['angles'], angles_source)
    assert all(bits(info['params'][k], params_source[k]) for k in params_source)
    assert ok.dtype == torch.bool and torch.equal(ok, want_ok) and bits(sv, want_sv)
    assert video.shape == (5, 256, 768, 3) and video.dtype == torch.uint8 and torch.equal(video, want)
    # the --save_images output: the reenacted panel alone, RGB
    r.set_source(rig.source, optimize=False)                                                                # (resets the hold carry)
    images, ok2, sv2 = r.reenact(rig.small, output='images')
    assert images.shape == (5, 256, 256, 3) and torch.equal(ok2, want_ok) and bits(sv2, want_sv)
    assert torch.equal(images.flip(3), video[:, :, 512:])                                                   # swap_rb is the video path's alone


def r_after_source(rig):
    r = rig.reenactor(batch=2)
    r.set_source(rig.source, optimize=False)
    return r


def test_fail_policies_end_to_end(rig):
    """valid = [F,T,F,F,T] on five frames that are all usable: 'hold' carries row 1's vector through rows 2 and 3 and leaves row 0 at
    zero, a second call starts from row 4's vector; 'source' renders the zero shift vector; 'raise' names rows 0, 2 and 3; the frames of
    ok rows do not depend on the policy."""
    r = r_after_source(rig)
    x, native_sv, native_ok = r.target_shift_vectors(rig.faces)
    print('fail policy: native ok %s' % native_ok.tolist())
    assert native_ok.tolist() == [True] * 5 and bool(torch.isfinite(native_sv).all())
    assert len({tuple(row) for row in native_sv.tolist()}) == 5                                    # five different vectors
    valid = torch.tensor([False, True, False, False, True]).cuda()
    hold, ok, sv = r.reenact(rig.faces, valid=valid, on_fail='hold')
    assert ok.tolist() == valid.tolist()
    assert bits(sv[[1, 4]], native_sv[[1, 4]]) and bits(sv[2], native_sv[1]) and bits(sv[3], native_sv[1])
    assert (sv[0] == 0).all() and not torch.signbit(sv[0]).any()
    # a second call since set_source starts from row 4's vector
    _, ok_b, sv_b = r.reenact(rig.faces[:2], valid=torch.tensor([False, True]).cuda(), on_fail='hold')
    assert ok_b.tolist() == [False, True] and bits(sv_b[0], native_sv[4]) and bits(sv_b[1], native_sv[1])
    # 'source': the failed rows are the zero-shift render
    source, ok_s, sv_s = r.reenact(rig.faces, valid=valid, on_fail='source')
    assert ok_s.tolist() == valid.tolist() and (sv_s[[0, 2, 3]] == 0).all() and bits(sv_s[[1, 4]], native_sv[[1, 4]])
    zero = r.session.video_frames(r.source_x, x, torch.zeros(5, D, device='cuda'), swap_rb=True)
    assert torch.equal(source[[0, 2, 3]], zero[[0, 2, 3]])
    assert not torch.equal(source[1, :, 512:], zero[1, :, 512:])                                   # ... which a live row is not
    # ok rows: the same bytes under either policy; the held rows differ from the zero-shift rows
    assert torch.equal(hold[[1, 4]], source[[1, 4]]) and torch.equal(hold[0], source[0])
    assert not torch.equal(hold[2, :, 512:], source[2, :, 512:])
    # 'raise': one message naming the rows; nothing raised when every row is ok
    with pytest.raises(RuntimeError, match=r'rows \[0, 2, 3\]'):
        r.reenact(rig.faces, valid=valid, on_fail='raise')
    every, ok_r, sv_r = r.reenact(rig.faces, on_fail='raise')
    assert ok_r.tolist() == [True] * 5 and bits(sv_r, native_sv) and torch.equal(every[[1, 4]], hold[[1, 4]])
    with pytest.raises(RuntimeError, match='valid'):
        r.reenact(rig.faces, valid=valid[:4])
    with pytest.raises(RuntimeError, match='set_source'):
        rig.reenactor().reenact(rig.faces)


def test_reenact_makes_no_synchronising_torch_call(rig):
    """After three warm-up calls (weight packs, workspaces, the generator's graph captures) 'hold' and 'source' run under
    torch.cuda.set_sync_debug_mode('error').  As in tests/test_gpu_train_step.py this sees synchronisations made through torch only;
    the session's wait for each chunk's range check is made on the HIP runtime and stays."""
    r = r_after_source(rig)
    valid = torch.tensor([False, True, False, False, True]).cuda()
    for _ in range(3):
        warm = [r.reenact(rig.faces, valid=valid, on_fail=p, output=o) for p in ('hold', 'source') for o in ('video', 'images')]
    torch.cuda.synchronize()
    probe = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                                  # the mode is honoured by this build of torch
        got = [r.reenact(rig.faces, valid=valid, on_fail=p, output=o) for p in ('hold', 'source') for o in ('video', 'images')]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for (a, ok_a, sv_a), (b, ok_b, sv_b) in zip(got, warm):
        assert torch.equal(a, b) and torch.equal(ok_a, ok_b) and bits(sv_a, sv_b)


def test_set_source_with_pti_leaves_the_base_generator_pristine(rig):
    """set_source(optimize=True, opt_steps=6): every parameter and buffer of the base G is bit-equal before and after, the tuned copy
    differs, the loss is finite.  Then another source on the same Reenactor renders what a fresh Reenactor renders for it: nothing of
    the first source -- tuned weights, session, hold carry -- is left.  The second source is set without PTI: the generator backward
    accumulates weight gradients with fp32 atomics, so two PTI runs are not reproducible bit for bit, and without PTI any weight the
    first run had leaked into G would still show."""
    before = {k: v.detach().clone() for k, v in rig.G.state_dict().items()}
    r = rig.reenactor(batch=2, lpips=rig.lpips)
    info = r.set_source(rig.source, optimize=True, opt_steps=6)
    after = rig.G.state_dict()
    assert list(after) == list(before) and all(bits(after[k], before[k]) if before[k].dtype == torch.float32 else torch.equal(after[k], before[k])
                                                for k in before)
    assert r.G_source is not rig.G and r.session.G is r.G_source
    tuned = r.G_source.state_dict()
    changed = [k for k in before if not torch.equal(tuned[k], before[k])]
    loss = info['loss']
    print('PTI, 6 steps: loss %.6g; %d of %d tensors of the copy changed (%s ...)' % (float(loss), len(changed), len(before), changed[:2]))
    assert loss.is_cuda and loss.dim() == 0 and bool(torch.isfinite(loss))
    assert changed and all(k.startswith('convs.') for k in changed)                                # optimize_all=False: convs[4..11]
    assert not any(p.grad is not None for p in r.G_source.parameters()) and not r.G_source.training
    valid = torch.tensor([True, False, True, True, True]).cuda()
    tuned_video, _, _ = r.reenact(rig.faces, valid=valid)                                          # leaves a valid hold carry behind
    # ---- the next source
    r.set_source(rig.source2, optimize=False)
    assert r.G_source is rig.G
    fresh = rig.reenactor(batch=2)
    fresh.set_source(rig.source2, optimize=False)
    head = torch.tensor([False, True, False, True, True]).cuda()                                   # row 0 reads the carry: zeros after set_source
    a, ok_a, sv_a = r.reenact(rig.faces, valid=head)
    b, ok_b, sv_b = fresh.reenact(rig.faces, valid=head)
    assert (sv_a[0] == 0).all() and bits(sv_a, sv_b) and torch.equal(ok_a, ok_b) and torch.equal(a, b)
    assert not torch.equal(a[:, :, 512:], tuned_video[:, :, 512:])
    assert rig.G.saturated_pairs() == 0

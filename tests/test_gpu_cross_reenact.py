"""GPU: cross-reenactment -- the grid launch that reads uint8 and indexed panels (sgdfr_video_frames_px through
reenact.video_frames_px), and Reenactor.analyse / reenact_analysed / reenact_many / cross_metrics on the rig of
tests/test_gpu_reenactor.py (synthetic weights in every network).

Bars.  Everything here is the existing launches on the same numbers in the same chunks, so every comparison is for equal bytes / equal
bits: the px launch against pool_images -> grid_frames_uint8 on materialised float panels (util.composed: both video entries run the
px kernels, so video_frames_uint8 would be no witness), the analysis against the head chain written out from
public calls, reenact_analysed against reenact, reenact_many against set_source + reenact per source, cross_metrics against
evaluation_metrics written out.  Every test prints the figures it asserts on."""
import pytest
import torch

import cross_reenact_restatement as X
from test_gpu_reenactor import Rig, bits, direction_matrix
from util import S, SEED, composed, hip_generator

pytestmark = pytest.mark.gpu

D = 15


# ------------------------------------------------------------------ the launch
def floats(shape, key):
    x = S.counter_tensor(SEED, key, shape, 0.0, 0.9).clamp_(-1.5, 1.5)
    flat = x.view(-1)
    flat[0], flat[1], flat[2], flat[3], flat[4] = 1.0, -1.0, -0.0, 1.25, -1.5          # exactly +-1, -0.0, beyond +-1
    return x.cuda()


def crop_bytes(shape, key):
    """uint8 [rows,P,P,3] with 0 and 255 in it."""
    u = (S.counter_tensor(SEED, key, shape, 0.0, 1.0) * 97.0 + 128.0).round().clamp_(0, 255).to(torch.uint8)
    u.view(-1)[0], u.view(-1)[1] = 0, 255
    return u.cuda()


def as_float_panel(u8):
    """What the alignment crop hands on as x for these bytes: u / 255 * 2 - 1 in float32, planar.  Restated on the host: torch's
    device division by a Python scalar multiplies by the reciprocal, which is not the crop kernel's correctly rounded quotient."""
    return torch.from_numpy(X.crop_byte_to_float(u8.cpu().numpy())).permute(0, 3, 1, 2).contiguous().cuda()


def fill_bytes(B, P, K):
    return torch.arange(B * P * K * P * 3, device='cuda').mul_(37).remainder_(251).to(torch.uint8).view(B, P, K * P, 3)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P,f', [(8, 1), (8, 2), (8, 4), (7, 1), (7, 2), (5, 4)])
def test_px_frames_equal_video_frames_uint8_on_materialised_float_panels(P, f, B):
    """The px launch on every panel layout against the frames of pool_images -> grid_frames_uint8 on materialised float panels
    (util.composed).  The name is from when video_frames_uint8 supplied the expected bytes; that entry now runs the px kernels too, so
    it would be no witness, and composed gives the bytes it gave."""
    from stylegan_directions_face_reenactment_amd.reenact import video_frames_px
    key = 'cross.px.%d.%d.%d' % (P, f, B)
    x = floats((B, 3, P * f, P * f), key)
    per_row = [floats((B, 3, P, P), key + '.p%d' % k) for k in range(3)]
    one = floats((1, 3, P, P), key + '.one')
    table = floats((4, 3, P, P), key + '.table')
    u8_rows, u8_table = crop_bytes((B, P, P, 3), key + '.u'), crop_bytes((4, P, P, 3), key + '.ut')
    rows = [2, 0, 2][:B]                                                   # repeated and out of order
    wild = [7, -3, 1][:B]                                                  # outside the table: clamped into it
    index, wild_index = torch.tensor(rows, dtype=torch.int32).cuda(), torch.tensor(wild, dtype=torch.int32).cuda()
    clamped = [min(max(i, 0), 3) for i in wild]
    checked = 0
    for swap_rb in (False, True):
        ref = lambda panels, out=None: composed(x, panels, P, swap_rb, out)
        px = lambda panels, **kw: video_frames_px(x, panels, P, swap_rb=swap_rb, **kw)
        cases = [
            ('no left panel', px([]), ref([])),
            ('float broadcast', px([one]), ref([one])),
            ('float per row', px(per_row), ref(per_row)),
            ('float broadcast + per row', px([one, per_row[1]]), ref([one, per_row[1]])),
            ('float indexed', px([table], index=index), ref([table[rows]])),
            ('float indexed, one entry per panel', px([one, table], index=[None, index]), ref([one, table[rows]])),
            ('float index outside the table', px([table], index=wild_index), ref([table[clamped]])),
            ('float index on a one-row table', px([one], index=wild_index), ref([one])),
            ('uint8 per row', px([one, u8_rows]), ref([one, as_float_panel(u8_rows)])),
            ('uint8 broadcast', px([u8_table[1:2]]), ref([as_float_panel(u8_table[1:2])])),
            ('uint8 indexed', px([u8_table, per_row[0]], index=[index, None]), ref([as_float_panel(u8_table[rows]), per_row[0]])),
            ('uint8 index outside the table', px([u8_table], index=wild_index), ref([as_float_panel(u8_table[clamped])])),
            ('three uint8 panels', px([u8_rows, u8_table, u8_rows], index=[None, index, None]),
             ref([as_float_panel(u8_rows), as_float_panel(u8_table[rows]), as_float_panel(u8_rows)])),
        ]
        for name, got, want in cases:
            assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want), (name, swap_rb)
            checked += 1
        # a skipped panel keeps what `out` held
        fill = fill_bytes(B, P, 4)
        got = px([per_row[0], None, u8_rows], out=fill.clone())
        want = ref([per_row[0], None, as_float_panel(u8_rows)], out=fill.clone())
        assert torch.equal(got, want) and torch.equal(got[:, :, P:2 * P], fill[:, :, P:2 * P])
        # x=None: the last panel is whatever `out` held (the generator's last launch wrote it), the left panels are converted
        fill = fill_bytes(B, P, 3)
        got = video_frames_px(None, [one, u8_rows], P, swap_rb=swap_rb, out=fill.clone())
        assert torch.equal(got[:, :, 2 * P:], fill[:, :, 2 * P:]) and torch.equal(got[:, :, :2 * P], want_left(x, [one, as_float_panel(u8_rows)], P, swap_rb))
        got = video_frames_px(None, [table, None], swap_rb=swap_rb, out=fill.clone(), index=index)     # P from `out`
        assert torch.equal(got[:, :, P:], fill[:, :, P:]) and torch.equal(got[:, :, :P], want_left(x, [table[rows]], P, swap_rb))
        checked += 3
    a, b = video_frames_px(x, [one, u8_rows], P, swap_rb=False), video_frames_px(x, [one, u8_rows], P, swap_rb=True)
    assert torch.equal(a.flip(3), b) and not torch.equal(a, b)
    print('P=%d f=%d B=%d: %d layouts equal pool -> grid byte for byte' % (P, f, B, checked))


def want_left(x, panels, P, swap_rb):
    return composed(x, panels, P, swap_rb, None)[:, :, :len(panels) * P]


@pytest.mark.parametrize('P,f', [(8, 1), (8, 4)])
def test_px_frames_from_unaligned_views(P, f):
    """x one float off 16 bytes takes the dword path; a uint8 table that starts at an odd byte takes byte loads: the same bytes."""
    from stylegan_directions_face_reenactment_amd.reenact import video_frames_px
    x = floats((3, 3, P * f, P * f), 'cross.off.%d' % f)
    one, u8 = floats((1, 3, P, P), 'cross.off.l'), crop_bytes((3, P, P, 3), 'cross.off.u')
    shifted = torch.empty(x.numel() + 1, device='cuda')[1:].view(x.shape).copy_(x)
    odd = torch.empty(u8.numel() + 1, device='cuda', dtype=torch.uint8)[1:].view(u8.shape).copy_(u8)
    assert x.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    assert u8.data_ptr() % 4 == 0 and odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    for swap_rb in (False, True):
        want = composed(x, [one, as_float_panel(u8)], P, swap_rb, None)
        for xx in (x, shifted):
            for uu in (u8, odd):
                assert torch.equal(video_frames_px(xx, [one, uu], P, swap_rb=swap_rb), want), (swap_rb, xx is x, uu is u8)
        fill = fill_bytes(3, P, 3)
        got = video_frames_px(None, [one, odd], P, swap_rb=swap_rb, out=fill.clone())
        assert torch.equal(got[:, :, :2 * P], want[:, :, :2 * P]) and torch.equal(got[:, :, 2 * P:], fill[:, :, 2 * P:])


def test_px_frames_uint8_map_over_all_256_values():
    """A [1,16,16,3] panel holding every byte value in every channel, against the float path and against the restated table."""
    from stylegan_directions_face_reenactment_amd.reenact import uint8_panel_map, video_frames_px
    u8 = (torch.arange(16 * 16 * 3) * 7 % 256).to(torch.uint8).view(1, 16, 16, 3).cuda()
    assert sorted(set(u8.flatten().tolist())) == list(range(256))
    x = floats((1, 3, 16, 16), 'cross.map.x')
    got = video_frames_px(x, [u8], 16)
    want = composed(x, [as_float_panel(u8)], 16, False, None)
    table = uint8_panel_map().cuda()
    differ = int((got[:, :, :16] != u8).sum())
    print('exhaustive uint8 map: %d of 768 bytes differ from the input byte (the map is not the identity)' % differ)
    assert torch.equal(got, want) and torch.equal(got[:, :, :16], table[u8.long()]) and differ > 0
    # the 12-byte-per-lane dword loads (f = 1) and the byte loads (f = 4 pools a 64 x 64 x) read the same bytes
    x4 = floats((1, 3, 64, 64), 'cross.map.x4')
    assert torch.equal(video_frames_px(x4, [u8], 16)[:, :, :16], got[:, :, :16])


def test_px_python_entry_refuses_bad_arguments():
    from stylegan_directions_face_reenactment_amd.reenact import video_frames_px
    x = floats((2, 3, 8, 8), 'cross.bad')
    u8 = crop_bytes((2, 8, 8, 3), 'cross.bad.u')
    with pytest.raises(RuntimeError, match='1, 2 or 4'):
        video_frames_px(floats((1, 3, 24, 24), 'cross.bad.f3'), [], 8)
    with pytest.raises(RuntimeError, match='left panels must be'):
        video_frames_px(x, [u8.permute(0, 3, 1, 2).contiguous()], 8)                    # uint8 panels are interleaved
    with pytest.raises(RuntimeError, match='1 or 2 rows'):
        video_frames_px(x, [crop_bytes((3, 8, 8, 3), 'cross.bad.u3')], 8)
    with pytest.raises(RuntimeError, match='int32'):
        video_frames_px(x, [u8], 8, index=torch.zeros(2, dtype=torch.int64, device='cuda'))
    with pytest.raises(RuntimeError, match=r'contiguous \[2\]'):
        video_frames_px(x, [u8], 8, index=torch.zeros(3, dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError, match='no CPU path'):
        video_frames_px(x, [u8], 8, index=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='up to 3'):
        video_frames_px(x, [u8, u8, u8, u8], 8)
    with pytest.raises(RuntimeError, match='skipped panel'):
        video_frames_px(x, [None], 8)
    with pytest.raises(RuntimeError, match='skipped panel'):
        video_frames_px(None, [u8], 8)
    with pytest.raises(RuntimeError, match='out must be'):
        video_frames_px(x, [u8], 8, out=torch.empty(2, 8, 8, 3, dtype=torch.uint8, device='cuda'))


# ------------------------------------------------------------------ the pipeline
@pytest.fixture(scope='module')
def rig():
    return Rig()


def same_analysis(a, b):
    return (len(a) == len(b) and a.batch == b.batch and list(a.params) == list(b.params) and torch.equal(a.crops, b.crops)
            and bits(a.angles, b.angles) and torch.equal(a.ok, b.ok) and torch.equal(a.valid, b.valid)
            and all(bits(a.params[k], b.params[k]) for k in a.params))


def with_source(rig, frame):
    r = rig.reenactor(batch=2)
    r.set_source(frame, optimize=False)
    return r


def test_analysis_is_the_head_chain_written_out_and_joins_bit_for_bit(rig):
    """analyse(small), N = 5 in chunks of 2, 2 and 1, on a Reenactor that has no source, against run_inference.py:173-175 written out
    from public calls; the analyses of rows 0..3 and of row 4 joined equal the analysis of the whole."""
    from stylegan_directions_face_reenactment_amd import face_crop, reenact as RE
    from stylegan_directions_face_reenactment_amd.face_detector import detect_landmarks
    from stylegan_directions_face_reenactment_amd.train_step import shape_params
    r = rig.reenactor(batch=2)
    a = r.analyse(rig.small)
    assert r.session is None and len(a) == 5 and a.batch == 2
    with torch.no_grad():
        crops, angles, oks, valids, params = [], [], [], [], {}
        for lo in range(0, 5, 2):
            chunk = rig.small[lo:lo + 2]
            crop, xt, ok_t = RE.preprocess_frames(rig.det, rig.fan, chunk)
            pts, _, _ = detect_landmarks(rig.det, rig.fan, chunk.permute(0, 3, 1, 2).float(), rule='last_above_0.99', input_range='255')
            _, valid = face_crop.crop_using_landmarks(chunk, pts.contiguous())
            _, boxes, has = detect_landmarks(rig.det, rig.fan, xt, input_range='gan')
            p, ang = shape_params(rig.det, rig.fan, rig.E, xt, boxes=boxes, has_face=has)
            for k, v in p.items():
                params.setdefault(k, []).append(v)
            crops.append(crop), angles.append(ang), oks.append(ok_t & has), valids.append(valid != 0)
    want = RE.TargetAnalysis(torch.cat(crops), {k: torch.cat(v) for k, v in params.items()}, torch.cat(angles), torch.cat(oks),
                             torch.cat(valids), 2)
    print('analyse: ok %s, valid crop %s' % (a.ok.tolist(), a.valid.tolist()))
    assert a.crops.dtype == torch.uint8 and a.crops.shape == (5, 256, 256, 3) and a.ok.dtype == torch.bool
    assert sorted(a.params) == ['alpha_exp', 'alpha_shp', 'cam', 'pose'] and same_analysis(a, want)
    assert not bool((a.ok & ~a.valid).any())                                           # ok implies a valid crop
    joined = RE.TargetAnalysis.cat([r.analyse(rig.small[:4]), r.analyse(rig.small[4:])])
    assert same_analysis(joined, a)
    # through the host and back: the cache of another process
    back = RE.TargetAnalysis.from_dict(a.to('cpu').as_dict()).to('cuda')
    assert same_analysis(back, a) and back.crops.is_cuda


@pytest.mark.parametrize('output', ['video', 'images'])
@pytest.mark.parametrize('on_fail', ['hold', 'source'])
def test_reenact_analysed_equals_reenact(rig, on_fail, output):
    """Three consecutive calls since set_source -- the noise frames (some fail on their own), the faces under a valid mask, two faces
    whose first row reads the carry of the call before -- through reenact and through reenact_analysed: equal bytes, ok and bits."""
    a_r, b_r = with_source(rig, rig.source), with_source(rig, rig.source)
    a_small, a_faces = b_r.analyse(rig.small), b_r.analyse(rig.faces)
    mask = torch.tensor([False, True, False, False, True]).cuda()
    calls = [(rig.small, a_small, None), (rig.faces, a_faces, mask), (rig.faces[:2], a_faces[:2], torch.tensor([False, True]).cuda())]
    for i, (frames, analysis, valid) in enumerate(calls):
        want, want_ok, want_sv = a_r.reenact(frames, valid=valid, on_fail=on_fail, output=output)
        got, ok, sv = b_r.reenact_analysed(analysis, valid=valid, on_fail=on_fail, output=output)
        print('call %d %s/%s: ok %s, %d bytes differ' % (i, on_fail, output, ok.tolist(), int((got != want).sum())))
        assert got.shape == want.shape and got.dtype == torch.uint8 and torch.equal(got, want)
        assert torch.equal(ok, want_ok) and bits(sv, want_sv)
    if on_fail == 'hold':
        assert bits(a_r._carry, b_r._carry) and bool(a_r._carry_valid) == bool(b_r._carry_valid)
        assert bits(sv[0], want_sv[0]) and bool((sv[0] != 0).any())                     # row 0 of the last call took the carried vector
    with pytest.raises(RuntimeError, match=r'rows \[0, 2, 3\]'):
        b_r.reenact_analysed(a_faces, valid=mask, on_fail='raise')
    with pytest.raises(RuntimeError, match='use_source'):
        rig.reenactor().reenact_analysed(a_faces)


def per_source(rig, sources, frames, **kw):
    outs, oks, svs = [], [], []
    for frame in sources:
        out, ok, sv = with_source(rig, frame).reenact(frames, **kw)
        outs.append(out), oks.append(ok), svs.append(sv)
    assert torch.equal(oks[0], oks[1])
    return torch.stack(outs), oks[0], torch.stack(svs)


def test_reenact_many_equals_set_source_and_reenact_per_source(rig):
    """Two sources against four faces (two full chunks each) and against the five noise frames (a partial last chunk each, rows that
    fail): frames, ok and shift vectors equal the stack of two set_source + reenact passes; the Reenactor's own state is untouched."""
    r = rig.reenactor(batch=2)
    sources = [r.make_source(rig.source, optimize=False), r.make_source(rig.source2, optimize=False)]
    assert r.session is None and sources[0].G_source is rig.G and sources[0].loss is None and sources[1].crop.shape == (1, 256, 256, 3)
    for name, frames in (('faces[:4]', rig.faces[:4]), ('small', rig.small)):
        a = r.analyse(frames)
        for kw in ({}, {'on_fail': 'source'}, {'output': 'images'}):
            got, ok, sv = r.reenact_many(sources, a, **kw)
            want, want_ok, want_sv = per_source(rig, [rig.source, rig.source2], frames, **kw)
            print('reenact_many %s %s: ok %s, %d bytes differ' % (name, kw, ok.tolist(), int((got != want).sum())))
            assert got.shape == (2, len(a), 256, 256 if kw.get('output') == 'images' else 768, 3) and torch.equal(got, want)
            assert torch.equal(ok, want_ok) and sv.shape == (2, len(a), D) and bits(sv, want_sv)
        assert not torch.equal(got[0], got[1])
    assert r.session is None and r._carry is None                                      # nothing selected, nothing carried
    got, ok, sv = r.reenact_many(sources, r.analyse(rig.faces[:4]), on_fail='raise')
    assert ok.tolist() == [True] * 4
    with pytest.raises(RuntimeError, match=r'rows \[1\]'):
        r.reenact_many(sources, r.analyse(rig.faces[:4]), valid=torch.tensor([True, False, True, True]).cuda(), on_fail='raise')


def test_reenact_many_with_a_tuned_source_beside_an_untuned_one(rig):
    """make_source(optimize=True, opt_steps=6) beside an un-tuned source: each row of reenact_many equals use_source +
    reenact_analysed on that source, and the base generator is bit-unchanged afterwards."""
    before = {k: v.detach().clone() for k, v in rig.G.state_dict().items()}
    r = rig.reenactor(batch=2, lpips=rig.lpips)
    tuned = r.make_source(rig.source, optimize=True, opt_steps=6)
    plain = r.make_source(rig.source2, optimize=False)
    assert tuned.G_source is not rig.G and plain.G_source is rig.G and bool(torch.isfinite(tuned.loss))
    a = r.analyse(rig.faces[:4])
    valid = torch.tensor([False, True, False, True]).cuda()
    got, ok, sv = r.reenact_many([tuned, plain], a, valid=valid)
    for s, src in enumerate((tuned, plain)):
        r.use_source(src)
        want, want_ok, want_sv = r.reenact_analysed(a, valid=valid)
        print('source %d (%s): %d bytes differ' % (s, 'tuned' if src is tuned else 'plain', int((got[s] != want).sum())))
        assert torch.equal(got[s], want) and torch.equal(ok, want_ok) and bits(sv[s], want_sv)
    assert not torch.equal(got[0, :, :, 512:], with_source(rig, rig.source).reenact(rig.faces[:4], valid=valid)[0][:, :, 512:])   # PTI shows
    after = rig.G.state_dict()
    assert list(after) == list(before) and all(bits(after[k], before[k]) if before[k].dtype == torch.float32 else torch.equal(after[k], before[k])
                                                for k in before)
    assert rig.G.saturated_pairs() == 0


class HeadCalls:
    """Counts the launches of S3FD, FAN and the DECA encoder: each reads its weight pack once per launch."""

    def __init__(self, rig):
        self.heads, self.count = {'det': rig.det, 'fan': rig.fan, 'E': rig.E}, {}

    def __enter__(self):
        for name, head in self.heads.items():
            self.count[name] = 0

            def packed(name=name, inner=head.packed):
                self.count[name] += 1
                return inner()
            head.packed = packed                                                       # an instance attribute over the method
        return self

    def __exit__(self, *exc):
        for head in self.heads.values():
            del head.packed


def test_the_heads_run_once(rig):
    r = with_source(rig, rig.source)
    sources = [r.make_source(rig.source, optimize=False), r.make_source(rig.source2, optimize=False)]
    with HeadCalls(rig) as calls:
        r.reenact(rig.small)
        reenact_calls = dict(calls.count)
    with HeadCalls(rig) as calls:
        a = r.analyse(rig.small)
        analyse_calls = dict(calls.count)
    with HeadCalls(rig) as calls:
        r.reenact_analysed(a)
        r.reenact_analysed(a, on_fail='source', output='images')
        r.reenact_many(sources, a)
        r.reenact_many(sources, a, on_fail='source', output='images')
        render_calls = dict(calls.count)
    print('head launches: reenact %s, analyse %s, reenact_analysed + reenact_many %s' % (reenact_calls, analyse_calls, render_calls))
    assert min(reenact_calls.values()) > 0 and analyse_calls == reenact_calls
    assert render_calls == {'det': 0, 'fan': 0, 'E': 0}
    assert not any('packed' in vars(h) for h in (rig.det, rig.fan, rig.E))


@pytest.fixture(scope='module')
def id_loss():
    from stylegan_directions_face_reenactment_amd.id_loss import IDLoss
    head = IDLoss()
    head.load_state_dict(S.synthetic_arcface_state(SEED))
    return head.cuda().eval()


def test_no_synchronising_torch_call(rig, id_loss):
    """After three warm-up rounds (weight packs, workspaces, graph captures) analyse, reenact_analysed, reenact_many ('hold' and
    'source', both outputs) and cross_metrics run under torch.cuda.set_sync_debug_mode('error'), the harness of
    test_reenact_makes_no_synchronising_torch_call: synchronisations made through torch are seen, the session's wait for each
    chunk's range check is made on the HIP runtime and stays."""
    r = with_source(rig, rig.source)
    sources = [r.make_source(rig.source, optimize=False), r.make_source(rig.source2, optimize=False)]
    valid = torch.tensor([False, True, False, False, True]).cuda()

    def everything():
        a = r.analyse(rig.faces)
        outs = [r.reenact_analysed(a, valid=valid, on_fail=p, output=o) for p in ('hold', 'source') for o in ('video', 'images')]
        many = [r.reenact_many(sources, a, valid=valid, on_fail=p, output=o) for p in ('hold', 'source') for o in ('video', 'images')]
        return a, outs, many, r.cross_metrics(sources, a, many[0][2], id_loss)

    for _ in range(3):
        r.use_source(sources[0])                                                       # (the same carry at the start of every round)
        warm = everything()
    torch.cuda.synchronize()
    probe = torch.ones(1, device='cuda')
    r.use_source(sources[0])
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                                               # the mode is honoured by this build of torch
        got = everything()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert same_analysis(got[0], warm[0])
    for (x, ok_x, sv_x), (y, ok_y, sv_y) in zip(got[1] + got[2], warm[1] + warm[2]):
        assert torch.equal(x, y) and torch.equal(ok_x, ok_y) and bits(sv_x, sv_y)
    assert all(torch.equal(x, y) if x.dtype == torch.bool else bits(x, y) for x, y in zip(got[3], warm[3]))


def test_cross_metrics_are_evaluation_metrics_written_out(rig, id_loss):
    """Two sources x faces[:4] in chunks of 2: csim, pose, exp_error and ok_reenacted against session.frames -> detect_landmarks ->
    shape_params -> train_step.evaluation_metrics written out from public calls on the same chunks."""
    from stylegan_directions_face_reenactment_amd import reenact as RE
    from stylegan_directions_face_reenactment_amd.face_detector import detect_landmarks
    from stylegan_directions_face_reenactment_amd.train_step import evaluation_metrics, shape_params
    r = rig.reenactor(batch=2)
    sources = [r.make_source(rig.source, optimize=False), r.make_source(rig.source2, optimize=False)]
    a = r.analyse(rig.faces[:4])
    _, ok, sv = r.reenact_many(sources, a, output='images')
    csim, pose, exp_error, ok_r = r.cross_metrics(sources, a, sv, id_loss)
    want = [[], [], [], []]
    with torch.no_grad():
        for s, src in enumerate(sources):
            sess = RE.ReenactmentSession(src.G_source, rig.A, src.code, 0.7, rig.trunc, batch=2, shifts=rig.shifts)
            rows = [[], [], [], []]
            for lo, img in zip(range(0, 4, 2), sess.frames(sv[s])):
                _, boxes, has = detect_landmarks(rig.det, rig.fan, img, input_range='gan')
                params, angles = shape_params(rig.det, rig.fan, rig.E, img, boxes=boxes, has_face=has)
                target = {k: v[lo:lo + 2] for k, v in a.params.items()}
                c, p, e = evaluation_metrics(rig.shifts, id_loss, params, target, angles, a.angles[lo:lo + 2], img, src.x)
                for col, v in zip(rows, (c, p, e, a.ok[lo:lo + 2] & has)):
                    col.append(v)
            for col, v in zip(want, rows):
                col.append(torch.cat(v))
    want = [torch.stack(col) for col in want]
    print('cross_metrics: csim %s\n pose %s\n exp_error %s\n ok_reenacted %s' % (csim.tolist(), pose.tolist(), exp_error.tolist(), ok_r.tolist()))
    for got, ref in zip((csim, pose, exp_error), want[:3]):
        assert got.shape == (2, 4) and got.dtype == torch.float32 and bits(got, ref)
    assert ok_r.shape == (2, 4) and ok_r.dtype == torch.bool and torch.equal(ok_r, want[3])
    assert not bool((ok_r & ~a.ok.unsqueeze(0)).any())                                 # a subset of analysis.ok
    assert bool(torch.isfinite(csim).all()) and bool((csim.abs() <= 1 + 1e-5).all()) and bool((pose >= 0).all()) and bool((exp_error >= 0).all())
    assert not bits(csim[0], csim[1])                                                  # two identities


def test_pooled_session_on_a_512_generator_takes_uint8_targets():
    """f = 2, three rows in chunks of 2 and 1: video_frames from the uint8 crops gives the bytes it gives from their float form."""
    from stylegan_directions_face_reenactment_amd.reenact import ReenactmentSession
    G, A = hip_generator(512, 1), direction_matrix()
    w = S.synthetic_latents(SEED, 1, n_latent=G.n_latent, key='reen.512.w').cuda()
    trunc = S.counter_tensor(SEED, 'reen.512.trunc', (1, 512)).cuda()
    sv = S.counter_tensor(SEED, 'reen.512.sv', (3, D), 0.0, 2.0).cuda()
    src = S.counter_tensor(SEED, 'reen.512.src', (1, 3, 256, 256), 0.0, 0.5).clamp_(-1, 1).cuda()
    tgt = crop_bytes((3, 256, 256, 3), 'cross.512.tgt')
    sess = ReenactmentSession(G, A, w, 0.7, trunc, batch=2, pool_to=256)
    want = sess.video_frames(src, as_float_panel(tgt), sv, swap_rb=True)
    got = sess.video_frames(src, tgt, sv, swap_rb=True)
    out = torch.empty(3, 256, 768, 3, dtype=torch.uint8, device='cuda')
    assert sess.video_frames(src, tgt, sv, swap_rb=True, out=out) is out
    print('512 generator pooled to 256: %d bytes differ between uint8 and float targets' % int((got != want).sum()))
    assert got.shape == (3, 256, 768, 3) and torch.equal(got, want) and torch.equal(out, want)
    with pytest.raises(RuntimeError, match='uint8 target crops'):
        sess.video_frames(src, tgt[:2], sv)
    assert G.saturated_pairs() == 0

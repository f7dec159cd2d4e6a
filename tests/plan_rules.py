"""The split-K plan rules and launch lists of csrc/e4e.hip and csrc/s3fd.hip restated in plain Python (no GPU, no library call):
which convs a forward pass launches at a given size, and into how many K slices the host code cuts each of them.  A conv with S > 1
slices runs its epilogue in the finish kernel, one with S = 1 ("whole") in the conv kernel itself, so the number of finish launches
of a pass is the number of launches with S > 1.  tests/test_cpu_e4e_taps.py and tests/test_cpu_s3fd.py pin the geometry to the C
ABI and assert the coverage condition over the cases listed here; tests/test_gpu_s3fd_e4e_plans.py runs those cases and compares
the profiler's launch counts with `e4e_counts` / `s3fd_counts`.  The e4e rules take the head count as an optional parameter (an
encoder for the 512 or 1024 generator has 16 or 18 heads on any input side): tests/test_cpu_e4e_head_plans.py proves what the
cases of E4E_HEADS_SMALL / E4E_HEADS_LARGE reach, tests/test_gpu_e4e_head_plans.py runs them.  `detail_plan` is the same for the one layer kernel of csrc/detail.hip
(sgdfr_detail_upconv_f32): tests/test_cpu_render_seams.py proves what the cases of tests/render_seam_cases.py reach,
tests/test_gpu_render_seams.py runs them."""
from collections import OrderedDict, namedtuple

Launch = namedtuple('Launch', 'cls name G N Ho Wo K')


def _ceil(a, b):
    return -(-a // b)


def _rederive(chunks, S):
    S = max(1, min(S, 32))
    cps = _ceil(chunks, S)
    return _ceil(chunks, cps)


# ---------------------------------------------------------------------------------------------------------------- e4e
E4E_SPLIT_BELOW = 192
E4E_MAX_ROWS = 256


def e4e_slices(B, G, N, Ho, Wo, K):
    """plan_conv of csrc/e4e.hip: 64 x 64 tiles, whole from 192 tiles on, else at most 512 / tiles slices of at least 8 chunks."""
    tiles = _ceil(B * Ho * Wo, 64) * _ceil(N, 64) * G
    chunks = _ceil(K, 16)
    S = 1 if tiles >= E4E_SPLIT_BELOW else min(512 // max(tiles, 1), chunks // 8)
    return _rederive(chunks, S)


def e4e_style_count(R):
    l = 0
    while (2 << l) <= R:
        l += 1                          # floor(log2 R)
    return 2 * l - 2


def e4e_units(R):
    """(cin, depth, stride, h, ho, has shortcut conv) of the 24 units."""
    out, c, h = [], 64, R
    for depth, count in ((64, 3), (128, 4), (256, 14), (512, 3)):
        for k in range(count):
            stride = 2 if k == 0 else 1
            ho = (h - 1) // stride + 1
            out.append((c, depth, stride, h, ho, c != depth))
            c, h = depth, ho
    return out


E4E_MIN_HEADS, E4E_MAX_HEADS = 8, 18


def e4e_heads(R, n=None):
    """The head count: `n` (8..18, the encoder's 2 log2(image_resolution) - 2), by default the side's own."""
    n = e4e_style_count(R) if n is None else n
    assert E4E_MIN_HEADS <= n <= E4E_MAX_HEADS, n
    return n


def e4e_groups(R, n=None):
    """(first head, one past the last, convs per head, side of the input map) of the three head groups of an encoder with n heads."""
    return ((0, 3, 4, R // 16), (3, 7, 5, R // 8), (7, e4e_heads(R, n), 6, R // 4))


def live_taps(side):
    """The filter positions of a 3 x 3 / stride 2 / pad 1 conv on a side x side map that meet the map for some output pixel."""
    so = (side - 1) // 2 + 1
    live = [any(0 <= 2 * o - 1 + k < side for o in range(so)) for k in range(3)]
    return [kh * 3 + kw for kh in range(3) for kw in range(3) if live[kh] and live[kw]]


def e4e_launches(R, n=None):
    """Every e4e_conv_kernel launch of one forward pass of an encoder with n heads at resolution R, in launch order.  K counts the
    live taps only."""
    out = [Launch('stem', 'stem', 1, 64, R, R, 27)]
    for i, (cin, d, stride, h, ho, sc) in enumerate(e4e_units(R)):
        out.append(Launch('conv1', 'u%d.conv1' % i, 1, d, h, h, cin * 9))
        out.append(Launch('conv2_s%d' % stride, 'u%d.conv2' % i, 1, d, ho, ho, d * 9))
        if sc:
            out.append(Launch('shortcut', 'u%d.shortcut' % i, 1, d, ho, ho, cin))
    out.append(Launch('lateral', 'latlayer1', 1, 512, R // 8, R // 8, 256))
    out.append(Launch('lateral', 'latlayer2', 1, 512, R // 4, R // 4, 128))
    for g, (lo, hi, depth, side) in enumerate(e4e_groups(R, n)):
        G = hi - lo
        for k in range(depth):
            so = (side - 1) // 2 + 1
            K = 512 * len(live_taps(side))
            if k == 0:
                out.append(Launch('head_first', 'g%d.k0' % g, 1, G * 512, so, so, K))
            elif k == depth - 1:
                assert so == 1, (R, g, so)
                out.append(Launch('head_last', 'g%d.k%d' % (g, k), G, 512, so, so, K))
            else:
                out.append(Launch('head_grouped' if G > 1 else 'head_single', 'g%d.k%d' % (g, k), G, 512, so, so, K))
            side = so
    out.append(Launch('linear', 'linear', e4e_heads(R, n), 512, 1, 1, 512))
    return out


def e4e_plan(B, R, n=None):
    return [(l, e4e_slices(B, l.G, l.N, l.Ho, l.Wo, l.K)) for l in e4e_launches(R, n)]


def e4e_counts(B, R, n=None):
    """(conv launches, finish launches) of one forward pass."""
    plan = e4e_plan(B, R, n)
    return len(plan), sum(S > 1 for _, S in plan)


E4E_CLASSES = ('stem', 'conv1', 'conv2_s1', 'conv2_s2', 'shortcut', 'lateral', 'head_first', 'head_grouped', 'head_single',
               'head_last', 'linear')
# (class, 'sliced' or 'whole') that no case can show, each with its reason; test_cpu_e4e_taps proves the reasons
E4E_EXCEPTIONS = OrderedDict([
    (('stem', 'sliced'), 'K = 27 is two chunks of 16: never eight chunks per slice, whole at every size'),
])
# the GPU cases of tests/test_gpu_s3fd_e4e_plans.py: (R, B).  Small batches of distinct images at every resolution, then batches
# of repeated rows: (64, 96) and (64, 192) run unit 21's shortcut, the lateral convs, the grouped head convs and (192) the
# EqualLinears whole; (48, 192) runs group 2's single-head convs whole (9 B pixels of a 3 x 3 map: from B = 164 on); (256, 194)
# runs the last head conv whole (7 heads x 8 channel tiles x ceil(B / 64) >= 192 only with 7 heads, i.e. R = 256, and B >= 193).
E4E_SMALL = ((32, 2), (48, 3), (64, 3), (80, 2), (96, 2), (128, 3))
E4E_LARGE = ((64, 96), (64, 192), (48, 192), (256, 194))
# the GPU cases of tests/test_gpu_e4e_head_plans.py: encoders whose head count is not their side's own, (R, n, B).  Small batches of
# distinct images (the encoders of tests/e4e_styles_cases.py; (32, 18, 2) and (80, 16, 3) are its cases d and e):
#   (32, 16, 2)   9 fine heads on the smallest side; d is its 11-head twin
#   (32, 18, 2)   case d: 11 fine heads, every head conv sliced
#   (48, 18, 3)   fine maps 12 -> 6 -> 3 -> 2 -> 1 -> 1, pixel counts off the 64-pixel tile, 11 groups
#   (64, 16, 3)   the first fine conv whole already at B = 3 (N = 4608 on 8 x 8 maps)
#   (64, 14, 2)   7 fine heads: 56 R^2, the last count inside the unit buffer
#   (80, 16, 3)   case e: first fine conv whole on 10 x 10 maps, the second in 3 slices
#   (96, 18, 2)   first fine conv whole, N = 5632 on 12 x 12 maps; the second fine conv in 2 slices
#   (128, 8, 2)   fewer heads than the side's own 12: one fine head, head_single on 16 x 16, 8 x 8, 4 x 4, 2 x 2 input maps
E4E_HEADS_SMALL = ((32, 16, 2), (32, 18, 2), (48, 18, 3), (64, 16, 3), (64, 14, 2), (80, 16, 3), (96, 18, 2), (128, 8, 2))
# batches of repeated rows, (R, n, B) -> (the launches the case is there for, the smallest B at which all of them run whole):
#   (32, 18, 9)    head_first of the fine group whole (11 x 512 channels on 4 x 4 maps)
#   (32, 18, 33)   head_grouped, G = 11, whole on 2 x 2 maps
#   (32, 18, 65)   linear with 18 groups whole; the deeper fine convs drop to 2 slices
#   (32, 18, 129)  every fine conv whole, head_last with 11 groups included: 41 finish launches of 70 convs
#   (32, 16, 129)  the same with G = 9 and 16 linear groups
#   (32, 18, 256)  the API's row limit: the 88 R^2 parked buffers at their largest row count for this side; nothing new runs whole
#   (48, 18, 43)   grouped convs whole on 3 x 3 and 2 x 2 maps with partial pixel tiles (387 = 6 x 64 + 3 and 172 = 2 x 64 + 44
#                  pixels).  They are whole from B = 33 on; 43 is the first B with a seventh pixel tile on the 3 x 3 maps
#   (64, 16, 24)   G = 9 whole on 4 x 4 maps (from B = 9 on), 2 x 2 in 3 slices (B = 17 .. 32)
#   (128, 8, 6)    the single fine head's first conv whole on 16 x 16 maps
#   (256, 18, 3)   the real shape with more than one row: (70, 18) launches, three fine convs whole (the third, on 8 x 8 maps, from 3 rows on)
E4E_HEADS_LARGE = OrderedDict([
    ((32, 18, 9), (('g2.k0',), 9)),
    ((32, 18, 33), (('g2.k1',), 33)),
    ((32, 18, 65), (('linear',), 65)),
    ((32, 18, 129), (('g2.k2', 'g2.k3', 'g2.k4', 'g2.k5'), 129)),
    ((32, 16, 129), (('g2.k2', 'g2.k3', 'g2.k4', 'g2.k5'), 129)),
    ((32, 18, 256), ((), 1)),
    ((48, 18, 43), (('g2.k1', 'g2.k2'), 33)),
    ((64, 16, 24), (('g2.k1',), 9)),
    ((128, 8, 6), (('g2.k0',), 6)),
    ((256, 18, 3), (('g2.k0', 'g2.k1', 'g2.k2'), 3)),
])
E4E_HEAD_CLASSES = ('head_first', 'head_grouped', 'head_last', 'linear')
# (class, 'sliced' or 'whole', groups) that the head-count cases leave to another list, each with its reason
E4E_HEADS_EXCEPTIONS = OrderedDict([
    (('head_single', 'whole', 1), 'a deeper conv of a single fine head runs whole from 24 rows on at R = 128 (8 x 8 maps), at a cost '
                                  'of a 128 x 128 trunk on 24 rows; (48, 192) of E4E_LARGE runs this kernel path whole and stays the witness'),
])


def e4e_head_key(l, S):
    """(class, 'sliced' | 'whole', groups in the launch); for head_first the heads whose channels the one conv holds, N / 512."""
    return (l.cls, 'sliced' if S > 1 else 'whole', l.N // 512 if l.cls == 'head_first' else l.G)


def coverage(plans, classes):
    """{(class, 'sliced' | 'whole')} seen over plans = iterables of (launch, S)."""
    seen = set()
    for plan in plans:
        for l, S in plan:
            assert l.cls in classes, l
            seen.add((l.cls, 'sliced' if S > 1 else 'whole'))
    return seen


# ---------------------------------------------------------------------------------------------------------------- S3FD
# (name, cin, cout, kernel, stride, pad, a pool follows, level fed)
S3FD_NET = (('conv1_1', 3, 64, 3, 1, 1, 0, -1), ('conv1_2', 64, 64, 3, 1, 1, 1, -1), ('conv2_1', 64, 128, 3, 1, 1, 0, -1),
            ('conv2_2', 128, 128, 3, 1, 1, 1, -1), ('conv3_1', 128, 256, 3, 1, 1, 0, -1), ('conv3_2', 256, 256, 3, 1, 1, 0, -1),
            ('conv3_3', 256, 256, 3, 1, 1, 1, 0), ('conv4_1', 256, 512, 3, 1, 1, 0, -1), ('conv4_2', 512, 512, 3, 1, 1, 0, -1),
            ('conv4_3', 512, 512, 3, 1, 1, 1, 1), ('conv5_1', 512, 512, 3, 1, 1, 0, -1), ('conv5_2', 512, 512, 3, 1, 1, 0, -1),
            ('conv5_3', 512, 512, 3, 1, 1, 1, 2), ('fc6', 512, 1024, 3, 1, 3, 0, -1), ('fc7', 1024, 1024, 1, 1, 0, 0, 3),
            ('conv6_1', 1024, 256, 1, 1, 0, 0, -1), ('conv6_2', 256, 512, 3, 2, 1, 0, 4), ('conv7_1', 512, 128, 1, 1, 0, 0, -1),
            ('conv7_2', 128, 256, 3, 2, 1, 0, 5))
S3FD_HEAD_C = (256, 512, 512, 1024, 512, 256)
S3FD_HEAD_CONF = (4, 2, 2, 2, 2, 2)
S3FD_MAX_ROWS = 256
S3FD_MAX_PIXELS = 1 << 24


def s3fd_slices(B, N, Ho, Wo, K, bn):
    """plan_conv of csrc/s3fd.hip: 64-pixel tiles of `bn` channels, at most 512 / tiles slices of at least 8 chunks."""
    tiles = _ceil(B * Ho * Wo, 64) * _ceil(N, bn)
    chunks = _ceil(K, 16)
    return _rederive(chunks, min(512 // max(tiles, 1), chunks // 8))


def s3fd_level_dims(H, W):
    dims, h, w = [None] * 6, H, W
    for _, _, _, ks, stride, pad, pool, level in S3FD_NET:
        h, w = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        if level >= 0:
            dims[level] = (h, w)
        if pool:
            h, w = h // 2, w // 2
    return dims


def s3fd_launches(H, W):
    """(launch, channel tile) of the 25 s3fd_conv_kernel launches of one pass over H x W images, in launch order."""
    out, h, w = [], H, W
    for name, cin, cout, ks, stride, pad, pool, _ in S3FD_NET:
        h, w = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        cls = 'fc6' if pad == 3 else 'stride2' if stride == 2 else 'one' if ks == 1 else 'trunk3_pool' if pool else 'trunk3'
        out.append((Launch(cls, name, 1, cout, h, w, cin * ks * ks), 64))
        if pool:
            h, w = h // 2, w // 2
    for l, (lh, lw) in enumerate(s3fd_level_dims(H, W)):
        out.append((Launch('head_rn' if l < 3 else 'head', 'head%d' % l, 1, S3FD_HEAD_CONF[l] + 4, lh, lw, 9 * S3FD_HEAD_C[l]), 16))
    return out


def s3fd_plan(B, H, W):
    return [(l, s3fd_slices(B, l.N, l.Ho, l.Wo, l.K, bn)) for l, bn in s3fd_launches(H, W)]


def s3fd_counts(B, H, W):
    plan = s3fd_plan(B, H, W)
    return len(plan), sum(S > 1 for _, S in plan)


S3FD_CLASSES = ('trunk3', 'trunk3_pool', 'one', 'stride2', 'fc6', 'head_rn', 'head')
S3FD_EXCEPTIONS = OrderedDict()         # every class runs sliced and whole within 256 rows and 2^24 pixels
# the GPU cases: name -> (B, H, W, subtract_mean, image seeds).  A batch holds the distinct images of its seeds (one image per seed,
# tests/s3fd_restatement.py plan_images), repeated in a permuted order up to B rows.  32 x 32 is the smallest legal image; at 63 x 95
# every pool drops a row and a column, and 47 x 63 (with the mean subtraction) is odd as well; the 128 x 128 batches are the first
# at which conv5_x, fc6, fc7 and the level-0 head (B = 33) and conv6_1 and the level-1 head (B = 65) run whole.  conv6_2 and a head
# without the L2Norm factor run whole only when their own map has more than 256 pixel tiles, i.e. more than 16384 fc7 pixels in
# the batch: the 8 x 8 fc7 map of 128 x 128 would need 257 rows, the 5 x 14 map of a 32 x 320 strip needs 235 (and has few enough
# candidates for a decisive image to exist).  The seeds are the first for which the fp64 restatement's decisions are decisive
# (test_cpu_s3fd.test_plan_cases_are_decisive).
S3FD_CASES = OrderedDict([
    ('tiny', (1, 32, 32, False, (1,))),
    ('odd', (2, 63, 95, False, (2, 3))),
    ('mean', (1, 47, 63, True, (1,))),
    ('b33', (33, 128, 128, False, (101, 153, 203))),
    ('b65', (65, 128, 128, False, (101, 153, 203))),
    ('b240', (240, 32, 320, False, (2, 3))),
])


# ---------------------------------------------------------------------------------------------------------------- the detail layer
DetailPlan = namedtuple('DetailPlan', 'bn Ho Wo M K mt nt chunks asked cps S last ktail')


def detail_plan(rows, cin, cout, h, w, up):
    """launch_conv of csrc/detail.hip for sgdfr_detail_upconv_f32: tile 16 for Cout <= 16, else 64; plan_conv of conv_tile.h on the
    launch's own tiles: at most 512 / tiles slices of at least 8 chunks, at most 32.  `asked` is the slice count the rule asks for,
    S the one it ends with after the chunks per slice are rounded up; `last` the chunks of the last slice, `ktail` the live K rows
    of the last chunk (0: it is full)."""
    f = 2 if up else 1
    Ho, Wo, K = f * h, f * w, 9 * cin
    bn = 16 if cout <= 16 else 64
    M = rows * Ho * Wo
    mt, nt = _ceil(M, 64), _ceil(cout, bn)
    chunks = _ceil(K, 16)
    asked = max(1, min(512 // max(mt * nt, 1), chunks // 8, 32))
    cps = _ceil(chunks, asked)
    S = _ceil(chunks, cps)
    return DetailPlan(bn, Ho, Wo, M, K, mt, nt, chunks, asked, cps, S, chunks - (S - 1) * cps, K % 16)


def detail_counts(rows, cin, cout, h, w, up):
    """(conv launches, finish launches) of one sgdfr_detail_upconv_f32 call."""
    return 1, int(detail_plan(rows, cin, cout, h, w, up).S > 1)


DETAIL_SEAMS = ('uneven_last_slice', 'fewer_slices_than_asked', 'cap_32', 'k_tail_sliced', 'partial_last_channel_tile', 'tile_over_rows',
                'source_side_1')


def detail_seams(rows, cin, cout, h, w, up):
    """Which of DETAIL_SEAMS one launch reaches.  partial_last_channel_tile: a second (or later) channel tile that is partly empty;
    tile_over_rows: some 64-pixel tile holds pixels of two or more rows of the batch; source_side_1 is reported per axis as
    'source_h_1' / 'source_w_1' (the class asks for both over the list)."""
    p = detail_plan(rows, cin, cout, h, w, up)
    HWo = p.Ho * p.Wo
    out = set()
    if p.S > 1 and p.last != p.cps:
        out.add('uneven_last_slice')
    if p.S < p.asked:
        out.add('fewer_slices_than_asked')
    if p.S == 32 and min(512 // (p.mt * p.nt), p.chunks // 8) > 32:
        out.add('cap_32')
    if p.S > 1 and p.ktail:
        out.add('k_tail_sliced')
    if p.nt > 1 and cout % p.bn:
        out.add('partial_last_channel_tile')
    if any(m0 // HWo != min(m0 + 63, p.M - 1) // HWo for m0 in range(0, p.M, 64)):
        out.add('tile_over_rows')
    if h == 1:
        out.add('source_h_1')
    if w == 1:
        out.add('source_w_1')
    return out


def detail_class(rows, cin, cout, h, w, up):
    p = detail_plan(rows, cin, cout, h, w, up)
    return (p.bn, 'up' if up else 'plain', 'sliced' if p.S > 1 else 'whole')


DETAIL_CLASSES = tuple((bn, u, s) for bn in (16, 64) for u in ('up', 'plain') for s in ('whole', 'sliced'))


def batch_rows(B, n):
    """Which distinct image each of B rows holds: every image about B / n times, in an order that is no period of the 64-pixel tile."""
    rows = [(i * 7 + i // n) % n for i in range(B)] if B > n else list(range(B))
    assert set(rows) == set(range(min(B, n)))
    return rows

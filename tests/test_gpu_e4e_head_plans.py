"""GPU: the e4e encoder (csrc/e4e.hip) with the head count apart from the input side, across head counts, sides and batch plans.
The 16- and 18-head encoders of the 512 and 1024 generators put 9 and 11 heads into the fine group: its first conv has 4608 or 5632
output channels, its deeper convs and the EqualLinears run as grouped launches of 9 / 11 and 16 / 18 groups (blockIdx.y = (head,
channel tile), 72 or 88 channel tiles), and its maps size the two parked buffers.  The cases are sizes, nothing else forces a plan:
tests/plan_rules.py restates the split-K rule with the head count as a parameter and lists the cases (E4E_HEADS_SMALL,
E4E_HEADS_LARGE), tests/test_cpu_e4e_head_plans.py proves on the CPU that over them every head launch runs sliced over K (epilogue
in e4e_finish_kernel) and whole (epilogue in e4e_conv_kernel) with 9 and with 11 fine heads, and that the parked buffers hold every
map at every side and head count; here `torch.profiler`'s launch counts must equal the rule's exactly.

Yardstick, from the reference side alone: the fp64 restatement on the CPU (tests/e4e_restatement.py, pinned to the reference's
fixture kat24 for 16 and 18 heads by test_cpu_e4e_styles).  Per tensor the bar is 8 x max |fp32 restatement - fp64 restatement| on
the case's distinct rows, computed here (the project's margin for the same fp32 sum in another order); for (256, 18, 3) 8 x the
fixture's dev_w_f against the reference's codes w_f.  Large batches repeat the distinct rows in plan_rules.batch_rows order: every row
within the bar against its fp64 source, all copies of a row in one launch bit-equal.

Measured on an MI355X, one run; (side, heads, B): ratio to the yardstick, smallest .. largest over the eleven taps and W+; (conv,
finish) launches, planned = observed in every case:
  small  (32, 16, 2) 0.49 .. 1.09 (70, 66)   (32, 18, 2) 0.60 .. 1.14 (70, 66)   (48, 18, 3) 0.73 .. 1.76 (70, 66)
         (64, 16, 3) 0.86 .. 2.45 (70, 64)   (64, 14, 2) 0.63 .. 1.56 (70, 66)   (80, 16, 3) 0.60 .. 2.25 (70, 64)
         (96, 18, 2) 0.84 .. 2.88 (70, 64)   (128, 8, 2) 0.79 .. 1.22 (70, 64)
  large  (32, 18, 9) 0.65 .. 1.40 (70, 65)   (32, 18, 33) 0.65 .. 1.62 (70, 62)   (32, 18, 65) 0.78 .. 1.76 (70, 55)
         (32, 18, 129) 0.89 .. 1.82 (70, 41)   (32, 16, 129) 0.71 .. 2.56 (70, 41)   (32, 18, 256) 0.89 .. 2.27 (70, 14)
         (48, 18, 43) 0.73 .. 2.87 (70, 45)   (64, 16, 24) 0.97 .. 3.19 (70, 46), the largest   (128, 8, 6) 0.82 .. 2.21 (70, 47)
         (256, 18, 3) W+ at 2.22 x the fixture's dev_w_f (70, 18); all copies of a row bit-equal in all ten
  rows   (48, 18) rows [2] 0.65 .. 1.31, [0] 0.66 .. 1.51, [1, 2, 0] 0.73 .. 1.76
  For d = (32, 18, 2) and e = (80, 16, 3) this yardstick equals kat24's dev_* on every tap (1.00 x) except W+ of d, where the
  fixture's dev is 0.60 x this one (5.914e-08 against 9.878e-08).
  wall time of the module: 37 s for the 20 tests; 2.0 .. 5.9 s for each small case (the CPU restatements in fp64 and fp32, once
  per encoder), 3.6 s for (256, 18, 3), under 0.1 s for every other test.
Found and fixed: nothing in the kernels.  Not run: odd head counts (no module can be built with one).

What each test is known to catch, from mutants of csrc/e4e.hip built apart and never committed (values only; each mutant ran once
per module).  `styles` is test_gpu_e4e_styles, `sweep` the e4e tests of test_gpu_s3fd_e4e_plans, both from before this module:
  the grouped bias index without g * in the LeakyReLU epilogue of the head convs, in e4e_conv_kernel only: the large cases (32,
      18, 33), (32, 18, 65), (32, 18, 129), (32, 16, 129), (32, 18, 256), (48, 18, 43), (64, 16, 24) and (256, 18, 3), first at
      h_fine (7.9e4 .. 3.1e6 x); (32, 18, 9), (128, 8, 6) and the eight small cases pass, their grouped convs are sliced or a
      single head.  Earlier: styles: case f alone (its grouped convs on 16 x 16 and 8 x 8 maps run whole at B = 1; W+ only);
      sweep: its four large cases, with at most 7 groups.
  the same in the bias epilogue of the EqualLinears, in e4e_conv_kernel only: (32, 18, 65), (32, 18, 129), (32, 16, 129), (32,
      18, 256), at W+ (5.3e6 .. 6.4e6 x): the cases whose `linear` runs whole, 16 and 18 groups.  Earlier: styles: none (d, e and f slice
      their EqualLinears); sweep: (64, 192), (48, 192), (256, 194), with 10, 8 and 14 groups.
  the last head conv's out_rs 14 x 512 instead of n x 512 (inside the head-vector buffer of max(n, 14) x 512 per row): every
      test but (64, 14, 2): all other small and all large cases, the rows test, and the replay test (part of the head vectors
      stays unwritten, so replay and eager read different leftovers).  Earlier: styles: d and e (taps and rows); f passes (B =
      1); sweep: all six resolutions, three large cases and its replay test; (256, 194) passes (14 heads).
  e4e_wplus_kernel adding w0 of row stride 14 x 512 instead of n x 512: every test but (64, 14, 2) and the replay test.
      Earlier: styles: d and e (taps and rows); sweep: as the line above.
  the group in that LeakyReLU bias index capped at 6 (right up to 7 groups), in e4e_conv_kernel only: the same eight large cases
      as the first line.  Earlier: styles: case f alone; sweep: none (it has at most 7 groups in a head conv).
  the group in the EqualLinears' bias index capped at 13 (right up to 14 groups), in e4e_conv_kernel only: (32, 18, 65), (32,
      18, 129), (32, 16, 129), (32, 18, 256).  Earlier: none: no earlier test runs more than 14 EqualLinear groups whole.
No mutant went uncaught.  The first four are caught by earlier tests too, at the group counts those reach; the last two are wrong
only past them.
"""
import copy

import pytest
import torch

from util import S, golden
import e4e_restatement as RE
import e4e_styles_cases as C
import plan_rules as P
from test_gpu_e4e_hip import _launches as e4e_launches
from test_gpu_s3fd_e4e_plans import _copies_equal, _row_ratios

pytestmark = pytest.mark.gpu

BAR = 8.0
_CASES = {}


def head_case(R, n):
    """Per (side, heads), once per process: the module on the device, the case's distinct images, the fp64 taps of the restatement
    and per tap dev = max |fp32 restatement - fp64 restatement| on the CPU.  Side 256 has no CPU pass: its yardstick is the
    fixture's.  Cases d and e share the encoders of test_gpu_e4e_styles; of the others the device copy alone is kept."""
    if (R, n) not in _CASES:
        name = C.by_side_and_heads()[(R, n)]
        enc, state = C.make_encoder(S, name) if name in C.CASES else C.build_encoder(S, name)
        assert (enc.input_size, enc.style_count) == (R, n)
        x = C.fixture_inputs(S, name)
        taps64, dev = None, None
        if R != 256:
            with torch.no_grad():
                taps64 = RE.forward(state, x.double())
                taps32 = RE.forward(state, x)
            dev = {k: float((taps32[k].double() - taps64[k]).abs().max()) for k in RE.TAPS}
            taps64 = {k: v.cuda() for k, v in taps64.items()}
        _CASES[(R, n)] = (copy.deepcopy(enc).cuda(), x, taps64, dev, name)
    return _CASES[(R, n)]


def _compare(label, got, taps64, rows, dev, kat=None, name=None):
    """Prints per tensor the worst row's ratio to the yardstick and whether all copies of a row are bit-equal, then the smallest and
    largest ratio; returns the first tensor that misses."""
    worst, ratios = None, []
    for k in got:
        assert tuple(got[k].shape[1:]) == tuple(taps64[k].shape[1:]) and got[k].shape[0] == len(rows), k
        ratio = float(_row_ratios(got[k], taps64[k], rows, dev[k]).max())
        same = _copies_equal(got[k], rows)
        fix = ''
        if kat is not None:
            d = float(kat['dev_%s_%s' % (k, name)])
            fix = '   (the fixture\'s dev %.3e = %.2f x this yardstick)' % (d, d / dev[k])
        print('%s tap %-8s %-20s worst row at %.2f x the fp32 restatement\'s deviation %.3e   bar %.0f x; copies of a row bit-equal: %s%s' % (
            label, k, tuple(got[k].shape), ratio, dev[k], BAR, same, fix))
        ratios.append(ratio)
        if not (ratio <= BAR and same) and worst is None:
            worst = (k, ratio, same)
    print('%s ratios %.2f .. %.2f' % (label, min(ratios), max(ratios)))
    return worst


def _counts(label, enc, xb, B, R, n):
    from stylegan_directions_face_reenactment_amd import encoder as E
    want = P.e4e_counts(B, R, n)
    seen = e4e_launches(lambda: E.encode(enc, xb))
    print('%s (conv, finish) launches planned %s observed %s' % (label, want, seen))
    return seen, want


@pytest.mark.parametrize('R,n,B', P.E4E_HEADS_SMALL)
def test_head_counts_against_the_fp64_restatement(R, n, B):
    """Distinct rows, every tap and W+ element by element.  (32, 16): 9 fine heads on the smallest side, (32, 18) its 11-head twin.
    (48, 18): fine maps 12 -> 6 -> 3 -> 2 -> 1 -> 1.  (64, 16), (80, 16), (96, 18): the fine group's first conv whole in front of
    sliced grouped convs.  (64, 14): 7 fine heads, 56 R^2, the last count inside the unit buffer.  (128, 8): fewer heads than the
    side's own 12, the fine group a single head."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, x, taps64, dev, name = head_case(R, n)
    assert x.shape[0] == B
    label = '(%3d, %2d, %3d)' % (R, n, B)
    xc = x.cuda()
    r = E.run_debug(enc, xc)
    got = dict(r['debug'], w=r['w'])
    assert list(got) == list(RE.TAPS)
    for k in RE.TAPS:
        assert tuple(got[k].shape) == tuple(taps64[k].shape), k
    assert tuple(got['h_coarse'].shape) == (B, 3, 512) and tuple(got['h_middle'].shape) == (B, 4, 512)
    assert tuple(got['h_fine'].shape) == (B, n - 7, 512) and tuple(got['w'].shape) == (B, n, 512)
    worst = _compare(label, got, taps64, list(range(B)), dev, golden(C.KAT) if name in C.CASES else None, name)
    assert worst is None, 'first tensor beyond the bar: %s at %.2f x, copies equal %s' % worst
    assert torch.equal(E.encode(enc, xc), r['w'])
    seen, want = _counts(label, enc, xc, B, R, n)
    assert seen == want


@pytest.mark.parametrize('R,n,B', list(P.E4E_HEADS_LARGE))
def test_large_batches_run_the_grouped_epilogues_whole(R, n, B):
    """plan_rules.E4E_HEADS_LARGE says which launch each case runs whole: the fine group's first conv (32, 18, 9), its grouped convs
    (32, 18, 33), (48, 18, 43), (64, 16, 24), the EqualLinears of 18 groups (32, 18, 65), the last head conv with 11 and 9 groups
    (32, 18, 129), (32, 16, 129), the row limit (32, 18, 256), the single fine head's first conv (128, 8, 6), and the real shape
    (256, 18, 3): W+ alone against the reference's codes of the fixture."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, x, taps64, dev, name = head_case(R, n)
    rows = P.batch_rows(B, x.shape[0])
    xb = x[rows].cuda()
    label = '(%3d, %2d, %3d)' % (R, n, B)
    if R == 256:
        kat = golden(C.KAT)
        got = {'w': E.encode(enc, xb)}
        taps64 = {'w': torch.from_numpy(kat['w_' + name]).double().cuda()}
        dev = {'w': float(kat['dev_w_' + name])}
        assert rows == [0] * B and tuple(got['w'].shape) == (B, n, 512)
    else:
        r = E.run_debug(enc, xb)
        got = dict(r['debug'], w=r['w'])
        assert list(got) == list(RE.TAPS) and tuple(got['h_fine'].shape) == (B, n - 7, 512)
        assert torch.equal(E.encode(enc, xb), r['w'])
    worst = _compare(label, got, taps64, rows, dev)
    assert worst is None, 'first tensor beyond the bar or with unequal copies: %s at %.2f x, equal %s' % worst
    seen, want = _counts(label, enc, xb, B, R, n)
    assert seen == want


def test_large_18_head_batch_graph_replay_and_second_stream():
    """(32, 18, 129), every head launch whole: a captured graph's replay and a run on a second stream give the eager bits."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    R, n, B = 32, 18, 129
    assert (R, n, B) in P.E4E_HEADS_LARGE
    enc, x, _, _, _ = head_case(R, n)
    xb = x[P.batch_rows(B, x.shape[0])].cuda()
    eager = E.encode(enc, xb)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.encode(enc, xb)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and float(eager.abs().max()) > 0.1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = E.encode(enc, xb)
    side.synchronize()
    assert torch.equal(other, eager)


def test_rows_of_an_18_head_encoder_are_independent_across_batch_sizes():
    """(48, 18): B = 1 and B = 3 permuted.  Each row of every tap stays within the bar against the fp64 taps of its source."""
    from stylegan_directions_face_reenactment_amd import encoder as E
    enc, x, taps64, dev, _ = head_case(48, 18)
    for rows in ([2], [0], [1, 2, 0]):
        r = E.run_debug(enc, x[rows].cuda())
        got = dict(r['debug'], w=r['w'])
        worst = _compare('(48, 18) rows %-9s' % (rows,), got, taps64, rows, dev)
        assert worst is None, 'first tensor beyond the bar: %s at %.2f x, equal %s' % worst

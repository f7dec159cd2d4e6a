"""CPU: the e4e encoder's head groups with the head count apart from the input side, on the restated rules (tests/plan_rules.py) and
the library's host queries alone.  What the cases of tests/test_gpu_e4e_head_plans.py reach, that the two parked head-map buffers
hold every map written into them at every side and head count the C ABI admits, and that each large case sits where its reason
says it does."""
import plan_rules as P
import e4e_styles_cases as C

SIDES = tuple(range(32, 257, 16))
HEADS = tuple(range(P.E4E_MIN_HEADS, P.E4E_MAX_HEADS + 1))


def _cases():
    return list(P.E4E_HEADS_SMALL) + list(P.E4E_HEADS_LARGE)


def test_the_head_count_defaults_to_the_sides_own():
    """Every call of the rules without a head count keeps its answer, at every side the ABI admits and for the older case lists."""
    for R in SIDES:
        n = P.e4e_style_count(R)
        assert P.e4e_groups(R) == P.e4e_groups(R, n) == ((0, 3, 4, R // 16), (3, 7, 5, R // 8), (7, n, 6, R // 4))
        assert P.e4e_launches(R) == P.e4e_launches(R, n) and len(P.e4e_launches(R)) == 70
        assert P.e4e_launches(R)[-1] == P.Launch('linear', 'linear', n, 512, 1, 1, 512)
        for B in (1, 2, 3, 96, 192, 194):
            assert P.e4e_plan(B, R) == P.e4e_plan(B, R, n) and P.e4e_counts(B, R) == P.e4e_counts(B, R, n)
    # the figures recorded in test_gpu_s3fd_e4e_plans from an MI355X, planned = observed
    assert [P.e4e_counts(B, R) for R, B in P.E4E_SMALL] == [(70, 66), (70, 66), (70, 65), (70, 65), (70, 65), (70, 57)]
    assert [P.e4e_counts(B, R) for R, B in P.E4E_LARGE] == [(70, 12), (70, 9), (70, 10), (70, 2)]
    # the head count moves the fine group and the EqualLinears and nothing else
    for R in (32, 128, 256):
        for n in HEADS:
            ls = P.e4e_launches(R, n)
            assert len(ls) == 70 and [l for l in ls if not l.name.startswith('g2.')][:-1] == \
                [l for l in P.e4e_launches(R) if not l.name.startswith('g2.')][:-1]
            fine = [l for l in ls if l.name.startswith('g2.')]
            assert [l.cls for l in fine] == ['head_first'] + ['head_grouped' if n > 8 else 'head_single'] * 4 + ['head_last']
            assert fine[0].N == 512 * (n - 7) and fine[0].G == 1 and all(l.G == n - 7 and l.N == 512 for l in fine[1:]) and ls[-1].G == n


def test_case_lists_name_encoders_that_exist_and_sizes_the_abi_admits():
    names = C.by_side_and_heads()
    for R, n, B in _cases():
        assert (R, n) in names and C.heads(names[(R, n)]) == n and C.case(names[(R, n)])[1] == R, (R, n)
        assert 1 <= B <= P.E4E_MAX_ROWS and B * R * R <= 1 << 24
    for R, n, B in P.E4E_HEADS_SMALL:
        assert C.case(names[(R, n)])[0] == B, (R, n, B)       # small cases are the encoder's distinct rows
    assert len(set(_cases())) == len(_cases())
    assert [(R, n, B) for R, n, B in P.E4E_HEADS_SMALL if names[(R, n)] in 'de'] == [(32, 18, 2), (80, 16, 3)]
    assert all(n != P.e4e_style_count(R) for R, n, _ in _cases())   # no case is an encoder the older lists could hold
    seeds = [C.case(k)[3] for k in names.values()]
    assert len(set(seeds)) == len(seeds) and len({C.case(k)[4] for k in names.values()}) == len(seeds)


def test_head_count_cases_cover_the_head_launches_sliced_and_whole():
    """The coverage condition.  Every head launch is keyed by (class, sliced or whole, groups in the launch; for head_first the heads
    in its one conv): over the small and large cases together head_first, head_grouped, head_last and linear are seen in both
    states with 9 and with 11 fine heads (16 and 18 groups for linear), head_single sliced on each of the four maps of the 8-head
    case.  What the cases leave to the older list is named in plan_rules.E4E_HEADS_EXCEPTIONS."""
    seen = {}
    for R, n, B in _cases():
        for l, S in P.e4e_plan(B, R, n):
            if l.cls.startswith('head') or l.cls == 'linear':
                seen.setdefault(P.e4e_head_key(l, S), []).append((R, n, B, l.name, l.Ho, S))
    print('%-13s %-7s %6s   first case (R, n, B), launch, output side, slices; cases' % ('class', 'state', 'groups'))
    for key in sorted(seen):
        R, n, B, name, ho, S = seen[key][0]
        print('%-13s %-7s %6d   (%3d, %2d, %3d) %-6s %2d x %-2d S = %-2d   %d' % (key + (R, n, B, name, ho, ho, S, len(seen[key]))))
    for key, why in P.E4E_HEADS_EXCEPTIONS.items():
        print('exception: %s %s with %d group(s): %s' % (key + (why,)))
    want = {(c, how, G + 7 if c == 'linear' else G) for c in P.E4E_HEAD_CLASSES for how in ('sliced', 'whole') for G in (9, 11)}
    assert want <= set(seen), sorted(want - set(seen))
    # the 7 fine heads of the 256 generator on a small side and the single fine head, sliced
    assert {('head_first', 'sliced', 7), ('head_grouped', 'sliced', 7), ('head_last', 'sliced', 7), ('linear', 'sliced', 14)} <= set(seen)
    single = {ho for R, n, B, name, ho, S in seen[('head_single', 'sliced', 1)] if (R, n) == (128, 8)}
    assert single == {8, 4, 2, 1}, single                     # the outputs of the 16 x 16, 8 x 8, 4 x 4 and 2 x 2 input maps
    assert ('head_first', 'whole', 1) in seen and ('head_first', 'sliced', 1) in seen
    # the exception: not reached here, reached by the older list
    assert list(P.E4E_HEADS_EXCEPTIONS) == [('head_single', 'whole', 1)] and not set(P.E4E_HEADS_EXCEPTIONS) & set(seen)
    assert min(B for B in range(1, 257) if all(S == 1 for l, S in P.e4e_plan(B, 128, 8) if l.name == 'g2.k1')) == 24
    assert any(l.cls == 'head_single' and S == 1 for l, S in P.e4e_plan(192, 48)) and (48, 192) in P.E4E_LARGE
    # what the issue found open at the three cases that came with the 16/18-head path: at d and e every deeper fine conv, the last
    # head conv and the EqualLinears are sliced
    for R, n, B in ((32, 18, 2), (80, 16, 3)):
        assert all(S > 1 for l, S in P.e4e_plan(B, R, n) if l.name in ('g2.k1', 'g2.k2', 'g2.k3', 'g2.k4', 'g2.k5', 'linear'))


def test_parked_buffers_hold_every_head_map_at_every_side_and_head_count():
    """The two unit buffers of the trunk hold the head maps behind it (csrc/e4e.hip ws_layout: max(64, 8 (n - 7)) R^2 floats per row
    each).  Every launch that writes there, the first conv of a group and its deeper convs except the last, writes G N Ho Wo floats
    per row; the last conv writes its group's 512-vectors into the head-vector buffer of max(n, 14) x 512 per row.  The workspace
    query reserves exactly two parked buffers and two head-vector buffers of that size for 1, 3 and 256 rows (as far as
    rows R^2 <= 2^24 admits): nothing on the GPU examines a buffer that is too small, this is the place."""
    from stylegan_directions_face_reenactment_amd import _native
    lib = _native.load()

    def align(k):
        return (k + 63) // 64 * 64

    worst, combos = (0.0, None), 0
    for R in SIDES:
        for n in HEADS:
            combos += 1
            room = max(64, 8 * (n - 7)) * R * R
            parked = [(l.G * l.N * l.Ho * l.Wo, l.name) for l in P.e4e_launches(R, n) if l.cls in ('head_first', 'head_grouped', 'head_single')]
            assert len(parked) == 12                          # 3 + 4 + 5 of the 15 head convs; the other three are the last ones
            need, name = max(parked)
            assert need <= room, (R, n, name, need, room)
            assert need == max(64, 8 * (n - 7)) * R * R or n < 15, (R, n, name)        # from 15 heads on the fine group's first conv fills it
            worst = max(worst, (need / room, (R, n, name)))
            last = [l for l in P.e4e_launches(R, n) if l.cls == 'head_last']
            assert sum(l.G * l.N for l in last) == n * 512 <= max(n, 14) * 512 and all(l.Ho == l.Wo == 1 for l in last)
            for rows in (1, 3, 256):
                r2 = rows * R * R
                if r2 > 1 << 24:
                    assert lib.sgdfr_e4e_workspace_bytes_n(rows, R, n) == -1
                    continue
                base = lib.sgdfr_e4e_workspace_bytes(rows, R)  # the side's own count: at most 14 heads, the unit buffers as they are
                vecs = rows * max(n, 14) * 512
                want = base + 4 * (2 * (align(rows * room) - align(64 * r2)) + 2 * (align(vecs) - align(rows * 14 * 512)))
                assert lib.sgdfr_e4e_workspace_bytes_n(rows, R, n) == want, (rows, R, n)
    print('%d (side, heads) combinations: the widest parked map fills its buffer to at most %.3f (%s); the workspace query reserves two '
          'buffers of max(64, 8 (n - 7)) R^2 per row at 1, 3 and 256 rows' % (combos, worst[0], worst[1]))
    assert combos == 165 and worst[0] == 1.0
    # the split-K partials of the cases: S slices of rows x G x N x Ho x Wo floats within the 512 tiles of 64 x 64 set aside for them
    for R, n, B in _cases():
        assert all(S == 1 or S * B * l.G * l.N * l.Ho * l.Wo <= 512 * 64 * 64 for l, S in P.e4e_plan(B, R, n)), (R, n, B)


def test_each_large_head_count_case_sits_where_its_reason_says():
    """Per large case the launches it is there for run whole at its B, and the smallest B at which they all do is the recorded one: the
    case's own B where the case is the first to leave split-K, else the smaller B named in the list's comment."""
    def whole(R, n, B, names):
        return all(S == 1 for l, S in P.e4e_plan(B, R, n) if l.name in names)

    for (R, n, B), (names, first) in P.E4E_HEADS_LARGE.items():
        assert whole(R, n, B, names), (R, n, B)
        assert min(b for b in range(1, B + 1) if whole(R, n, b, names)) == first, (R, n, B)
        assert first == 1 or not whole(R, n, first - 1, names), (R, n, B)
        print('(%3d, %2d, %3d): %-24s whole from B = %3d on; (conv, finish) launches %s' % (
            R, n, B, ' '.join(names) or '-', first, P.e4e_counts(B, R, n)))
    plan = {k: dict((l.name, S) for l, S in P.e4e_plan(k[2], k[0], k[1])) for k in P.E4E_HEADS_LARGE}
    assert [plan[(32, 18, 65)][k] for k in ('g2.k2', 'g2.k3', 'g2.k4', 'g2.k5')] == [2, 2, 2, 2]
    assert P.e4e_counts(129, 32, 18) == P.e4e_counts(129, 32, 16) == (70, 41)
    assert plan[(64, 16, 24)]['g2.k2'] == 3 and plan[(48, 18, 43)]['g2.k3'] > 1
    assert -(-43 * 9 // 64) == 7 and -(-42 * 9 // 64) == 6 and 43 * 9 % 64 and 43 * 4 % 64
    assert P.e4e_counts(3, 256, 18) == (70, 18) and plan[(256, 18, 3)]['g2.k3'] > 1
    # the row limit: everything that can run whole at this side does
    assert plan[(32, 18, 256)] == dict((l.name, S) for l, S in P.e4e_plan(256, 32, 18)) and P.e4e_counts(256, 32, 18) == (70, 14)

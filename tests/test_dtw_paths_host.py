"""CPU only: the mined predecessor-rule fixture (tests/golden/dtw_rules.npz) still tells fastdtw's three rules apart, the two
oracles agree on the pairs that do, and the cases of tests/test_gpu_dtw_paths.py reach every path ``sgnn_dtw_similarity`` can
launch (tests/dtw_cases.py restates the dispatch).  Every comparison is bit for bit; the only thresholds are counts."""
import os

import numpy as np

import dtw_cases as C
from oracle import cbind, fastdtw_restate as FD


def _score(xs, ys, tie):
    xp, xv = cbind.ragged(xs)
    yp, yv = cbind.ragged(ys)
    return cbind.fastdtw_sim(xp, xv, yp, yv, tie)


def test_the_fixture_tells_the_three_rules_apart():
    """Recomputed with the C oracle, every cell's three matrices are the stored ones, and in every cell at least 16 pairs
    differ between rules 1 and 2 and at least 16 between rules 0 and 1 (float32 similarities).  A change of the oracle that
    merges two rules fails here."""
    cells = C.load_rule_cells()
    assert [c.name for c in cells] == ['x%d_%d__y%d_%d' % (xc + yc) for xc in ((3, 12), (13, 20), (21, 32), (33, 70))
                                       for yc in ((34, 65), (66, 97), (98, 130))]
    assert os.path.getsize(C.GOLDEN_RULES) < 100 * 1024
    for c in cells:
        assert 1 <= len(c.xs) <= 128 and 1 <= len(c.ys) <= 8
        assert all(c.x_class[0] <= len(x) <= c.x_class[1] for x in c.xs), c.name
        assert all(c.y_class[0] <= len(y) <= c.y_class[1] for y in c.ys), c.name
        assert {len(y) for y in c.ys} >= set(c.y_class), c.name                  # the class's shortest and longest length
        got = [_score(c.xs, c.ys, t) for t in C.TIES]
        for t in C.TIES:
            assert got[t].dtype == np.float32 and np.array_equal(got[t], c.sims[t]), (c.name, t)
        n12, n01 = int((got[1] != got[2]).sum()), int((got[0] != got[1]).sum())
        print('%-16s rule 1 != rule 2: %3d pairs, rule 0 != rule 1: %3d of %d' % (c.name, n12, n01, got[0].size))
        assert n12 >= C.MIN_RULE_PAIRS and n01 >= C.MIN_RULE_PAIRS, (c.name, n12, n01)


def test_python_and_c_oracle_agree_where_the_rules_differ():
    """oracle.fastdtw_restate.calc_dtw (the definition) equals the C oracle under all three rules on EVERY pair of the fixture
    on which rules 1 and 2 differ or rules 0 and 1 do: the first comparison of the two oracles on pairs where rule 2 is not
    rule 1 (about 2 000 pairs x 3 evaluations of the pure-Python DP, 15 s)."""
    checked = 0
    for c in C.load_rule_cells():
        pairs = np.argwhere((c.sims[1] != c.sims[2]) | (c.sims[0] != c.sims[1]))
        assert int((c.sims[1] != c.sims[2]).sum()) >= 16 and int((c.sims[0] != c.sims[1]).sum()) >= 16, c.name
        for i, j in pairs:
            for t in C.TIES:
                assert np.float32(FD.calc_dtw(c.xs[i], c.ys[j], t)) == c.sims[t][i, j], (c.name, int(i), int(j), t)
        checked += len(pairs)
    print('pairs compared under three rules: %d' % checked)
    assert checked >= 12 * 32


def test_the_dispatch_restatement_at_its_edges():
    """The few numbers the restatement rests on, written out: where the predecessor words leave LDS, which row count an
    instantiation holds, how many levels a pair has, which form a level takes."""
    assert C.words_in_lds(97) and not C.words_in_lds(98) and C.words_in_lds(1)
    assert [C.rmax_of(m) for m in (1, 12, 13, 20, 21, 32)] == [12, 12, 20, 20, 32, 32]
    assert [C.n_levels(*p) for p in ((0, 5), (5, 0), (1, 50), (2, 50), (3, 3), (12, 50), (20, 2), (32, 131))] == [0, 0, 1, 1, 2, 4, 1, 5]
    assert C.pair_labels(12, 65, 0, 65, 12) == {'reg/RMAX12/WLDS1', 'reg/RMAX12/WLDS1/finest/chunks2', 'reg/RMAX12/WLDS1/rm-RH/chunks1',
                                                'reg/RMAX12/WLDS1/rm-R2/chunks1', 'reg/RMAX12/WLDS1/rm-R3/chunks1'}
    assert C.pair_labels(20, 97, 0, 66, 20) == {'reg/RMAX20/WLDS1', 'reg/RMAX20/WLDS1/finest/chunks2', 'reg/RMAX20/WLDS1/pp-lds/chunks1',
                                                'reg/RMAX20/WLDS1/rm-R2/chunks1', 'reg/RMAX20/WLDS1/rm-R3/chunks1'}
    assert C.pair_labels(20, 130, 0, 40, 6) == {'reg/RMAX20/WLDS0', 'reg/RMAX20/WLDS0/finest/chunks1', 'reg/RMAX20/WLDS0/pp-global/chunks1'}
    assert C.pair_labels(32, 131, 0, 131, 5) == {'reg/RMAX32/WLDS0', 'reg/RMAX32/WLDS0/finest/chunks3+', 'reg/RMAX32/WLDS0/coarse32/chunks2'}
    assert C.pair_labels(33, 50, 0, 50, 6) == {'general'} == C.pair_labels(12, 50, 1, 50, 6)
    assert 'reg/empty' in C.pair_labels(12, 50, 0, 0, 6) and 'general/empty' in C.pair_labels(40, 50, 0, 7, 0)


def test_the_gpu_cases_reach_every_path_under_every_rule():
    """The union of the path labels over the calls tests/test_gpu_dtw_paths.py makes holds EVERY label of the dispatch --
    the 6 register instantiations with every form and chunk count their levels can take up to max_y_len 200, the general
    kernel, both grid-stride loops, the six pyramid forms -- under each of the three predecessor rules (the rule is a
    template argument: 18 register instantiations in all), and asks for nothing the restatement does not know."""
    calls = C.all_calls()
    required = C.required_labels()
    assert len(required) == 11 + 6 + 2 * (2 + 4) + 2 * (3 + 2) + (2 + 1) + (3 + 2)
    for tie in C.TIES:
        have = set()
        for name, ties, max_x, max_y, kernel, xl, yl, ordered in calls:
            assert max(xl) <= max_x and max(yl) <= max_y, name       # a call never understates a length
            assert max_y <= 200 and (max_x <= 32 or max_x * max_y <= 70 * 300), name
            if tie in ties:
                have |= C.call_labels(max_x, max_y, kernel, xl, yl, ordered)
        assert not required - have, (tie, sorted(required - have))
        assert not have - required, (tie, sorted(have - required))
    for label in sorted(required):
        print(label)


def test_a_row_against_itself_in_the_oracle():
    """What the GPU file asserts of the kernels holds in the oracle on the sweep's rows: a row against itself has similarity
    exactly 1.  Under rules 1 and 2 that is a theorem (the diagonal wins every tie, on every level), and so it is under rule 0
    for a sorted row (equal means of neighbouring pairs then mean equal entries, so a zero-cost coarse path projects onto
    zero-cost cells).  For an unsorted row under rule 0 it is a fact about these seeded rows only: a coarse path may leave
    the diagonal along a tie of zero costs that the finer level does not share."""
    for max_x in C.SWEEP_MAX_X:
        xs, _ = C.sweep_rows(max_x)
        rows = [x for x in xs if x]
        assert sum(C.sorted_row(x) for x in rows) >= len(rows) // 2 and not all(C.sorted_row(x) for x in rows) or max_x == 1
        for tie in C.TIES:
            assert bool((np.diagonal(_score(rows, rows, tie)) == 1.0).all()), (max_x, tie)

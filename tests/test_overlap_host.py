"""CPU: the reference of tests/overlap_cases.py against an independent formulation (a dense incidence-matrix product), that the
named cases reach every tier and both sides of its bound, the float32 collision the exact order is there for, the threshold's
fraction, the CLI's arguments and lines, and that ``discover.select`` / ``rank_order`` are what they were."""
import inspect
from fractions import Fraction

import numpy as np
import pytest

import overlap_cases as OC


def _dense(sets, width):
    M = np.zeros((len(sets), width), dtype=np.int64)
    for i, s in enumerate(sets):
        M[i, s] = 1
    return M


@pytest.mark.parametrize('name', ['lengths', 'random', 'tiers', 'equal_fractions', 'measures'])
def test_reference_against_incidence_product(name):
    queries, bank = OC.SEARCH_CASES[name]()
    seen = [int(s.max()) for s in bank if len(s)]
    width = max(seen) + 1
    inside = [q[q < width] for q in queries]                           # (an id no row holds shares nothing)
    dense = _dense(inside, width) @ _dense(bank, width).T
    I = OC.intersections(queries, bank)
    assert np.array_equal(I, dense)
    nq = np.array([len(q) for q in queries], dtype=np.float64).reshape(-1, 1)
    nb = np.array([len(b) for b in bank], dtype=np.float64).reshape(1, -1)
    for measure in OC.MEASURES:
        rows, shared, touched, scores = OC.topk(queries, bank, 5, measure, inter=I)
        assert np.array_equal(touched, (dense > 0).sum(1))
        den = {'jaccard': nq + nb - dense, 'containment': nq + 0 * nb, 'coverage': nb + 0 * nq, 'count': 1 + 0 * dense}[measure]
        value = np.where(dense > 0, dense / np.maximum(den, 1), -1.0)
        for qi in range(len(queries)):
            got = rows[qi][rows[qi] >= 0]
            assert len(got) == min(5, touched[qi]) and np.array_equal(shared[qi, :len(got)], dense[qi, got])
            v = value[qi, got]
            assert bool((np.diff(v) <= 1e-12).all())                   # best first, up to float64 rounding of the quotient
            rest = np.setdiff1d(np.flatnonzero(dense[qi] > 0), got)
            if len(rest):
                assert value[qi, rest].max() <= v[-1] + 1e-12
            assert np.allclose(scores[qi, :len(got)], v, rtol=1e-6) and not scores[qi, len(got):].any()


def test_every_tier_and_both_sides_of_its_bound_are_reached():
    queries, bank = OC.tier_case()
    P = [OC.postings_walked(q, bank) for q in queries]
    assert P == [OC.LDS_MAX - 1, OC.LDS_MAX, OC.LDS_MAX + 1]
    assert [OC.tier_of(p) for p in P] == ['lds', 'lds', 'workspace']
    queries, bank = OC.hub_case()
    assert len(bank) == OC.HUB_ROWS and all(0 in b for b in bank)
    assert OC.tier_of(OC.postings_walked(queries[0], bank)) == 'workspace' and OC.tier_of(OC.postings_walked(queries[2], bank)) == 'lds'
    rows, shared, touched, _ = OC.topk(queries[:1], bank, 64, 'jaccard')
    assert touched[0] == OC.HUB_ROWS and int((shared[0] == 1).sum()) >= 32           # most of the best tie on i = 1 ...
    ones = rows[0][shared[0] == 1]
    sizes = [len(bank[b]) for b in ones]
    assert sizes == sorted(sizes) and len(set(sizes)) < len(sizes)                    # ... and go by size, then by row
    assert all(a < b for a, b, sa, sb in zip(ones, ones[1:], sizes, sizes[1:]) if sa == sb)
    queries, bank = OC.lengths_case()
    assert [len(q) for q in queries[:6]] == [0, 1, 2, 63, 64, 65] and any(len(b) == 0 for b in bank)
    assert all(OC.tier_of(OC.postings_walked(q, bank)) == 'lds' for q in queries)
    queries, bank = OC.collision_case()
    assert OC.tier_of(OC.postings_walked(queries[0], bank)) == 'workspace'
    sets = OC.past_lds_sets()
    assert OC.postings_walked(sets[0], sets) > OC.LDS_MAX and OC.tier_of(OC.postings_walked(sets[1], sets)) == 'lds'
    queries, bank = OC.many_case()
    assert len(queries) == OC.MANY > OC.GRID_CAP and all(len(q) == 1 for q in queries)


def test_float32_collision_and_equal_fractions():
    assert np.float32(4095) / np.float32(8191) == np.float32(4096) / np.float32(8193)
    assert Fraction(4095, 8191) < Fraction(4096, 8193)
    queries, bank = OC.collision_case()
    assert (len(queries[0]), len(bank[0]), len(bank[1])) == (6000, 6286, 6289)
    rows, shared, touched, scores = OC.topk(queries, bank, 2, 'jaccard')
    assert rows.tolist() == [[1, 0]] and shared.tolist() == [[4096, 4095]] and touched.tolist() == [2]
    assert scores[0, 0] == scores[0, 1]                                # the numbers returned tie; the order does not
    queries, bank = OC.equal_fractions_case()
    rows, shared, _, _ = OC.topk(queries, bank, 3, 'coverage')
    assert rows.tolist() == [[0, 1, 2]] and shared.tolist() == [[1, 2, 1]]
    assert OC.fraction('coverage', 1, 2, 2) == OC.fraction('coverage', 2, 2, 4) == Fraction(1, 2)
    queries, bank = OC.measures_case()
    order = {m: OC.topk(queries, bank, 3, m)[0][0].tolist() for m in OC.MEASURES}
    assert len({tuple(order[m]) for m in ('jaccard', 'coverage', 'count')}) == 3 and order['containment'] == order['count']
    queries, bank, exclude = OC.touched_case()
    rows, shared, touched, _ = OC.topk(queries, bank, 3, 'jaccard', exclude)
    assert rows.tolist() == [[1, -1, -1], [0, 1, -1], [0, 1, -1]] and touched.tolist() == [2, 2, 2]


def test_greedy_reference_on_the_named_cases():
    half = Fraction(1, 2)
    acc, n, by = OC.greedy(OC.chain_sets(), half, 10)
    assert acc[:n].tolist() == [0, 2] and by.tolist() == [-1, 0, -1]                  # b falls to a, c survives
    acc, n, by = OC.greedy(OC.half_sets(), half, 3)
    assert acc[:n].tolist() == [0, 1] and by.tolist() == [-1, -1, 0]                  # exactly 1/2 is kept, 3/4 is not
    acc, n, by = OC.greedy(OC.degenerate_sets(), Fraction(0), 100)
    assert acc[:n].tolist() == [0, 1, 2, 6] and by.tolist() == [-1, -1, -1, 1, 1, 1, -1]
    sets = OC.ranked_sets()
    acc, n, by = OC.greedy(sets, Fraction(1), 1000)
    assert n == len(sets) and not (by >= 0).any()                                     # tau = 1: nothing is suppressed
    acc, n, by = OC.greedy(sets, Fraction(0), 5)
    assert n == 5 and acc[4] < len(sets) - 1                                          # ``top`` reached mid-list
    acc, n, by = OC.greedy(sets, Fraction(0), 60)
    assert 5 < n < 60 and acc[n:].tolist() == [-1] * (60 - n)                         # ... and never reached
    for i in range(n):
        for j in range(i):
            assert not set(sets[acc[i]].tolist()) & set(sets[acc[j]].tolist())        # tau = 0: any shared node suppresses


def test_threshold_fraction():
    from subgnn_amd import ops
    assert ops.overlap_threshold(0.5) == (1, 2) and ops.overlap_threshold(0) == (0, 1) and ops.overlap_threshold(1.0) == (1, 1)
    assert ops.overlap_threshold(0.1) == (1, 10) and ops.overlap_threshold(1 / 3) == (1, 3)
    for t in (0.0, 0.2, 0.3333, 0.74, 0.999999):
        num, den = ops.overlap_threshold(t)
        f = OC.threshold(t)
        assert (num, den) == (f.numerator, f.denominator) and 0 <= num <= den <= 1 << 20
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            ops.overlap_threshold(bad)
    assert set(ops.OVERLAP_MEASURES) == set(OC.MEASURES)


def test_chunks_cover_the_queries_within_the_budget():
    from subgnn_amd import ops
    P = np.array([10, 3000, 5, 2049, 2048, 9000, 1, 2500], dtype=np.int64)
    assert ops._overlap_chunks(P, OC.LDS_MAX, 1 << 28, None) == [(0, 8)]
    assert ops._overlap_chunks(P[:0], OC.LDS_MAX, 1 << 28, None) == []
    for budget, per in ((6000, None), (100, None), (1 << 28, 3), (5100, 2)):
        chunks = ops._overlap_chunks(P, OC.LDS_MAX, budget, per)
        assert chunks[0][0] == 0 and chunks[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        for lo, hi in chunks:
            big = P[lo:hi][P[lo:hi] > OC.LDS_MAX]
            assert hi > lo and (per is None or hi - lo <= per)
            assert big.sum() <= budget or len(big) == 1                               # (a query beyond the budget goes alone)


def test_cli_arguments_and_lines(tmp_path):
    from subgnn_amd import overlap
    ok = overlap.parse_args([str(tmp_path), '-out', 'o.txt'])
    assert (ok.k, ok.measure, ok.splits, ok.index, ok.subgraphs, ok.summary) == (10, 'jaccard', ('train', 'val', 'test'), None, None, None)
    ok = overlap.parse_args(['-index', 'i.npz', '-out', 'o.txt', '-k', '3', '-measure', 'coverage', '-splits', 'val,train',
                             '-subgraphs', 'r.txt', '-summary', 's.json'])
    assert (ok.k, ok.measure, ok.splits, ok.dataset) == (3, 'coverage', ('val', 'train'), None)
    for bad in (['-out', 'o.txt'], [str(tmp_path), '-index', 'i.npz', '-out', 'o.txt'], [str(tmp_path)],
                [str(tmp_path), '-out', 'o.txt', '-k', '0'], [str(tmp_path), '-out', 'o.txt', '-k', '65'],
                [str(tmp_path), '-out', 'o.txt', '-measure', 'cosine'], [str(tmp_path), '-out', 'o.txt', '-splits', 'train,dev'],
                [str(tmp_path), '-out', 'o.txt', '-splits', 'train,train'], ['-index', 'i.txt', '-out', 'o.txt'],
                [str(tmp_path), '-out', 'o.txt', '-summary', 's.txt'], [str(tmp_path), '-out', 'o.txt', '-subgraphs', 'o.txt']):
        with pytest.raises(SystemExit):
            overlap.parse_args(bad)
    line = overlap.format_line(3, 0, np.float32(4096) / np.float32(8193), 4096, 'val', 7, [5, 2, 9], ['a', 'b'])
    assert line == '3\t0\t0.499938965\t4096\tval\t7\t5-2-9\ta-b'
    assert np.float32(line.split('\t')[2]) == np.float32(4096) / np.float32(8193)     # %.9g: the float32 survives
    assert overlap.format_line(0, 2, 0.0, 0, '', -1, [], []) == '0\t2\t0\t0\t\t-1\t\t'
    assert overlap.HEADER.split('\t') == ['request', 'rank', 'score', 'shared', 'split', 'row', 'subgraph', 'label']


def test_dataset_index_and_discover_arguments(tmp_path):
    from subgnn_amd import discover, overlap
    (tmp_path / 'subgraphs.pth').write_text('3-1-2\tx\ttrain\t\n4-5\ty\ttrain\t\n1-2\tx\tval\t\n7\ty\ttest\t\n8-9\tx\ttest\t\n')
    idx = overlap.index_of_dataset(tmp_path, ('test', 'train'))
    # (read_subgraphs swaps val and test where val is the smaller: the file's one 'val' row is the split 'test')
    assert idx.subgraphs == [[1, 2], [3, 1, 2], [4, 5]] and idx.splits == ['test', 'train', 'train'] and idx.labels[0] == ['x']
    assert set(idx.splits) == {'test', 'train'} and idx.labels[-1] == ['y'] and idx.rows[-2:] == [0, 1] and idx.width == 0
    only = overlap.restrict(idx, ('train',))
    assert only.subgraphs == [[3, 1, 2], [4, 5]] and only.splits == ['train', 'train'] and overlap.restrict(idx, ('train', 'test')) is idx
    sig = inspect.signature(discover.discover).parameters
    assert sig['max_overlap'].default is None and sig['overlap_pool'].default == 4096
    base = ['-config_path', 'c', '-restoreModelPath', 'd', '-seeds', 'all', '-out', 'o']
    a = discover.parse_args(base)
    assert a.max_overlap is None and a.overlap_pool == 4096
    a = discover.parse_args(base + ['-max_overlap', '0.25', '-overlap_pool', '9'])
    assert a.max_overlap == 0.25 and a.overlap_pool == 9
    for bad in (['-max_overlap', '1.5'], ['-max_overlap', '-0.1'], ['-overlap_pool', '0']):
        with pytest.raises(SystemExit):
            discover.parse_args(base + bad)
    assert discover.HEADER == 'rank\tseed\tscore\tscore_std\tprob\tsubgraph\tlabel\tknown'


def test_select_and_rank_order_are_what_they_were():
    """``max_overlap=None`` goes through these two alone, as before: their answers on a list with ties, NaN and several seeds."""
    from subgnn_amd import discover
    score = [0.5, float('nan'), 2.0, 0.5, -1.0, 2.0, 0.5]
    item = [12, 3, 9, 4, 0, 1, 8]
    order = discover.rank_order(score, item)
    assert order.tolist() == [5, 2, 3, 6, 0, 4, 1]
    seed = [q // 4 for q in item]
    assert discover.select(order, seed).tolist() == order.tolist()
    assert discover.select(order, seed, top=3).tolist() == [5, 2, 3]
    assert discover.select(order, seed, top_per_seed=1).tolist() == [5, 2, 3, 0]
    assert discover.select(order, seed, top=2, top_per_seed=1).tolist() == [5, 2]
    assert discover.select([], [], top=3, top_per_seed=2).tolist() == []

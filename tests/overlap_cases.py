"""The definition of the node-overlap search and of the greedy diverse selection (include/subgnn_hip.h: sgnn_overlap_topk /
sgnn_overlap_diverse) in Python ints and numpy, the kernels' dispatch restated (which tier a set takes), and the cases the tests
send through the kernels.  No GPU, no library.

A set is an ascending array of ids >= 0 without repeats; it may be empty.  With i = |q n b| the measures are the fractions
jaccard i / (|q| + |b| - i), containment i / |q|, coverage i / |b|, count i / 1.  A query's result: the bank rows with i >= 1,
the larger fraction first (``fractions.Fraction``: exact), equal fractions by the smaller row, cut at k; fillers -1 / 0."""
from fractions import Fraction

import numpy as np

LDS_MAX = 2048           # csrc/id_table.h SGNN_SET_LDS_MAX (sgnn_overlap_lds_max): postings a set walks with its table in LDS
MAX_K = 64               # csrc/overlap.hip OVL_MAX_K (sgnn_overlap_max_k)
GRID_CAP = 256 * 16      # sgnn_grid_for(n_queries, 1): the workgroups of a launch; more queries take the grid-stride loop
MANY = 9000              # one-node queries of the grid-stride case (as insertion_cases.MANY)
assert MANY > GRID_CAP
MEASURES = ('jaccard', 'containment', 'coverage', 'count')
KS = (1, 2, 64)


def tier_of(P):
    """The home of the counting table of a set that walks P postings.  (There is no one-wavefront tier.)"""
    return 'lds' if P <= LDS_MAX else 'workspace'


def arr(ids):
    return np.asarray(sorted(ids), dtype=np.int32)


def postings_walked(q, bank):
    """P of the set ``q`` against ``bank``: over its members, the number of bank rows that hold the member."""
    held = {}
    for b in bank:
        for v in b.tolist():
            held[v] = held.get(v, 0) + 1
    return sum(held.get(v, 0) for v in q.tolist())


def fraction(measure, i, nq, nb):
    return {'jaccard': lambda: Fraction(i, nq + nb - i), 'containment': lambda: Fraction(i, nq),
            'coverage': lambda: Fraction(i, nb), 'count': lambda: Fraction(i, 1)}[measure]()


def intersections(queries, bank):
    """(Q, B) int64: |q n b| by brute force."""
    bs = [set(b.tolist()) for b in bank]
    out = np.zeros((len(queries), len(bank)), dtype=np.int64)
    for qi, q in enumerate(queries):
        qs = set(q.tolist())
        for bi, b in enumerate(bs):
            out[qi, bi] = len(qs & b)
    return out


def topk(queries, bank, k, measure, exclude=None, inter=None):
    """-> rows (Q, k) int64, inter (Q, k) int32, touched (Q) int32, scores (Q, k) float32 of the definition."""
    I = intersections(queries, bank) if inter is None else inter
    Q = len(queries)
    rows = np.full((Q, k), -1, dtype=np.int64)
    shared = np.zeros((Q, k), dtype=np.int32)
    touched = np.zeros(Q, dtype=np.int32)
    scores = np.zeros((Q, k), dtype=np.float32)
    for qi, q in enumerate(queries):
        met = [b for b in range(len(bank)) if I[qi, b] >= 1]
        touched[qi] = len(met)
        skip = -1 if exclude is None else int(exclude[qi])
        cand = [(-fraction(measure, int(I[qi, b]), len(q), len(bank[b])), b) for b in met if b != skip]
        cand.sort()
        for j, (f, b) in enumerate(cand[:k]):
            rows[qi, j], shared[qi, j] = b, I[qi, b]
            scores[qi, j] = np.float32(np.float64(-f.numerator) / np.float64(f.denominator))
    return rows, shared, touched, scores


def greedy(sets, tau, top):
    """The greedy loop of the header, verbatim; tau a Fraction -> accepted (top) int64 with fillers -1, n, by (N) int32."""
    N = len(sets)
    ss = [set(s.tolist()) for s in sets]
    accepted, by = [], [-1] * N
    for r in range(N):
        if by[r] >= 0:
            continue
        accepted.append(r)
        if len(accepted) == top:
            break
        for c in range(r + 1, N):
            i = len(ss[r] & ss[c])
            if by[c] < 0 and i * tau.denominator > tau.numerator * (len(ss[r]) + len(ss[c]) - i):
                by[c] = r
    out = np.full(top, -1, dtype=np.int64)
    out[:len(accepted)] = accepted
    return out, len(accepted), np.asarray(by, dtype=np.int32).reshape(N)


def threshold(t):
    return Fraction(float(t)).limit_denominator(1 << 20)


# ---------------------------------------------------------------------------------------------------------------- search cases
def _random_sets(rng, n, ids, sizes):
    return [arr(rng.choice(ids, size=int(rng.choice(sizes)), replace=False)) for _ in range(n)]


def lengths_case():
    """Query lengths 0, 1, 2, 63, 64, 65 against 40 random rows (one of them empty) over 300 ids; the last query holds ids the
    bank has never seen, beyond its largest id too."""
    rng = np.random.default_rng(11)
    ids = np.arange(0, 300)
    bank = _random_sets(rng, 40, ids, (1, 2, 5, 17, 40))
    bank[7] = arr([])
    queries = [arr(rng.choice(ids, size=n, replace=False)) for n in (0, 1, 2, 63, 64, 65)]
    queries.append(arr([3, 299, 300, 5000, 2 ** 31 - 1]))
    return queries, bank


def random_case():
    rng = np.random.default_rng(12)
    ids = np.arange(0, 500)
    return _random_sets(rng, 100, ids, (1, 3, 8, 20)), _random_sets(rng, 300, ids, (1, 2, 4, 9, 30))


def tier_case():
    """Three queries that walk LDS_MAX - 1, LDS_MAX and LDS_MAX + 1 postings: ids 0 and 1 are held by all 700 rows, id 2 by the
    first LDS_MAX - 1 - 1400 of them, ids 3 and 4 by one row each; every row has r % 7 ids of its own."""
    B, part = 700, LDS_MAX - 1 - 1400
    bank = []
    for r in range(B):
        ids = [0, 1] + ([2] if r < part else []) + ([3] if r == 5 else []) + ([4] if r == 9 else [])
        bank.append(arr(ids + [1000 + 10 * r + j for j in range(r % 7)]))
    queries = [arr([0, 1, 2]), arr([0, 1, 2, 3]), arr([0, 1, 2, 3, 4])]
    return queries, bank


HUB_ROWS = 5000


def hub_case():
    """Id 0 is held by all HUB_ROWS rows: the query's table, in the workspace, holds 5000 candidates.  Every 50th row also holds
    id 1, three rows id 2; rows have (37 r) % 11 ids of their own, so most rows tie on i = 1 and go by size, then by row."""
    bank = []
    for r in range(HUB_ROWS):
        ids = [0] + ([1] if r % 50 == 0 else []) + ([2] if r in (17, 100, 4999) else [])
        bank.append(arr(ids + [10 + 11 * r + j for j in range((37 * r) % 11)]))
    return [arr([0, 1, 2]), arr([0]), arr([1, 2, 7])], bank


def touched_case():
    """One query that meets exactly two rows, sent three times: with the best row excluded, with a row it does not meet
    excluded, and with -1.  k = 2 is the number of rows met, k = 3 and 64 give fillers."""
    bank = [arr([1, 2]), arr([2, 3, 4]), arr([7, 8]), arr([])]
    queries = [arr([2])] * 3
    return queries, bank, np.asarray([0, 2, -1], dtype=np.int64)


def equal_fractions_case():
    """Under 'coverage' the query {1, 2} gives rows 0 and 2 the fraction 1/2 and row 1 the fraction 2/4: the rows in order."""
    return [arr([1, 2])], [arr([1, 11]), arr([1, 2, 9, 10]), arr([2, 12]), arr([1, 2, 3, 4, 5, 6, 7, 8])]


def collision_case():
    """A 6000-node query; row 0 of 6286 nodes shares 4095 of them, row 1 of 6289 nodes shares 4096: Jaccard 4095/8191 against
    4096/8193, two different numbers that the float32 quotient of float32 operands cannot tell apart."""
    q = np.arange(0, 6000, dtype=np.int32)
    row0 = np.concatenate([np.arange(0, 4095), np.arange(10000, 10000 + 6286 - 4095)]).astype(np.int32)
    row1 = np.concatenate([np.arange(0, 4096), np.arange(20000, 20000 + 6289 - 4096)]).astype(np.int32)
    return [q], [row0, row1]


def measures_case():
    """One query and three rows that 'jaccard', 'coverage' and 'count' order in three different ways ('containment' divides
    the count by |q|, the same for all rows of a query: its order is that of 'count', its scores are not)."""
    q = arr(range(1, 7))
    return [q], [arr([1, 2, 3, 4] + list(range(200, 220))), arr([1, 2]), arr([1, 2, 3, 100])]


def many_case():
    """MANY one-node queries against 60 random rows over 200 ids; every query id is i % 220, so some meet nothing."""
    rng = np.random.default_rng(13)
    bank = _random_sets(rng, 60, np.arange(0, 200), (1, 4, 12))
    return [arr([i % 220]) for i in range(MANY)], bank


SEARCH_CASES = {'lengths': lengths_case, 'random': random_case, 'tiers': tier_case, 'hub': hub_case,
                'equal_fractions': equal_fractions_case, 'collision': collision_case, 'measures': measures_case}


# --------------------------------------------------------------------------------------------------------------- diverse cases
def chain_sets():
    """a ~ b, b ~ c, not a ~ c at tau = 1/2: b falls to a, so c survives."""
    return [arr([1, 2, 3, 4]), arr([2, 3, 4, 5]), arr([3, 4, 5, 6])]


def half_sets():
    """Rows 0 and 1 share 2 of 4 ids: exactly 1/2, which tau = 1/2 keeps (the test is '>'); rows 0 and 2 share 3 of 4."""
    return [arr([1, 2, 3]), arr([2, 3, 4]), arr([1, 2, 3, 9])]


def degenerate_sets():
    """Empty sets (an empty union is never too similar) and duplicates (Jaccard 1: suppressed by every tau < 1)."""
    return [arr([]), arr([5, 6]), arr([]), arr([5, 6]), arr([6]), arr([5, 6]), arr([])]


def ranked_sets():
    """60 random sets over 40 ids: many overlaps, so that ``top`` is reached mid-list at some thresholds and never at others."""
    return _random_sets(np.random.default_rng(14), 60, np.arange(0, 40), (1, 2, 3, 5, 8))


def past_lds_sets():
    """Row 0 holds 30 ids, each of which 80 further rows hold: it walks 30 * 81 postings, past the LDS tier.  Of the further
    rows, those of one id share 1/30 with it, those of four ids 4/30."""
    big = list(range(30))
    sets = [arr(big)]
    for j in range(30 * 80):
        v = j % 30
        sets.append(arr([v]) if j % 3 else arr([v, (v + 1) % 30, (v + 2) % 30, (v + 3) % 30]))
    return sets


DIVERSE_CASES = {           # name -> (sets, thresholds, tops)
    'chain': (chain_sets, (0.0, 0.5, 1.0), (1, 2, 3, 10)),
    'half': (half_sets, (0.0, 0.5, 0.74, 0.75, 1.0), (3,)),
    'degenerate': (degenerate_sets, (0.0, 0.5, 1.0), (2, 7, 100)),
    'ranked': (ranked_sets, (0.0, 0.2, 0.5, 1.0), (1, 5, 20, 60, 1000)),
    'past_lds': (past_lds_sets, (0.1, 0.0), (5000,)),
}

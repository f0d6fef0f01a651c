"""Nearest rows (sgnn_topk_rows, ops.topk_rows): the reference in numpy, the cases and a restatement of the dispatch.

``topk_ref`` evaluates the float32 definition of include/subgnn_hip.h literally: dot(i, j) is the chain acc = fmaf(q[i][d],
bank[j][d], acc) over ascending d from 0 -- each product-and-add formed in float64 (the product of two float32 is exact there)
and rounded to float32 -- then the metric's epilogue in float32, one rounding per operation, then a stable sort by
(score, index) with NaN behind every number and fillers (-1, -inf; +inf for l2) behind everything.

The bit-for-bit cases draw from the DYADIC grid: integers in [-8, 8] scaled by 2^-3.  Every product is a multiple of 2^-6 of
magnitude <= 1, so every partial sum over D <= 130 columns is a multiple of 2^-6 below 2^8: exact in float32 in any order.  The
squared norms of l2 are exact for the same reason, and so are (qa + ba) and 2 dot and their difference.
"""
import numpy as np

METRIC_CODE = {'dot': 0, 'cosine': 1, 'l2': 2}
MAX_K = 64
TQ, TB, KC = 32, 128, 32                  # csrc/neighbors.hip: queries per workgroup, bank rows per tile, columns per chunk
WANT_BLOCKS, MAX_SPLITS = 1024, 1024


# ---------------------------------------------------------------------- reference ---------
def dot_chain_f32(q, bank, reverse=False):
    """(Q, N) float32: the fmaf chain over d (descending d if ``reverse``)."""
    q, bank = np.asarray(q, dtype=np.float32), np.asarray(bank, dtype=np.float32)
    acc = np.zeros((q.shape[0], bank.shape[0]), dtype=np.float32)
    order = range(q.shape[1] - 1, -1, -1) if reverse else range(q.shape[1])
    with np.errstate(invalid='ignore', over='ignore'):
        for d in order:
            acc = (acc.astype(np.float64) + q[:, d, None].astype(np.float64) * bank[None, :, d].astype(np.float64)).astype(np.float32)
    return acc


def aux_f32(x, metric):
    """What ops.topk_aux forms, in float32 (exact on the dyadic grid; elsewhere the device's sum may round differently)."""
    if metric == 'dot':
        return None
    x = np.asarray(x, dtype=np.float32)
    sq = (x * x).sum(axis=1, dtype=np.float32)
    return (np.float32(1) / np.sqrt(np.maximum(sq, np.float32(1e-30)))).astype(np.float32) if metric == 'cosine' else sq


def scores_f32(q, bank, metric, q_aux=None, b_aux=None):
    dot = dot_chain_f32(q, bank)
    if metric == 'dot':
        return dot
    qa = np.asarray(aux_f32(q, metric) if q_aux is None else q_aux, dtype=np.float32)[:, None]
    ba = np.asarray(aux_f32(bank, metric) if b_aux is None else b_aux, dtype=np.float32)[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        if metric == 'cosine':
            return ((dot * qa).astype(np.float32) * ba).astype(np.float32)
        return ((qa + ba).astype(np.float32) - (np.float32(2) * dot).astype(np.float32)).astype(np.float32)


def order_rows(scores, metric, exclude=None):
    """Per query the bank rows in the total order (excluded row left out) -> list of int64 arrays."""
    scores = np.asarray(scores)
    out = []
    for i in range(scores.shape[0]):
        s = scores[i].astype(np.float64)
        idx = np.arange(s.shape[0], dtype=np.int64)
        nan = np.isnan(s)
        key = np.where(nan, 0.0, s if metric == 'l2' else -s) + 0.0            # -0 == +0 either way
        o = np.lexsort((idx, key, nan))                                          # last key first: numbers, then score, then row
        if exclude is not None and exclude[i] >= 0:
            o = o[o != exclude[i]]
        out.append(o)
    return out


def select(scores, k, metric, exclude=None):
    """(scores (Q, k) of ``scores``' dtype, indices (Q, k) int64) with fillers."""
    scores = np.asarray(scores)
    Q = scores.shape[0]
    fill = np.inf if metric == 'l2' else -np.inf
    out_s = np.full((Q, k), fill, dtype=scores.dtype)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for i, o in enumerate(order_rows(scores, metric, exclude)):
        o = o[:k]
        out_s[i, :len(o)] = scores[i, o]
        out_i[i, :len(o)] = o
    return out_s, out_i


def topk_ref(q, bank, k, metric, exclude=None, q_aux=None, b_aux=None):
    return select(scores_f32(q, bank, metric, q_aux, b_aux), k, metric, exclude)


def scores_f64(q, bank, metric):
    """(Q, N) float64: the metric of the float32 inputs evaluated in float64 (cosine by the true norms, floored like the
    float32 ones; l2 as the squared distance)."""
    q, bank = np.asarray(q, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    dot = q @ bank.T
    if metric == 'dot':
        return dot
    qs, bs = (q * q).sum(1), (bank * bank).sum(1)
    if metric == 'cosine':
        return dot / np.sqrt(np.maximum(qs, 1e-30))[:, None] / np.sqrt(np.maximum(bs, 1e-30))[None, :]
    return qs[:, None] + bs[None, :] - 2.0 * dot


def tolerance(q, bank, metric):
    """(Q, N) float64, per pair: gamma * sum_d |q_d b_d| with gamma = (D + 2) u / (1 - (D + 2) u), u = 2^-24 -- the standard
    bound of a length-D fma chain plus the two roundings of the epilogue.  cosine: times the two inverse norms.  l2: doubled
    (the score holds 2 dot), plus the same gamma on each of the three squared-norm terms: |q|^2, |b|^2 (their float32 sums) and
    their float32 sum |q|^2 + |b|^2."""
    q, bank = np.asarray(q, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    D = q.shape[1]
    u = 2.0 ** -24
    gamma = (D + 2) * u / (1.0 - (D + 2) * u)
    t = gamma * (np.abs(q) @ np.abs(bank).T)
    if metric == 'dot':
        return t
    qs, bs = (q * q).sum(1), (bank * bank).sum(1)
    if metric == 'cosine':
        return t / np.sqrt(np.maximum(qs, 1e-30))[:, None] / np.sqrt(np.maximum(bs, 1e-30))[None, :]
    return 2.0 * t + gamma * (qs[:, None] + bs[None, :] + (qs[:, None] + bs[None, :]))


# ---------------------------------------------------------------------- inputs ------------
def dyadic(rng, rows, cols):
    return (rng.integers(-8, 9, size=(rows, cols)).astype(np.float32) / np.float32(8)).astype(np.float32)


def make_inputs(case, seed_base=20240):
    """(q, bank) of a case: dyadic grids, or float32 normals for ``case['data'] == 'normal'``."""
    rng = np.random.default_rng(seed_base + case['Q'] * 7 + case['N'] * 11 + case['D'] * 13 + case['k'])
    if case.get('data', 'dyadic') == 'dyadic':
        return dyadic(rng, case['Q'], case['D']), dyadic(rng, case['N'], case['D'])
    return (rng.standard_normal((case['Q'], case['D'])).astype(np.float32),
            rng.standard_normal((case['N'], case['D'])).astype(np.float32))


# ---------------------------------------------------------------------- dispatch ----------
def geometry(Q, N, splits):
    """(bank tiles, tiles per slice, slices) as tk_geometry of csrc/neighbors.hip picks them."""
    nq, nt = -(-Q // TQ), -(-N // TB)
    if splits <= 0:
        s = max(1, min(-(-WANT_BLOCKS // nq), nt, MAX_SPLITS))
        per = max(1, -(-nt // s))
        s = max(1, -(-nt // per))
    else:
        s, per = splits, max(1, -(-nt // splits))
    return nt, per, s


def branches(Q, N, D, k, splits, exclude=False):
    """The names of the branches a call takes."""
    nt, per, s = geometry(Q, N, splits)
    b = {'splits_auto' if splits <= 0 else 'splits_forced', 'direct' if s == 1 else 'merge'}
    b.add('no_tiles' if nt == 0 else ('one_tile_per_slice' if per == 1 else 'many_tiles_per_slice'))
    if s * per > nt and nt > 0:
        b.add('empty_slice')
    if nt > 0 and (nt - 1) // per + 1 >= 2:
        b.add('two_filled_slices')
    if N % TB:
        b.add('row_tail')
    if N >= TB:
        b.add('full_tile')
    b.add('q_tail' if Q % TQ else 'q_exact')
    if Q > TQ:
        b.add('many_q_tiles')
    if D % 2:
        b.add('d_odd')                     # the last MFMA k-step is half padding
    b.add('d_tail' if D % KC else 'd_exact')
    if D > KC:
        b.add('many_chunks')
    if N - (1 if exclude and N > 0 else 0) < k:
        b.add('fillers')
    if k == MAX_K:
        b.add('k_max')
    if k == 1:
        b.add('k_one')
    if exclude:
        b.add('exclude')
    return b


ALL_BRANCHES = {'splits_auto', 'splits_forced', 'direct', 'merge', 'no_tiles', 'one_tile_per_slice', 'many_tiles_per_slice',
                'empty_slice', 'two_filled_slices', 'row_tail', 'full_tile', 'q_tail', 'q_exact', 'many_q_tiles', 'd_odd', 'd_tail',
                'd_exact', 'many_chunks', 'fillers', 'k_max', 'k_one', 'exclude'}

QS, NS, DS, KS, SPLITS = (1, 31, 32, 33, 65), (1, 31, 32, 33, 64, 65, 1000), (1, 2, 3, 4, 31, 33, 130), (1, 2, 63, 64), (0, 1, 2, 7)


def _case(Q=33, N=65, D=4, k=2, splits=0, **kw):
    return dict(Q=Q, N=N, D=D, k=k, splits=splits, **kw)


def exact_cases():
    """Each edge of each dimension beside plain values of the others (both metrics run every case)."""
    cases = [_case(Q=Q, N=1000, D=33) for Q in QS]
    cases += [_case(N=N) for N in NS]
    cases += [_case(D=D) for D in DS]
    cases += [_case(N=1000, k=k, splits=2) for k in KS]
    cases += [_case(N=1000, D=31, k=63, splits=s) for s in SPLITS]
    cases += [_case(Q=64, N=256, D=64, k=64, splits=1),        # no tail anywhere
              _case(Q=1, N=1000, D=130, k=64, splits=7)]       # the one-query form the library slices most
    seen, out = set(), []
    for c in cases:
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


EDGE_CASES = [_case(Q=3, N=0, D=5, k=4), _case(Q=5, N=3, D=5, k=4), _case(Q=33, N=64, D=7, k=64, exclude=True)]
RANDOM_CASE = _case(Q=65, N=1000, D=130, k=64, data='normal')


def case_id(c):
    return 'Q%d-N%d-D%d-k%d-s%d' % (c['Q'], c['N'], c['D'], c['k'], c['splits'])

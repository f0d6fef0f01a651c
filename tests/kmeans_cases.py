"""k-means (sgnn_kmeans_step / sgnn_kmeans_finish, ops.kmeans_step, ops.kmeans): the reference in numpy, the cases, the
tolerances and a restatement of the dispatch.

The score of (row, centre), the total order and the score tolerance are those of tests/neighbors_cases.py (the kernel's
assignment IS topk_rows with k = 1).  ``step_ref`` evaluates the rest of include/subgnn_hip.h's definition literally: per slot
and cluster the float32 chain over the slot's rows in ascending order, the slots added in slot order, one rounded division.

The bit-for-bit cases draw from the DYADIC grid of neighbors_cases: multiples of 2^-3 in [-1, 1].  A sum of n <= 2^20 such
values is a multiple of 2^-3 below 2^20: exact in float32 in ANY order (23 bits), so sums, counts and the float64 inertia do not
depend on the slot geometry, and the division by the count is the only rounding of a step.
"""
import numpy as np

import neighbors_cases as NC

TR, TC, KC = 32, 128, 32                  # csrc/kmeans.hip: rows per tile, centres per tile, columns per staged chunk
MAX_K, MAX_SLOTS, PART_CAP = 1024, 1024, 64 << 20
RB, ACC_BYTES, THREADS = 64, 32 << 10, 256
U = 2.0 ** -24


# ---------------------------------------------------------------------- dispatch ----------
def geometry(N, K, D):
    """(row tiles, tiles per slot, slots, accumulator columns W) as km_geometry of csrc/kmeans.hip picks them."""
    nt = -(-N // TR)
    s = max(1, min(PART_CAP // (K * D * 4), MAX_SLOTS, nt))
    per = -(-nt // s)
    W = 32 if K * 32 * 4 <= ACC_BYTES else (16 if K * 16 * 4 <= ACC_BYTES else 8)
    return nt, per, -(-nt // per), W


def workspace_bytes(N, K, D):
    S = geometry(N, K, D)[2]
    return S * 8 + S * K * D * 4 + S * K * 4 + S * 4


def slot_rows(N, K, D):
    """[(first row, end row)] of every slot."""
    nt, per, S, _ = geometry(N, K, D)
    return [(s * per * TR, min(N, (s + 1) * per * TR)) for s in range(S)]


def branches(N, K, D, prev=False):
    nt, per, S, W = geometry(N, K, D)
    b = {'one_slot' if S == 1 else 'many_slots', 'one_tile_per_slot' if per == 1 else 'many_tiles_per_slot',
         'w%d' % W, 'prev' if prev else 'no_prev'}
    if nt > MAX_SLOTS and PART_CAP // (K * D * 4) >= MAX_SLOTS:
        b.add('slots_capped_by_count')
    if PART_CAP // (K * D * 4) < min(nt, MAX_SLOTS):
        b.add('slots_capped_by_bytes')
    if S > 1 and nt - (S - 1) * per < per:
        b.add('last_slot_fewer_tiles')
    b.add('row_tail' if N % TR else 'row_exact')
    b.add('one_centre_tile' if K <= TC else 'many_centre_tiles')
    if K % TC:
        b.add('centre_tail')
    if K == 1:
        b.add('one_centre')
    if N < K:
        b.add('empty_certain')
    if D % 2:
        b.add('d_odd')
    b.add('d_tail' if D % KC else 'd_exact')
    if D > KC:
        b.add('many_staged_chunks')
    if D > W:
        b.add('many_column_chunks')
    if D % W:
        b.add('column_chunk_tail')
    rows = [hi - lo for lo, hi in slot_rows(N, K, D)]
    if max(rows) > RB:
        b.add('many_row_blocks')
    if any(r % RB for r in rows):
        b.add('row_block_tail')
    return b


ALL_BRANCHES = {'one_slot', 'many_slots', 'one_tile_per_slot', 'many_tiles_per_slot', 'w32', 'w16', 'w8', 'prev', 'no_prev',
                'slots_capped_by_count', 'slots_capped_by_bytes', 'last_slot_fewer_tiles', 'row_tail', 'row_exact',
                'one_centre_tile', 'many_centre_tiles', 'centre_tail', 'one_centre', 'empty_certain', 'd_odd', 'd_tail',
                'd_exact', 'many_staged_chunks', 'many_column_chunks', 'column_chunk_tail', 'many_row_blocks', 'row_block_tail'}

NS, KS, DS = (1, 31, 32, 33, 1000, 65605), (1, 2, 33, 129, 300), (1, 31, 32, 33, 130)
# 129 tiles, at most 126 slots by the byte cap -> 65 slots of two tiles; W = 8; eight centre tiles
BIG = dict(N=4100, K=1024, D=130, prev=True)


def _case(N=200, K=7, D=9, prev=False):
    return dict(N=N, K=K, D=D, prev=prev)


def exact_cases():
    """Each edge of each dimension beside plain values of the others (both metrics run every case)."""
    cases = [_case(N=N, prev=N in (33, 65605)) for N in NS] + [_case(K=K, prev=K == 33) for K in KS] + [_case(D=D) for D in DS]
    cases += [_case(N=256, K=128, D=64, prev=True), dict(BIG)]
    return cases


def case_id(c):
    return 'N%d-K%d-D%d%s' % (c['N'], c['K'], c['D'], '-prev' if c['prev'] else '')


def make_inputs(case, seed_base=31000):
    """(X, C, prev or None): dyadic grids; prev = random clusters (int32)."""
    rng = np.random.default_rng(seed_base + case['N'] * 7 + case['K'] * 11 + case['D'] * 13)
    X, C = NC.dyadic(rng, case['N'], case['D']), NC.dyadic(rng, case['K'], case['D'])
    prev = rng.integers(0, case['K'], size=case['N']).astype(np.int32) if case['prev'] else None
    return X, C, prev


RANDOM_CASE = dict(N=1000, K=7, D=130, prev=False)


def random_inputs():
    rng = np.random.default_rng(777)
    return (rng.standard_normal((RANDOM_CASE['N'], RANDOM_CASE['D'])).astype(np.float32),
            rng.standard_normal((RANDOM_CASE['K'], RANDOM_CASE['D'])).astype(np.float32))


# ---------------------------------------------------------------------- reference ---------
def assign_ref(X, C, metric, x_aux=None, c_aux=None):
    """(assign int32 (N), score float32 (N)): neighbors_cases.topk_ref with k = 1."""
    s, i = NC.topk_ref(X, C, 1, metric, q_aux=x_aux, b_aux=c_aux)
    return i[:, 0].astype(np.int32), s[:, 0]


def sums_f32(X, assign, K, slots, reverse=False):
    """(K, D) float32 as the kernels form it: per slot the chain over its rows (ascending; descending if ``reverse``), then the
    chain over the slots' partials (in slot order; reversed likewise)."""
    X = np.asarray(X, dtype=np.float32)
    total = np.zeros((K, X.shape[1]), dtype=np.float32)
    for lo, hi in (slots[::-1] if reverse else slots):
        part = np.zeros_like(total)
        for i in (range(hi - 1, lo - 1, -1) if reverse else range(lo, hi)):
            part[assign[i]] = part[assign[i]] + X[i]                 # float32 + float32 -> one rounding
        total = total + part
    return total


def sums_f64(X, assign, K):
    out = np.zeros((K, np.asarray(X).shape[1]), dtype=np.float64)
    np.add.at(out, np.asarray(assign, dtype=np.int64), np.asarray(X, dtype=np.float64))
    return out


def step_ref(X, C, assign, score, prev, slots):
    """dict of what a step returns beside assign and score, from the definition."""
    K = C.shape[0]
    sums = sums_f32(X, assign, K, slots)
    counts = np.bincount(assign, minlength=K).astype(np.int32)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = (sums / counts.astype(np.float32)[:, None]).astype(np.float32)          # float32 / float32: correctly rounded
    centers = np.where(counts[:, None] > 0, mean, np.asarray(C, dtype=np.float32))
    return {'sums': sums, 'counts': counts, 'centers': centers, 'empty': int((counts == 0).sum()),
            'inertia': float(np.sum(score.astype(np.float64))),
            'changed': int(len(assign) if prev is None else (np.asarray(prev) != assign).sum())}


def gamma(n):
    return n * U / (1.0 - n * U)


def sums_tolerance(X, assign, K, n_slots):
    """(K, D) float64: gamma_m * sum_{i in k} |x_i|, m = n_k + S.  A row's value passes through at most n_k - 1 additions of
    its slot's chain (gamma_n of the issue, n the cluster's size) and at most S additions of the chain over the S slots'
    partials (the partial-order term); the standard bound of a summation whose longest path has m additions."""
    n = np.bincount(assign, minlength=K).astype(np.float64)
    return gamma(n + n_slots)[:, None] * sums_f64(np.abs(np.asarray(X, dtype=np.float64)), assign, K)


def centers_tolerance(X, assign, K, n_slots, centers):
    """(K, D) float64: the sums' bound divided by the count, plus the division's rounding u |c| (times 1 + the sums' relative
    bound, absorbed by rounding u up to 2^-23 there).  Clusters without rows: 0 (the centre is copied)."""
    n = np.bincount(assign, minlength=K).astype(np.float64)
    t = sums_tolerance(X, assign, K, n_slots) / np.maximum(n, 1)[:, None] + 2 * U * np.abs(centers)
    return np.where(n[:, None] > 0, t, 0.0)


def aux_tolerance(D):
    """Relative bound of a c_aux entry: D fmaf + 8 tree additions (+ sqrt and division for cosine, whose halved exponent only
    helps): (D + 12) u."""
    return (D + 12) * U


# ---------------------------------------------------------------------- initialisation ----
def l2_to_row_f32(X, r):
    """max(float32 l2 score of every row to row r, 0) as float64: what ops.kmeans_init_rows reads from topk_rows."""
    return np.maximum(NC.scores_f32(X, X[r:r + 1], 'l2')[:, 0], np.float32(0)).astype(np.float64)


def init_rows(X, K, init, seed, dist=l2_to_row_f32):
    """The restatement of ops.kmeans' initialisation in numpy."""
    N = X.shape[0]
    rng = np.random.default_rng(seed)
    if init == 'random':
        return [int(r) for r in rng.choice(N, K, replace=False)]
    u = rng.random(K)
    picks = [min(int(np.floor(u[0] * N)), N - 1)]
    d2 = np.full(N, np.inf)
    for j in range(1, K):
        d2 = np.minimum(d2, dist(X, picks[-1]))
        p = np.cumsum(d2)
        if p[-1] == 0:
            picks.append(min(set(range(N)) - set(picks)))
        else:
            picks.append(min(int(np.searchsorted(p, u[j] * p[-1], side='right')), N - 1))
    return picks


def init_rows_plain(X, K, seed):
    """A straightforward second implementation of 'k-means++' for integer-grid data (every quantity exact): python loops."""
    N = len(X)
    u = np.random.default_rng(seed).random(K)
    picks = [min(int(u[0] * N), N - 1)]
    for j in range(1, K):
        d2 = [min(sum((float(a) - float(b)) ** 2 for a, b in zip(X[i], X[c])) for c in picks) for i in range(N)]
        total = sum(d2)
        if total == 0:
            picks.append(next(i for i in range(N) if i not in picks))
            continue
        target, run, pick = u[j] * total, 0.0, N - 1
        for i in range(N):
            run += d2[i]
            if run > target:                                         # searchsorted(side='right'): first p[i] > target
                pick = i
                break
        picks.append(pick)
    return picks


# ---------------------------------------------------------------------- whole fit ---------
FIT = dict(N=700, D=37, K=6, spread=2.0, noise=1.2, seed=11, max_iter=50)


def blobs(metric, fit=FIT):
    """Gaussian blobs as float32; for 'cosine' the rows normalised (float64, rounded once)."""
    rng = np.random.default_rng(fit['seed'])
    mu = fit['spread'] * rng.standard_normal((fit['K'], fit['D']))
    which = rng.integers(0, fit['K'], size=fit['N'])
    X = mu[which] + fit['noise'] * rng.standard_normal((fit['N'], fit['D']))
    if metric == 'cosine':
        X = X / np.sqrt((X * X).sum(1, keepdims=True))
    return X.astype(np.float32)


def lloyd_f64(X, rows, metric, max_iter, n_slots):
    """The float64 reference Lloyd run from the centres X[rows] -> dict: ``labels`` per iteration, ``centers`` per iteration,
    ``n_iter`` (first iteration whose labels repeat; None if none within max_iter), ``min_margin``: over iterations and rows,
    (gap between best and second-best score) / (2 * allowance), where the allowance is the two scores' float32 tolerances
    (neighbors_cases.tolerance; for cosine plus the aux vectors' own error 2 (D + 12) u |score|) plus the effect on each of the
    two scores of the centres' rounding bound (centers_tolerance of the previous iteration's assignment):
        l2      |d score| <= sum_d (2 |x_d - c_d| t_d + t_d^2)
        cosine  |d score| <= 2 |t|_2 / |c|_2       (a unit row's cosine is 1-Lipschitz in the centre's angle, which moves by at
                                                    most asin(|t| / |c|) <= (pi / 2) |t| / |c|)
    and ``no_empty``: no cluster ever lost all its rows.  A margin above 1 means no float32 evaluation within its bounds can
    choose another centre than this run."""
    X64 = np.asarray(X, dtype=np.float64)
    N, D = X64.shape
    C = X64[rows].copy()
    K = C.shape[0]
    tolC = np.zeros_like(C)
    labels, centers, n_iter, min_margin, no_empty = [], [], None, np.inf, True
    sign = 1.0 if metric == 'l2' else -1.0
    for it in range(max_iter):
        s = NC.scores_f64(X64, C, metric)
        tol = NC.tolerance(X64, C, metric)
        if metric == 'l2':
            eff = (2 * np.abs(X64[:, None, :] - C[None, :, :]) * tolC[None] + (tolC ** 2)[None]).sum(2)
        else:
            tol = tol + 2 * (D + 12) * U * np.abs(s)
            eff = np.broadcast_to((2 * np.sqrt((tolC ** 2).sum(1)) / np.sqrt((C ** 2).sum(1)))[None, :], s.shape)
        if K > 1:
            order = np.argsort(sign * s, axis=1, kind='stable')
            a, b = order[:, 0], order[:, 1]
            r = np.arange(N)
            gap = sign * (s[r, b] - s[r, a])
            allow = tol[r, a] + tol[r, b] + eff[r, a] + eff[r, b]
            min_margin = min(min_margin, float((gap / (2 * allow)).min()))
        else:
            a = np.zeros(N, dtype=np.int64)
        lab = a.astype(np.int32)
        counts = np.bincount(lab, minlength=K)
        no_empty = no_empty and bool((counts > 0).all())
        newC = np.where(counts[:, None] > 0, sums_f64(X64, lab, K) / np.maximum(counts, 1)[:, None], C)
        tolC = centers_tolerance(X64, lab, K, n_slots, newC)
        labels.append(lab)
        centers.append(newC)
        if it > 0 and np.array_equal(labels[-2], lab):
            n_iter = it + 1
            break
        C = newC
    return {'labels': labels, 'centers': centers, 'n_iter': n_iter, 'min_margin': min_margin, 'no_empty': no_empty,
            'center_tolerance': tolC}

"""Test helpers of the exact-DTW structure similarity (structure_similarity_fn = 'dtw_exact'): the seeded set both test
files use and a float64 restatement of the DP that is vectorised over the pairs, for sets too large for the pure-Python
oracle.  tests/test_dtw_exact_host.py pins the restatement to oracle.fastdtw_restate.exact_dtw bit for bit."""
import numpy as np


def seeded_set(sort):
    """64 x rows of 0-20 entries below 12, then 48 y rows of 1-50 entries below 30 (seed 11); ``sort``: every row
    ascending, like degree sequences, else as drawn."""
    rng = np.random.default_rng(11)
    xs = [rng.integers(0, 12, int(rng.integers(0, 21))).tolist() for _ in range(64)]
    ys = [rng.integers(0, 30, int(rng.integers(1, 51))).tolist() for _ in range(48)]
    if sort:
        xs, ys = [sorted(x) for x in xs], [sorted(y) for y in ys]
    return xs, ys


def _padded(rows):
    width = max(1, max((len(r) for r in rows), default=1))
    out = np.zeros((len(rows), width), dtype=np.float64)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out, np.array([len(r) for r in rows], dtype=np.int64)


def exact_dtw_distances(xs, ys):
    """D[i][j] = min(D[i-1][j], D[i][j-1], D[i-1][j-1]) + calc_dist(x[i], y[j]) over the whole grid, float64, for every
    (x row, y row) pair -> (len(xs), len(ys)) float64; NaN where either row is empty.  Column by column over the padded rows:
    a cell depends on cells above and to the left of it only, so the padding never reaches D[lx-1][ly-1]."""
    X, lx = _padded(xs)
    Y, ly = _padded(ys)
    N, M = len(xs), len(ys)
    res = np.full((N, M), np.nan)
    if N == 0 or M == 0:
        return res
    col = np.full((N, M, X.shape[1]), np.inf)
    rows = np.arange(N)
    x1 = X[:, None, :]
    for j in range(Y.shape[1]):
        yj = Y[None, :, j, None]
        cost = (np.maximum(x1, yj) + 1) / (np.minimum(x1, yj) + 1) - 1            # gamma.calc_dist
        up = np.full((N, M), np.inf)
        diag = np.full((N, M), 0.0 if j == 0 else np.inf)
        for i in range(X.shape[1]):
            old = col[:, :, i].copy()
            up = np.minimum(np.minimum(old, diag), up) + cost[:, :, i]
            col[:, :, i] = up
            diag = old
        for m in np.nonzero(ly - 1 == j)[0]:
            ok = lx > 0
            res[ok, m] = col[rows[ok], m, lx[ok] - 1]
    return res


def exact_dtw_similarities(xs, ys):
    """float32(1 / (1 + d)); pairs with an empty row are PAD (0), like the library's output."""
    d = exact_dtw_distances(xs, ys)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(d), 0.0, 1.0 / (d + 1.0)).astype(np.float32)

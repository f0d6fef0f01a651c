#!/usr/bin/env python3
"""Pairs on which fastdtw's three predecessor rules give different similarities (needs oracle/ and numpy only; no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_dtw_rules.py

Rules 1 and 2 (oracle/fastdtw_restate.py) differ only where rounding makes or breaks a tie between sums: on sorted rows --
what every other DTW fixture and random test holds -- no pair of 14 million sampled ones told them apart, and in ties.npz the
two rules' matrices are equal on every pair.  Unsorted rows of small values do tell them apart, on about 1 pair in 3 000, so
this script MINES them: per cell of

    x rows of 3..12 / 13..20 / 21..32 / 33..70 entries   (the register kernel's 12 / 20 / 32-row forms, the general kernel)
  x y rows of 34..65 / 66..97 / 98..130 entries          (coarse levels row-major / per-column words in LDS / in global scratch)

it draws DRAWS x X_PER_DRAW unsorted x rows and Y_CANDIDATES unsorted y rows (values below 3..6, fixed seed), scores every
pair with oracle.cbind.fastdtw_sim under rules 0, 1 and 2, keeps the Y_KEPT y rows (one of them of the class's shortest
length, one of its longest) and the X_KEPT x rows on which most pairs differ between rules 1 and 2, and stores the rows and
the three float32 matrices.  Differences are counted on the float32 similarities, as the kernels' output is compared.
Asserted here and again by tests/test_dtw_paths_host.py: every cell holds at least MIN_PAIRS pairs on which rules 1 and 2
differ and at least MIN_PAIRS on which rules 0 and 1 do.  Output: tests/golden/dtw_rules.npz (data only)."""
import os
import sys
from pathlib import Path

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

import numpy as np              # noqa: E402

from oracle import cbind        # noqa: E402

X_CLASSES = ((3, 12), (13, 20), (21, 32), (33, 70))
Y_CLASSES = ((34, 65), (66, 97), (98, 130))
SEED = 20261
DRAWS, X_PER_DRAW, Y_CANDIDATES = 4, 6000, 24
X_KEPT, Y_KEPT = 64, 4
MIN_PAIRS = 16


def cell_name(xc, yc):
    return 'x%d_%d__y%d_%d' % (xc[0], xc[1], yc[0], yc[1])


def _rows(rng, n, lo, hi, forced=()):
    """n unsorted rows of lo..hi entries, values below 3..6 (the bound drawn per row); the first rows take the forced lengths."""
    out = []
    for k in range(n):
        length = forced[k] if k < len(forced) else int(rng.integers(lo, hi + 1))
        out.append(rng.integers(0, int(rng.integers(3, 7)), length).astype(np.int32))
    return out


def _score(xs, ys):
    xp, xv = cbind.ragged(xs)
    yp, yv = cbind.ragged(ys)
    return [cbind.fastdtw_sim(xp, xv, yp, yv, t) for t in (0, 1, 2)]


def mine_cell(rng, xc, yc):
    # y candidates in Y_KEPT groups; the first group holds the class's shortest length only, the second its longest
    per = Y_CANDIDATES // Y_KEPT
    ys = _rows(rng, Y_CANDIDATES, yc[0], yc[1], forced=[yc[0]] * per + [yc[1]] * per)
    xs, sims = [], [[], [], []]
    for _ in range(DRAWS):
        part = _rows(rng, X_PER_DRAW, xc[0], xc[1], forced=[xc[0], xc[1]])
        xs += part
        for t, s in enumerate(_score(part, ys)):
            sims[t].append(s)
    s0, s1, s2 = (np.concatenate(s, 0) for s in sims)
    d12, d01 = s1 != s2, s0 != s1
    keep_y = [g * per + int(np.argmax(d12[:, g * per:(g + 1) * per].sum(0))) for g in range(Y_KEPT)]
    # x rows: most rule-1-vs-2 pairs first, then most rule-0-vs-1 pairs; a stable sort keeps the draw order among equals
    key = d12[:, keep_y].sum(1) * 100 + d01[:, keep_y].sum(1)
    keep_x = np.sort(np.argsort(-key, kind='stable')[:X_KEPT])
    xs, ys = [xs[int(i)] for i in keep_x], [ys[j] for j in keep_y]
    out = _score(xs, ys)                                            # scored again as stored: what the tests recompute
    for t, s in enumerate((s0, s1, s2)):
        assert np.array_equal(out[t], s[np.ix_(keep_x, keep_y)])
    n12, n01 = int((out[1] != out[2]).sum()), int((out[0] != out[1]).sum())
    assert n12 >= MIN_PAIRS and n01 >= MIN_PAIRS, (cell_name(xc, yc), n12, n01)
    return xs, ys, out, n12, n01


def main():
    rng = np.random.default_rng(SEED)
    z = {'cells': np.array([cell_name(xc, yc) for xc in X_CLASSES for yc in Y_CLASSES])}
    x_len, x_val, x_cell, y_len, y_val, y_cell = [], [], [], [], [], []
    for k, (xc, yc) in enumerate((xc, yc) for xc in X_CLASSES for yc in Y_CLASSES):
        xs, ys, sims, n12, n01 = mine_cell(rng, xc, yc)
        print('%-16s rule 1 != rule 2 on %3d pairs, rule 0 != rule 1 on %3d of %d' % (cell_name(xc, yc), n12, n01, sims[0].size),
              flush=True)
        x_len += [len(x) for x in xs]; x_val += xs; x_cell += [k] * len(xs)
        y_len += [len(y) for y in ys]; y_val += ys; y_cell += [k] * len(ys)
        for t in (0, 1, 2):
            z['%s_tie%d' % (cell_name(xc, yc), t)] = sims[t]
    z.update(x_len=np.array(x_len, dtype=np.uint8), x_val=np.concatenate(x_val).astype(np.uint8),
             x_cell=np.array(x_cell, dtype=np.uint8), y_len=np.array(y_len, dtype=np.uint8),
             y_val=np.concatenate(y_val).astype(np.uint8), y_cell=np.array(y_cell, dtype=np.uint8))
    np.savez_compressed(HERE / 'dtw_rules.npz', **z)
    print('wrote', HERE / 'dtw_rules.npz', os.path.getsize(HERE / 'dtw_rules.npz'), 'bytes')


if __name__ == '__main__':
    main()

"""-m gpu: every kernel path and predecessor rule of ``sgnn_dtw_similarity`` (structure_similarity_fn = 'dtw', csrc/dtw.hip)
against the oracle -- oracle.cbind.fastdtw_sim, which tests/test_dtw_paths_host.py grounds in the pure-Python restatement.
Every comparison is bit for bit (np.array_equal on float32): the cost function's division step is proven exact on the CPU
(test_reciprocal_division_is_exact), min and + round once, and the predecessor rule fixes the path.  No number here is a
tolerance.  tests/dtw_cases.py holds the cases and says which path each one runs; the host file asserts that together they
reach every path.  Every call goes into an output buffer of NaNs (or a sentinel) and states a workspace of at most 2 GiB."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dtw_cases as C
from oracle import cbind

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LARGEST_WORKSPACE = [0]


def _ops():
    from subgnn_amd import ops
    return ops


def _oracle(xs, ys, tie):
    xp, xv = cbind.ragged(xs)
    yp, yv = cbind.ragged(ys)
    return cbind.fastdtw_sim(xp, xv, yp, yv, tie)


def _raw(xs, ys, max_x, max_y, tie, kernel=0, order=None, live=None, fill=float('nan'), expect=0):
    """sgnn_dtw_similarity (sgnn_dtw_similarity_live when ``live`` is given) into an output buffer of ``fill`` -> the buffer."""
    from subgnn_amd import _lib
    ops = _ops()
    lib = _lib.load()
    assert max(map(len, xs)) <= max_x and max(map(len, ys)) <= max_y          # the arguments size the kernel's tables
    X, Y = ops.Ragged.from_lists(xs, DEV), ops.Ragged.from_lists(ys, DEV)
    out = torch.full((len(xs), len(ys)), fill, dtype=torch.float32, device=DEV)
    wsb = lib.sgnn_dtw_workspace_bytes(len(xs), max_x, len(ys), max_y)
    assert 0 < wsb <= C.WORKSPACE_CAP, wsb
    LARGEST_WORKSPACE[0] = max(LARGEST_WORKSPACE[0], wsb)
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    if live is None:
        rc = lib.sgnn_dtw_similarity(p(X.ptr), p(X.nodes), len(xs), max_x, p(Y.ptr), p(Y.nodes), len(ys), max_y, tie, kernel,
                                     p(order), p(out), p(ws), wsb, ops._stream())
    else:
        rc = lib.sgnn_dtw_similarity_live(p(X.ptr), p(X.nodes), len(xs), max_x, p(Y.ptr), p(Y.nodes), len(ys), max_y, tie, kernel,
                                          p(order), p(live), p(out), p(ws), wsb, ops._stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return out


def _written(out):
    """Every pair was written -> the matrix as numpy."""
    assert not bool(torch.isnan(out).any())
    return out.cpu().numpy()


def _call(xs, ys, max_x, max_y, **kw):
    ops = _ops()
    X, Y = ops.Ragged.from_lists(xs, DEV), ops.Ragged.from_lists(ys, DEV)
    return ops.dtw_similarity(X.ptr, X.nodes, max_x, Y.ptr, Y.nodes, max_y, **kw).cpu().numpy()


# ---- a. the mined fixture: every cell, every rule, every instantiation its rows fit ---------------------------------------------

CELLS = C.load_rule_cells()


@pytest.mark.parametrize('cell', CELLS, ids=[c.name for c in CELLS])
def test_mined_fixture_every_cell_every_rule(cell):
    """A cell of tests/golden/dtw_rules.npz -- unsorted rows mined so that at least 16 pairs differ between rules 1 and 2
    and 16 between rules 0 and 1 -- through the instantiation its lengths select and through the general kernel, under
    rules 0, 1, 2: the stored matrices.  Then the same rows with ``max_x_len`` and ``max_y_len`` overstated (the arguments
    choose the instantiation, not the data): 12-row data also through the 20- and 32-row forms, every y class also with its
    predecessor words in LDS (max_y_len 97) and in global scratch (130), so identical pairs go through the row-major form,
    the per-column words in LDS and in global scratch, and all three row counts.  A rule decided wrongly in one
    instantiation, or in the general kernel's run-time switch, fails here and nowhere else in the suite."""
    for tie in C.TIES:
        assert int((cell.sims[1] != cell.sims[2]).sum()) >= C.MIN_RULE_PAIRS
        for max_x, max_y, kernel in cell.calls():
            got = _written(_raw(cell.xs, cell.ys, max_x, max_y, tie, kernel))
            wrong = int((got != cell.sims[tie]).sum())
            labels = sorted(C.call_labels(max_x, max_y, kernel, [len(x) for x in cell.xs], [len(y) for y in cell.ys]))
            assert wrong == 0, (cell.name, tie, max_x, max_y, kernel, wrong, labels)


# ---- b. the length-boundary sweep -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _sweep(max_x, tie):
    xs, ys = C.sweep_rows(max_x)
    return xs, ys, _oracle(xs, ys, tie)


@pytest.mark.parametrize('tie', C.TIES)
@pytest.mark.parametrize('max_x', C.SWEEP_MAX_X)
def test_length_boundary_sweep(max_x, tie):
    """x rows of every length 0..max_x, at and around the row counts the register kernel is instantiated for, then random
    ones (231 rows: three wavefronts and a part of one), against y rows of 1..131 entries at every length where a level
    count, a column chunk, the row-major form or the place of the predecessor words changes, and an empty one; values below
    6, heavy-tailed up to 2e5 and near 2^31 - 1; sorted and unsorted.  The C entry with no processing order (a wavefront
    holds rows of 0, 1, 2, 3, ... entries: different level counts, a wide hull), once with max_y_len 97 over the rows that
    fit and once with the true maximum, then the general kernel, then ops.dtw_similarity over five copies of the rows with
    and without ordering and grouping: the oracle's matrix every time, every pair written."""
    xs, ys, want = _sweep(max_x, tie)
    empty_x = [i for i, x in enumerate(xs) if not x]
    for max_y, idx in C.sweep_runs(max_x, ys):
        sub = [ys[k] for k in idx]
        got = _written(_raw(xs, sub, max_x, max_y, tie))
        wrong = np.argwhere(got != want[:, idx])
        assert len(wrong) == 0, (max_y, len(wrong), [(len(xs[i]), len(sub[j])) for i, j in wrong[:8]])
        assert float(np.abs(got[empty_x]).max()) == 0.0 and float(np.abs(got[:, -1]).max()) == 0.0     # empty rows: PAD
        for order_rows in (True, False):
            for dedupe in (True, False):
                rep = _call(xs * 5, sub, max_x, max_y, tie_order=tie, order_rows=order_rows, dedupe=dedupe)
                assert np.array_equal(rep, np.tile(want[:, idx], (5, 1))), (max_y, order_rows, dedupe)
    assert np.array_equal(_written(_raw(xs, ys, max_x, max(map(len, ys)), tie, kernel=1)), want)


@pytest.mark.parametrize('tie', C.TIES)
@pytest.mark.parametrize('max_x', C.SWEEP_MAX_X)
def test_sweep_properties_that_need_no_oracle(max_x, tie):
    """On the sweep's rows: a similarity lies in (0, 1] for a non-empty pair and is exactly 0 for an empty one; fastdtw's
    is at most the exact one (fn='dtw_exact', pinned to its own restatement) and equal to it when either length is below 3
    (the window is the whole grid); a second call gives the same bits; a row against itself gives exactly 1 in every
    instantiation its length allows (tests/test_dtw_paths_host.py::test_a_row_against_itself_in_the_oracle says why)."""
    xs, ys, _ = _sweep(max_x, tie)
    max_y = max(map(len, ys))
    first = _raw(xs, ys, max_x, max_y, tie)
    got = _written(first)
    assert torch.equal(_raw(xs, ys, max_x, max_y, tie), first)
    lx, ly = np.array([len(x) for x in xs])[:, None], np.array([len(y) for y in ys])[None, :]
    live = (lx > 0) & (ly > 0)
    assert bool((got[live] > 0).all()) and bool((got[live] <= 1).all()) and bool((got[~live] == 0).all())
    exact = _call(xs, ys, max_x, max_y, fn='dtw_exact')
    assert bool((got <= exact).all())
    small = (lx < 3) | (ly < 3)
    assert np.array_equal(got[small & live], exact[small & live]) and int((small & live).sum()) > 100
    rows = [x for x in xs if x][:96]
    where = [xs.index(r) for r in rows]
    want = _oracle(xs, rows, tie)
    for my in sorted({max(max_x, 1), 97, 130}):
        for kernel in (0, 1):
            self_sim = _written(_raw(xs, rows, max_x, my, tie, kernel))
            assert np.array_equal(self_sim, want), (my, kernel)
            assert bool((self_sim[where, np.arange(len(rows))] == 1.0).all()), (my, kernel)


# ---- c. grid-stride loops and pyramid forms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', C.BIG_CASES)
def test_grid_stride_loops_and_pyramid_forms(name):
    """More tasks than the register kernel's launch has wavefronts (35 200 for 32 768), more pairs than the general
    kernel's has lanes (150 000 for 131 072), and more than 8 192 series on either side (the one-thread-per-series pyramid
    kernel: transposed with and without a processing order for x, plain for y).  The rows are drawn from a few hundred
    distinct ones: the oracle scores those and the test gathers."""
    c = C.big_case(name)
    xs, ys = [c['base_x'][int(i)] for i in c['pick_x']], [c['base_y'][int(j)] for j in c['pick_y']]
    labels = C.call_labels(c['max_x'], c['max_y'], c['kernel'], [len(x) for x in xs], [len(y) for y in ys], True)
    assert {'reg-tasks': 'reg/grid-stride', 'general-pairs': 'general/grid-stride', 'many-y': 'pyr/y/thread'}[name] in labels
    lens = np.array([len(x) for x in xs])
    for tie in C.TIES:
        want = _oracle(c['base_x'], c['base_y'], tie)[np.ix_(c['pick_x'], c['pick_y'])]
        for ordered in c['ordered']:
            order = torch.from_numpy(np.argsort(lens, kind='stable').astype(np.int32)).to(DEV) if ordered else None
            got = _written(_raw(xs, ys, c['max_x'], c['max_y'], tie, c['kernel'], order=order))
            assert np.array_equal(got, want), (name, tie, ordered, int((got != want).sum()))


# ---- d. the live-range entry ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('max_x,max_y', C.LIVE_CASES)
def test_live_range_entry_writes_its_range_only(max_x, max_y):
    """sgnn_dtw_similarity_live itself: a processing order that puts the empty rows first and a range {first, count} that
    leaves them and the last 37 positions out, into a buffer of a sentinel: the rows at positions inside the range equal
    the oracle, every other row keeps the sentinel, and a range without an order is refused."""
    xs, ys = C.live_rows(max_x, max_y)
    lens = np.array([len(x) for x in xs])
    order = np.argsort(lens, kind='stable').astype(np.int32)
    first = int((lens == 0).sum())
    count = len(xs) - first - 37
    assert first >= 8 and count > 192
    inside = order[first:first + count]
    outside = np.setdiff1d(np.arange(len(xs)), inside)
    live = torch.tensor([first, count], dtype=torch.int64, device=DEV)
    for tie in C.TIES:
        want = _oracle(xs, ys, tie)
        got = _raw(xs, ys, max_x, max_y, tie, order=torch.from_numpy(order).to(DEV), live=live, fill=-7.0).cpu().numpy()
        assert np.array_equal(got[inside], want[inside]), tie
        assert bool((got[outside] == -7.0).all()), tie
        kept = _raw(xs, ys, max_x, max_y, tie, order=None, live=live, fill=-7.0, expect=-1)
        assert bool((kept == -7.0).all())


def test_largest_workspace_asked_for():
    """(Reported, and bounded in every call: the general kernel at 70 x 131 and the register kernel's global scratch at
    max_y_len 131 are the large ones.)"""
    print('largest workspace any call of this file stated: %d bytes' % LARGEST_WORKSPACE[0])
    assert LARGEST_WORKSPACE[0] <= C.WORKSPACE_CAP

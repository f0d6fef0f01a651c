"""-m gpu: the DTW x side prepared once (sgnn_dtw_prepare_rows + sgnn_dtw_similarity_rows / _rows_live, and the exact-DTW
twins) gives what the per-call entries give, bit for bit -- the same kernels read the same pyramids, only from a buffer the
caller keeps -- and ``ops.dtw_similarity(x_fixed=True)`` keeps and reuses it.  "Equal" is torch.equal throughout."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAD_ARG = -1

# row lengths per case: 0-3 are where the coarsest-level and empty-row rules switch; the longest row picks the register
# kernel's instantiation (12 / 20 / 32 rows)
LENGTHS = {12: (0, 1, 2, 3, 5, 12), 20: (0, 1, 2, 3, 5, 12, 13, 20), 32: (0, 1, 2, 3, 5, 12, 13, 20, 21, 27, 32)}
N_X = 130                                   # three wavefront tasks, the last one partial


def _ragged(lengths, rng, sort):
    ptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lengths)
    pool = rng.integers(1, 3001, size=40)   # values in [1, 3000], drawn from a small pool: repeats
    rows = [np.sort(rng.choice(pool, size=n))[::-1] if sort else rng.choice(pool, size=n) for n in lengths]
    val = np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    if val.size == 0:
        val = np.zeros(1, dtype=np.int32)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(val).to(DEV)


def _x_rows(max_len, seed=0):
    rng = np.random.default_rng(100 + max_len + seed)
    kinds = LENGTHS[max_len]
    lengths = list(kinds) + list(rng.choice(kinds, size=N_X - len(kinds)))
    rng.shuffle(lengths)
    assert set(lengths) == set(kinds) and len(lengths) == N_X
    return _ragged(lengths, rng, sort=True), np.array(lengths)


def _y_rows():
    return _ragged([50, 7, 1], np.random.default_rng(7), sort=True)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Lib:
    """The raw entries of one similarity function: per call, prepare, over prepared rows."""

    def __init__(self, fn):
        from subgnn_amd import _lib
        self.lib, self.fn = _lib.load(), fn
        self.pre = 'sgnn_dtw_' if fn == 'dtw' else 'sgnn_dtwx_'
        self.plain = 'sgnn_dtw_similarity' if fn == 'dtw' else 'sgnn_dtw_exact_similarity'
        self.plain_ws = 'sgnn_dtw_workspace_bytes' if fn == 'dtw' else 'sgnn_dtw_exact_workspace_bytes'

    def _tail(self, tie, kernel, order, live, out, ws, wsb):
        args = ([int(tie)] if self.fn == 'dtw' else []) + [int(kernel), _p(order)]
        if live is not None:
            args.append(_p(live))
        return args + [_p(out), _p(ws), wsb, None]

    def _out(self, nx, ny, live):
        return (torch.zeros if live is not None else torch.empty)((nx, ny), dtype=torch.float32, device=DEV)

    def per_call(self, x, mx, y, my, tie, kernel, order, live):
        nx, ny = x[0].numel() - 1, y[0].numel() - 1
        wsb = getattr(self.lib, self.plain_ws)(nx, mx, ny, my)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=DEV)
        out = self._out(nx, ny, live)
        rc = getattr(self.lib, self.plain + ('_live' if live is not None else ''))(
            _p(x[0]), _p(x[1]), nx, mx, _p(y[0]), _p(y[1]), ny, my, *self._tail(tie, kernel, order, live, out, ws, wsb))
        assert rc == 0
        return out

    def prepare(self, x, mx, kernel, order):
        nx = x[0].numel() - 1
        nbytes = getattr(self.lib, self.pre + 'rows_bytes')(nx, mx)
        buf = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
        header = (ctypes.c_int64 * int(self.lib.sgnn_dtw_rows_header_words()))()
        rc = getattr(self.lib, self.pre + 'prepare_rows')(_p(x[0]), _p(x[1]), nx, mx, int(kernel), _p(order), _p(buf), nbytes,
                                                          ctypes.addressof(header), None)
        assert rc == 0
        return buf, header

    def over_rows(self, rows, nx, mx, y, my, tie, kernel, order, live, want_rc=0):
        ny = y[0].numel() - 1
        wsb = getattr(self.lib, self.pre + 'rows_workspace_bytes')(nx, mx, ny, my)
        assert wsb == getattr(self.lib, self.plain_ws)(nx, mx, ny, my) - getattr(self.lib, self.pre + 'rows_bytes')(nx, mx)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=DEV)
        out = self._out(nx, ny, live)
        rc = getattr(self.lib, self.pre + 'similarity_rows' + ('_live' if live is not None else ''))(
            ctypes.addressof(rows[1]), nx, mx, _p(y[0]), _p(y[1]), ny, my, *self._tail(tie, kernel, order, live, out, ws, wsb))
        assert rc == want_rc
        return out


def _orders(lengths):
    """No order; a permutation; the length-first order with its live range (empty rows first, as the ``_live`` entries ask)."""
    n = len(lengths)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n).astype(np.int32)).to(DEV)
    by_len = torch.from_numpy(np.argsort(lengths, kind='stable').astype(np.int32)).to(DEV)
    n_empty = int((lengths == 0).sum())
    live = torch.tensor([n_empty, n - n_empty], dtype=torch.int64, device=DEV)
    return (('no order', None, None), ('order', perm, None), ('live range', by_len, live))


@pytest.mark.parametrize('fn', ['dtw', 'dtw_exact'])
@pytest.mark.parametrize('kernel', [0, 1])
@pytest.mark.parametrize('max_len', [12, 20, 32])
def test_prepared_rows_give_the_per_call_result_bit_for_bit(max_len, kernel, fn):
    L = _Lib(fn)
    x, lengths = _x_rows(max_len)
    y = _y_rows()
    assert int(lengths.max()) == max_len and (lengths == 0).any()
    for name, order, live in _orders(lengths):
        rows = L.prepare(x, max_len, kernel, order)
        for tie in ((0, 1, 2) if fn == 'dtw' else (0,)):
            want = L.per_call(x, max_len, y, 50, tie, kernel, order, live)
            got = L.over_rows(rows, N_X, max_len, y, 50, tie, kernel, order, live)
            torch.cuda.synchronize()
            assert torch.equal(got, want), (name, tie)
            assert bool((want[torch.from_numpy(lengths == 0).to(DEV)] == 0).all())           # empty rows are PAD
            assert bool((want[torch.from_numpy(lengths > 0).to(DEV)] > 0).all())


@pytest.mark.parametrize('fn', ['dtw', 'dtw_exact'])
def test_a_buffer_of_another_layout_count_or_function_is_refused(fn):
    L = _Lib(fn)
    x, lengths = _x_rows(20)
    y = _y_rows()
    _, perm, _ = _orders(lengths)[1]
    reg = L.prepare(x, 20, 0, perm)            # the register kernel's layout: positions follow the order
    gen = L.prepare(x, 20, 1, perm)            # the general kernel's: positions are the row numbers
    assert reg[1][1] != gen[1][1]
    L.over_rows(reg, N_X, 20, y, 50, 0, 1, perm, None, want_rc=BAD_ARG)
    L.over_rows(gen, N_X, 20, y, 50, 0, 0, perm, None, want_rc=BAD_ARG)
    L.over_rows(reg, N_X, 20, y, 50, 0, 0, None, None, want_rc=BAD_ARG)          # prepared in an order, called without one
    L.over_rows(reg, N_X - 1, 20, y, 50, 0, 0, perm, None, want_rc=BAD_ARG)      # another row count
    L.over_rows(reg, N_X, 21, y, 50, 0, 0, perm, None, want_rc=BAD_ARG)          # another length bound
    other = _Lib('dtw_exact' if fn == 'dtw' else 'dtw')
    other.over_rows(reg, N_X, 20, y, 50, 0, 0, perm, None, want_rc=BAD_ARG)      # the other function's buffer
    blank = (reg[0], (ctypes.c_int64 * len(reg[1]))())
    L.over_rows(blank, N_X, 20, y, 50, 0, 0, perm, None, want_rc=BAD_ARG)        # a header nobody filled
    torch.cuda.synchronize()
    # the natural layout serves the register kernel without an order and the general kernel with any
    want = L.per_call(x, 20, y, 50, 0, 0, None, None)
    assert torch.equal(L.over_rows(gen, N_X, 20, y, 50, 0, 0, None, None), want)
    assert torch.equal(L.over_rows(gen, N_X, 20, y, 50, 0, 1, perm, None), want)


def _grouped_rows(n, distinct, max_len, seed):
    rng = np.random.default_rng(seed)
    base = [np.sort(rng.integers(1, 3001, size=int(k)))[::-1] for k in rng.integers(0, max_len + 1, size=distinct)]
    base[0], base[1] = base[0][:0], np.sort(rng.integers(1, 3001, size=max_len))[::-1]
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])
    rng.shuffle(pick)
    rows = [base[i] for i in pick]
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    val = np.concatenate(rows).astype(np.int32)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(val).to(DEV)


@pytest.mark.parametrize('fn', ['dtw', 'dtw_exact'])
@pytest.mark.parametrize('n,dedupe', [(1100, True), (1100, False), (130, True)])
def test_fixed_rows_are_prepared_once_and_give_the_same_similarities(n, dedupe, fn):
    """ops.dtw_similarity(x_fixed=True) three times with one DtwRowPrep == three calls without: 1 100 rows with 200 distinct
    ones (grouping needs more than 1 024 rows), grouped and not, and 130 rows (never grouped)."""
    from subgnn_amd import ops
    x_ptr, x_val = _grouped_rows(n, 200 if n > 1024 else n, 20, seed=n)
    y_ptr, y_val = _y_rows()
    prep = ops.DtwRowPrep()
    seen = []
    for k in range(3):
        want = ops.dtw_similarity(x_ptr, x_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn)
        got = ops.dtw_similarity(x_ptr, x_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn, x_prep=prep, x_fixed=True)
        torch.cuda.synchronize()
        assert torch.equal(got, want), k
        assert prep.rows is not None and prep.rows.key == (fn, 0, 20, dedupe and n > 1024)
        assert (prep.grouped_val is not None) == (dedupe and n > 1024)
        seen.append((prep.rows, prep.grouped_val))
    assert seen[0][0] is seen[1][0] is seen[2][0] and seen[0][1] is seen[2][1]            # built once
    assert prep.nbytes >= prep.rows.nbytes > 0
    # without the promise nothing of the values is kept
    plain = ops.DtwRowPrep()
    ops.dtw_similarity(x_ptr, x_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn, x_prep=plain)
    assert plain.rows is None and plain.grouped_val is None
    # another row count: everything is rebuilt for it
    x2_ptr, x2_val = _grouped_rows(n + 7, 200 if n > 1024 else n, 20, seed=n + 1)
    want = ops.dtw_similarity(x2_ptr, x2_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn)
    got = ops.dtw_similarity(x2_ptr, x2_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn, x_prep=prep, x_fixed=True)
    assert torch.equal(got, want) and prep.rows is not seen[0][0] and prep.shape[0] == n + 7
    # the same count and length but another tensor: the promise was about the first one
    x3_val = x2_val.clone()
    x3_val[:5] += 1
    rows2 = prep.rows
    want = ops.dtw_similarity(x2_ptr, x3_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn)
    got = ops.dtw_similarity(x2_ptr, x3_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn, x_prep=prep, x_fixed=True)
    assert torch.equal(got, want) and prep.rows is not rows2 and not torch.equal(got, ops.dtw_similarity(
        x2_ptr, x2_val, 20, y_ptr, y_val, 50, 2, dedupe=dedupe, fn=fn))


def test_fixed_rows_built_on_one_stream_are_read_on_another():
    from subgnn_amd import ops
    x_ptr, x_val = _grouped_rows(1100, 200, 20, seed=5)
    y_ptr, y_val = _y_rows()
    want = ops.dtw_similarity(x_ptr, x_val, 20, y_ptr, y_val, 50, 2)
    torch.cuda.synchronize()
    prep, second = ops.DtwRowPrep(), torch.cuda.Stream()
    with torch.cuda.stream(second):
        a = ops.dtw_similarity(x_ptr, x_val, 20, y_ptr, y_val, 50, 2, x_prep=prep, x_fixed=True)
    b = ops.dtw_similarity(x_ptr, x_val, 20, y_ptr, y_val, 50, 2, x_prep=prep, x_fixed=True)   # (no synchronisation in between)
    torch.cuda.synchronize()
    assert torch.equal(a, want) and torch.equal(b, want)

"""-m gpu: the content-keyed draws (sgnn_set_keys, sgnn_sample_anchors_ragged_keyed, sgnn_choice_ragged_keyed,
sgnn_sample_border_anchors_keyed).  With keys = item_base + arange(n) each keyed kernel writes the bits of its unkeyed twin; with
arbitrary keys (values >= 2^63 among them) a set's row depends on its own key, flag and content only -- the list may be permuted
or extended -- and is what the tape's law says for that key; sgnn_set_keys is tape.set_key_np and ignores the order of a set's
entries.  Integers, and floats that hold small integers: every comparison is exact.  Every output lies between guard words."""
import numpy as np
import pytest
import torch

from oracle import tape as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PATTERN = 0x5A5A5A5A
SIZES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 200)       # 32: the bound of the "every variate negative" draw; 64: the wavefront
SLOTS = (1, 37)
SEED = 11
ITEM_BASE = 5
MASK64 = (1 << 64) - 1


def _ops():
    from subgnn_amd import ops
    return ops


def _lib():
    from subgnn_amd import _lib
    return _lib.load()


class _Guarded:
    """A tensor of ``shape`` between two guards of 256 bytes, all pre-filled with PATTERN."""

    def __init__(self, shape, dtype):
        size = torch.empty(0, dtype=dtype).element_size()
        self.g, self.n = 256 // 4, int(np.prod(shape)) * size // 4
        self.buf = torch.full((2 * self.g + self.n,), PATTERN, dtype=torch.int32, device=DEV)
        self.t = self.buf[self.g:self.g + self.n].view(dtype).view(shape)

    def done(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:self.g] == PATTERN).all()), what + ': a store in front of the output'
        assert bool((self.buf[self.g + self.n:] == PATTERN).all()), what + ': a store behind the output'
        return self.t.clone()


_case = []


def _lists():
    """The one ragged list of all kernel checks: ascending sets of SIZES entries, an aligned hop per entry (1..3), and keys."""
    if not _case:
        rng = np.random.default_rng(3)
        sets = [sorted(int(v) for v in rng.choice(np.arange(1, 5000), n, replace=False)) for n in SIZES]
        hops = [[int(h) for h in rng.integers(1, 4, n)] for n in SIZES]
        keys = [int(k) for k in rng.integers(0, 1 << 63, len(SIZES), dtype=np.uint64)]
        keys[1], keys[4], keys[7] = (1 << 63) + 12345, MASK64, (1 << 63)            # the sign bit, all ones
        flags = [1, 1, 0, 1, 1, 1, 0, 1, 1, 0]
        _case.append((sets, hops, keys, flags))
    return _case[0]


def _ragged(sets):
    return _ops().Ragged.from_lists(sets, DEV)


def _flat(xs, dtype):
    return torch.tensor([v for x in xs for v in x] or [0], dtype=dtype, device=DEV)


def _keys_t(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def _u8(xs):
    return torch.tensor(list(xs), dtype=torch.uint8, device=DEV)


def _anchors(keyed, r, flags, keys, A, st, item_base=0):
    ops, lib = _ops(), _lib()
    P = ops._ptr
    out = _Guarded((r.n, A), torch.int64)
    if keyed:
        rc = lib.sgnn_sample_anchors_ragged_keyed(P(r.ptr), P(r.nodes), r.n, P(flags), P(keys), A, SEED, st, P(out.t), ops._stream())
    else:
        rc = lib.sgnn_sample_anchors_ragged(P(r.ptr), P(r.nodes), r.n, P(flags), A, SEED, st, item_base, P(out.t), ops._stream())
    assert rc == 0
    return out.done('anchors')


def _choice(keyed, r, keys, A, st, item_base=0):
    ops, lib = _ops(), _lib()
    P = ops._ptr
    out = _Guarded((r.n, A), torch.int64)
    if keyed:
        rc = lib.sgnn_choice_ragged_keyed(P(r.ptr), P(r.nodes), r.n, P(keys), A, SEED, st, P(out.t), ops._stream())
    else:
        rc = lib.sgnn_choice_ragged(P(r.ptr), P(r.nodes), r.n, A, SEED, st, item_base, P(out.t), ops._stream())
    assert rc == 0
    return out.done('choice')


def _border_keyed(r, hops, flags, keys, A, st):
    ops, lib = _ops(), _lib()
    P = ops._ptr
    a, w = _Guarded((r.n, A), torch.int64), _Guarded((r.n, A), torch.float32)
    assert lib.sgnn_sample_border_anchors_keyed(P(r.ptr), P(r.nodes), P(hops), r.n, P(flags), P(keys), A, SEED, st, P(a.t), P(w.t),
                                                ops._stream()) == 0
    return a.done('border anchors'), w.done('border similarities')


@pytest.mark.parametrize('A', SLOTS)
def test_row_number_keys_give_the_unkeyed_bits(A):
    ops, lib = _ops(), _lib()
    P = ops._ptr
    sets, hops, _, flags = _lists()
    r, n = _ragged(sets), len(sets)
    keys = _keys_t([ITEM_BASE + i for i in range(n)])
    fl = _u8(flags)
    st = T.stream_id(T.STREAM_N_INT, 'train', 1)
    assert torch.equal(_anchors(True, r, fl, keys, A, st), _anchors(False, r, fl, None, A, st, ITEM_BASE))
    st = T.stream_id(T.STREAM_P_INT, 'val', 0)
    assert torch.equal(_choice(True, r, keys, A, st), _choice(False, r, None, A, st, ITEM_BASE))
    # the border form against the kept-border draw at hop 1 on the same sorted borders: row_has_pad = counts < width
    st = T.stream_id(T.STREAM_N_BOR, 'train', 0)
    for width in (max(SIZES), 64, 0):                         # nobody but the widest row / rows under 64 / no row has a PAD
        counts = r.lengths.contiguous()
        wd = torch.tensor([width], dtype=torch.int64, device=DEV)
        a0, w0 = _Guarded((n, A), torch.int64), _Guarded((n, A), torch.float32)
        assert lib.sgnn_sample_border_anchors(P(r.ptr), P(r.nodes), P(counts), n, P(wd), A, SEED, st, ITEM_BASE, 1, P(a0.t), P(w0.t),
                                              ops._stream()) == 0
        ones = torch.ones(max(int(r.ptr[-1]), 1), dtype=torch.uint8, device=DEV)
        a1, w1 = _border_keyed(r, ones, (counts < width).to(torch.uint8), keys, A, st)
        assert torch.equal(a1, a0.done('kept border anchors')) and torch.equal(w1, w0.done('kept border similarities'))
        assert w1.dtype == torch.float32 and a1.dtype == torch.int64


def test_set_keys_are_the_host_formula_and_ignore_order():
    from subgnn_amd import tape
    ops, lib = _ops(), _lib()
    sets = _lists()[0]
    rng = np.random.default_rng(9)
    shuffled = [[s[i] for i in rng.permutation(len(s))] for s in sets]
    assert any(a != b for a, b in zip(sets, shuffled))
    want = [tape.set_key_np(s) for s in sets]
    assert len(set(want)) == len(want)
    for lists in (sets, shuffled):
        r = _ragged(lists)
        out = _Guarded((r.n,), torch.int64)
        assert lib.sgnn_set_keys(ops._ptr(r.ptr), ops._ptr(r.nodes), r.n, ops._ptr(out.t), ops._stream()) == 0
        got = out.done('keys').cpu().numpy().view(np.uint64).tolist()
        assert got == want
    assert ops.set_keys(_ragged(shuffled)).cpu().numpy().view(np.uint64).tolist() == want
    # repeated entries count: {1, 2}, {1, 2, 2}, {1, 2, 3}
    got = ops.set_keys(_ragged([[1, 2], [1, 2, 2], [1, 2, 3], [2, 1, 2]])).cpu().numpy().view(np.uint64).tolist()
    assert got == [tape.set_key_np(s) for s in ([1, 2], [1, 2, 2], [1, 2, 3], [1, 2, 2])] and len(set(got)) == 3


@pytest.mark.parametrize('A', SLOTS)
def test_arbitrary_keys_follow_the_law_and_nothing_else_in_the_list(A):
    sets, hops, keys, flags = _lists()
    n = len(sets)
    r = _ragged(sets)
    s_ni, s_nb, s_pi = (T.stream_id(k, 3, 1) for k in (T.STREAM_N_INT, T.STREAM_N_BOR, T.STREAM_P_INT))

    def run(order, extra=()):
        ss = [sets[i] for i in order] + [e[0] for e in extra]
        hh = [hops[i] for i in order] + [e[1] for e in extra]
        kk = _keys_t([keys[i] for i in order] + [e[2] for e in extra])
        ff = _u8([flags[i] for i in order] + [e[3] for e in extra])
        rr = _ragged(ss)
        a = _anchors(True, rr, ff, kk, A, s_ni)
        ba, bw = _border_keyed(rr, _flat(hh, torch.uint8), ff, kk, A, s_nb)
        c = _choice(True, rr, kk, A, s_pi)
        return a, ba, bw, c

    base = run(range(n))
    # the law, from the oracle's tape, for every (set, slot)
    a, ba, bw, c = (x.cpu().numpy() for x in base)
    for i, (s, h, k, f) in enumerate(zip(sets, hops, keys, flags)):
        for slot in range(A):
            item = (k * A + slot) & MASK64
            kk = T.nanchor_pick(SEED, s_ni, item, len(s), bool(f))
            assert a[i, slot] == (0 if kk < 0 else s[kk]), (i, slot)
            kk = T.nanchor_pick(SEED, s_nb, item, len(s), bool(f))
            assert ba[i, slot] == (0 if kk < 0 else s[kk]) and bw[i, slot] == (0.0 if kk < 0 else float(h[kk])), (i, slot)
            assert c[i, slot] == (s[T.choice_index(SEED, s_pi, k, slot, len(s))] if s else 0), (i, slot)
    # empty set: anchor 0, similarity 0
    e = SIZES.index(0)
    assert not a[e].any() and not ba[e].any() and not bw[e].any() and not c[e].any()
    # permuting the sets with their keys and flags permutes the rows
    perm = [int(i) for i in np.random.default_rng(5).permutation(n)]
    assert perm != list(range(n))
    got = run(perm)
    for x, y in zip(got, base):
        assert torch.equal(x, y[torch.tensor(perm, device=DEV)])
    # a set appended to the list leaves the other rows as they were
    got = run(range(n), extra=[([7, 8, 9], [2, 1, 3], (1 << 63) + 77, 1)])
    for x, y in zip(got, base):
        assert x.shape[0] == n + 1 and torch.equal(x[:n], y)
    del r


def test_rows_without_a_pad_column_never_draw_pad():
    """Sets of 1 and 2 entries draw PAD in a half / a quarter of their slots when the row has a PAD column (checked: the flag is
    what switches it off), and never without one."""
    A = 37
    sets = [[5], [5, 9], [3]] * 40
    r = _ragged(sets)
    keys = _keys_t([int(k) for k in np.random.default_rng(1).integers(0, MASK64, len(sets), dtype=np.uint64, endpoint=True)])
    hops = torch.ones(int(r.ptr[-1]), dtype=torch.uint8, device=DEV)
    st = T.stream_id(T.STREAM_N_BOR, 3, 0)
    for flag in (0, 1):
        fl = _u8([flag] * len(sets))
        a = _anchors(True, r, fl, keys, A, st)
        ba, bw = _border_keyed(r, hops, fl, keys, A, st)
        assert torch.equal(a, ba) and torch.equal(bw, (ba != 0).float())
        if flag:
            assert bool((a == 0).any())
        else:
            assert bool((a != 0).all())


def test_wrapper_argument_checks():
    ops = _ops()
    sets, hops, keys, flags = _lists()
    r = _ragged(sets)
    with pytest.raises(ValueError):
        ops.sample_anchors_ragged_keyed(r, _keys_t(keys[:-1]), _u8(flags), 2, SEED, 1)
    with pytest.raises(ValueError):
        ops.choice_ragged_keyed(r, _keys_t(keys + [1]), 2, SEED, 1)
    with pytest.raises(TypeError):
        ops.sample_anchors_ragged_keyed(r, _keys_t(keys), _u8(flags).to(torch.int32), 2, SEED, 1)
    a, w = ops.draw_border_anchors_keyed(r, _flat(hops, torch.uint8), _keys_t(keys), _u8(flags), 3, SEED, 1)
    assert a.shape == (len(sets), 3) and w.shape == (len(sets), 3) and w.dtype == torch.float32

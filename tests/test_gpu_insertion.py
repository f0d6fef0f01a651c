"""-m gpu: the insertion-set kernels (sgnn_insertion_count / sgnn_insertion_write, ops.insertion_sets) against the numpy
definition of tests/insertion_cases.py, bit for bit: the counts, the variants' nodes, parents, inserted ids and keys, at every set
length the kernels branch on (each alone and all mixed in one call), every candidate-row length around the chunk edges and every
candidate shape, with one row per set and with one shared row.  The entries are called directly with guard words around every
output; refused calls write nothing; a call on another stream gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import insertion_cases as IC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 16
FIELDS = ('variants', 'ptr', 'parent', 'cand', 'nodes', 'keys')


def _ragged(sets):
    from subgnn_amd import ops
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    flat = np.concatenate(list(sets) + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    if flat.size == 0:
        flat = np.zeros(1, dtype=np.int32)                            # (a tensor of no elements has no address)
    return ops.Ragged(torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), max_len=max(len(s) for s in sets))


class Guarded:
    """A device buffer of ``n`` elements with GUARD sentinel words on either side."""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        # (the address is taken from the whole buffer: an empty slice has none)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _run_entries(sets, rows, shared):
    """The two entries called as ops.insertion_sets calls them, on guarded outputs -> dict of numpy arrays."""
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    r, c = _ragged(sets), _ragged(rows)
    head = (ops._ptr(r.ptr), ops._ptr(r.nodes), r.n, r.max_len, ops._ptr(c.ptr), ops._ptr(c.nodes), 1 if shared else 0)
    variants = Guarded(r.n, torch.int64, -7)
    assert lib.sgnn_insertion_count(*head, variants.ptr, ops._stream()) == 0
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    var_ptr = torch.cat([zero, torch.cumsum(variants.t, 0)])
    entry_ptr = torch.cat([zero, torch.cumsum(variants.t * (r.lengths + 1), 0)])
    V, T = int(var_ptr[-1]), int(entry_ptr[-1])
    out_ptr = Guarded(V + 1, torch.int64, -7)
    out_ptr.t.zero_()
    nodes, parent, cand, keys = (Guarded(T, torch.int32, -7), Guarded(V, torch.int32, -7), Guarded(V, torch.int32, -7),
                                 Guarded(V, torch.int64, -7))
    assert lib.sgnn_insertion_write(*head, ops._ptr(var_ptr), ops._ptr(entry_ptr), V, out_ptr.ptr, nodes.ptr, parent.ptr, cand.ptr,
                                    keys.ptr, ops._stream()) == 0
    torch.cuda.synchronize()
    bufs = {'variants': variants, 'ptr': out_ptr, 'nodes': nodes, 'parent': parent, 'cand': cand, 'keys': keys}
    for k, b in bufs.items():
        assert b.intact(), 'guard words of ' + k
    got = {k: b.t.cpu().numpy() for k, b in bufs.items()}
    got['keys'] = got['keys'].view(np.uint64)
    return got


def _check(got, want, what):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


def _ops_result(o, T):
    got = {'variants': o.variants, 'ptr': o.sets.ptr, 'nodes': o.sets.nodes[:T], 'parent': o.parent, 'cand': o.cand, 'keys': o.keys}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got['keys'] = got['keys'].view(np.uint64)
    return got


def _check_ops(sets, rows, shared, want, what, side_stream=True):
    """ops.insertion_sets gives the same, its keys are ops.set_keys of what it wrote, and so does a call on another stream."""
    from subgnn_amd import ops
    r, c = _ragged(sets), _ragged(rows)
    results = [ops.insertion_sets(r, c, shared)]
    if side_stream:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            results.append(ops.insertion_sets(r, c, shared))
        side.synchronize()
    torch.cuda.synchronize()
    T = int(want['ptr'][-1])
    for o in results:
        _check(_ops_result(o, T), want, what + ' (ops)')
        assert o.sets.max_len == r.max_len + 1 and o.sets.n == len(want['parent'])
        assert o.parent.dtype == o.cand.dtype == torch.int32 and o.keys.dtype == o.variants.dtype == torch.int64
    if results[0].sets.n:
        assert torch.equal(ops.set_keys(results[0].sets), results[0].keys), what


@pytest.mark.parametrize('shape', IC.SHAPES)
@pytest.mark.parametrize('n', IC.SET_LENGTHS)
def test_every_set_length_alone(n, shape):
    """One set, one candidate row of every length: per set and shared read the same arrays and must write the same bits."""
    for name, (sets, rows) in IC.single_cases(lengths=(n,), shapes=(shape,)).items():
        want = IC.expand(sets, rows)
        _check(_run_entries(sets, rows, False), want, name)
        _check(_run_entries(sets, rows, True), want, name + ', shared')
        _check_ops(sets, rows, False, want, name, side_stream=len(rows[0]) in (65, 1000))
        _check_ops(sets, rows, True, want, name + ', shared', side_stream=False)


def test_all_lengths_in_one_list():
    sets, rows = IC.mixed_case()
    want = IC.expand(sets, rows)
    assert int((want['variants'] > 0).sum()) >= 12
    _check(_run_entries(sets, rows, False), want, 'mixed')
    _check_ops(sets, rows, False, want, 'mixed')


def test_a_shared_pool_and_its_rows_per_set_give_the_same_bits():
    sets, pool = IC.pool_case()
    want = IC.expand(sets, pool, shared=True)
    again = IC.expand(sets, pool * len(sets))
    for k in FIELDS:
        assert np.array_equal(want[k], again[k]), k
    shared, per_set = _run_entries(sets, pool, True), _run_entries(sets, pool * len(sets), False)
    _check(shared, want, 'pool, shared')
    _check(per_set, want, 'pool, one row per set')
    _check_ops(sets, pool, True, want, 'pool, shared')
    _check_ops(sets, pool * len(sets), False, want, 'pool, one row per set', side_stream=False)


def test_more_sets_than_one_trip_of_the_grid_stride_loop():
    sets, rows = IC.many_case()
    assert len(sets) > IC.WAVE_GRID_CAP
    want = IC.expand(sets, rows)
    assert want['variants'].tolist() == [0 if i % 7 == 0 else 1 for i in range(IC.MANY)]
    _check(_run_entries(sets, rows, False), want, 'many sets')
    _check_ops(sets, rows, False, want, 'many sets')


def test_refused_calls_write_nothing():
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    sets = [IC.make_set(5, 1), IC.make_set(70, 2)]
    rows = [IC.make_candidates(s, 4, 'disjoint', 3) for s in sets]
    r, c = _ragged(sets), _ragged(rows)
    out = Guarded(8, torch.int64, -7)
    P, N, CP, CN, st = ops._ptr(r.ptr), ops._ptr(r.nodes), ops._ptr(c.ptr), ops._ptr(c.nodes), ops._stream()
    refused = [
        lib.sgnn_insertion_count(P, N, -2, 70, CP, CN, 0, out.ptr, st),                 # negative sizes
        lib.sgnn_insertion_count(P, N, r.n, -1, CP, CN, 0, out.ptr, st),
        lib.sgnn_insertion_count(P, N, 2 ** 31, 70, CP, CN, 0, out.ptr, st),            # n_sets above 2^31 - 1
        lib.sgnn_insertion_count(P, N, r.n, 70, CP, CN, 2, out.ptr, st),                # shared outside {0, 1}
        lib.sgnn_insertion_count(P, N, r.n, 70, CP, CN, -1, out.ptr, st),
        lib.sgnn_insertion_count(None, N, r.n, 70, CP, CN, 0, out.ptr, st),             # null pointers with work to do
        lib.sgnn_insertion_count(P, None, r.n, 70, CP, CN, 0, out.ptr, st),
        lib.sgnn_insertion_count(P, N, r.n, 70, None, CN, 0, out.ptr, st),
        lib.sgnn_insertion_count(P, N, r.n, 70, CP, None, 0, out.ptr, st),
    ]
    assert lib.sgnn_insertion_count(P, N, r.n, 70, CP, CN, 0, None, st) == -1           # (no output: nothing to look at)
    w = [Guarded(8, torch.int64, -7) for _ in range(2)] + [Guarded(80, torch.int32, -7)] + [Guarded(8, torch.int32, -7) for _ in range(2)]
    q = [b.ptr for b in w]                                             # out_ptr, out_keys, out_nodes, out_parent, out_cand
    vp = torch.tensor([0, 4, 8], dtype=torch.int64, device=DEV)
    ep = torch.tensor([0, 24, 24 + 4 * 71], dtype=torch.int64, device=DEV)
    VP, EP = ops._ptr(vp), ops._ptr(ep)
    refused += [
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, -4, q[0], q[2], q[3], q[4], q[1], st),          # negative sizes
        lib.sgnn_insertion_write(P, N, -1, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, -70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, 2 ** 31, q[0], q[2], q[3], q[4], q[1], st),     # variants above 2^31 - 1
        lib.sgnn_insertion_write(P, N, 2 ** 31, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 3, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),           # shared
        lib.sgnn_insertion_write(None, N, r.n, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),        # null inputs
        lib.sgnn_insertion_write(P, None, r.n, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, None, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, None, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, None, EP, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, None, 4, q[0], q[2], q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, 4, None, q[2], q[3], q[4], q[1], st),           # a null output
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, 4, q[0], None, q[3], q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], None, q[4], q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], None, q[1], st),
        lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], None, st),
        lib.sgnn_insertion_write(P, N, 0, 70, CP, CN, 0, VP, EP, 4, q[0], q[2], q[3], q[4], q[1], st),             # variants of no set
    ]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert all(b.untouched() for b in [out] + w)
    # no variants to write: nothing is written, and that is no error
    assert lib.sgnn_insertion_write(P, N, r.n, 70, CP, CN, 0, VP, EP, 0, None, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in w)
    with pytest.raises(ValueError):
        ops.insertion_sets(r, c, shared=True)
    bad = ops.Ragged(c.ptr, c.nodes, max_len=4)
    bad.ptr = c.ptr.int()                                              # (the constructor refuses them: set behind it)
    with pytest.raises(TypeError):
        ops.insertion_sets(r, bad)

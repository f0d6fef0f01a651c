"""-m gpu: the seeded walk kernel (sgnn_seeded_walk_sets, ops.seeded_walk_sets) against the numpy definition of
tests/discover_cases.py, bit for bit in all four outputs: every size alone and all mixed in one call, the three restart
thresholds, the three step limits, clamped sizes, more items than one trip of the grid-stride loop, chunks by ``item_base`` and a
shuffled list of ``item_ids`` against the whole call.  The entry is called directly with guard words around every output; refused
calls write nothing; a call on another stream gives the same bits."""
import numpy as np
import pytest
import torch

import discover_cases as DC
from test_gpu_insertion import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIELDS = ('nodes', 'len', 'steps', 'keys')


@pytest.fixture(scope='module')
def graph():
    """The cases' graph on the device -> (ops.DeviceGraph, rowptr, col_sorted tensors)."""
    from subgnn_amd import ops
    rowptr, col = DC.graph()
    g = ops.DeviceGraph(rowptr, col, np.arange(1, DC.MAX_ID + 1), torch.device(DEV))
    assert torch.equal(g.col_sorted.cpu(), torch.from_numpy(col))
    return g


def _dev(a, dtype):
    t = torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)
    return t if t.numel() else torch.zeros(1, dtype=dtype, device=DEV)          # (a tensor of no elements has no address)


def _run_entry(g, c, item_base=0, n_items=None, item_ids=None, seed=DC.SEED, stream=DC.STREAM):
    """The entry on guarded outputs -> dict of numpy arrays."""
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    seeds, sizes = _dev(c['seeds'], torch.int32), _dev(c['sizes'], torch.int32)
    ids = None if item_ids is None else _dev(item_ids, torch.int64)
    n = len(item_ids) if item_ids is not None else (len(c['seeds']) * c['per_seed'] - item_base if n_items is None else n_items)
    W = c['width']
    out = {'nodes': Guarded(n * W, torch.int32, -7), 'len': Guarded(n, torch.int32, -7), 'steps': Guarded(n, torch.int32, -7),
           'keys': Guarded(n, torch.int64, -7)}
    rc = lib.sgnn_seeded_walk_sets(ops._ptr(g.rowptr), ops._ptr(g.col_sorted), g.max_id, ops._ptr(seeds), len(c['seeds']),
                                   ops._ptr(sizes), c['per_seed'], W, c['restart_thr'], c['max_steps'], seed, stream, item_base,
                                   ops._ptr(ids), n, out['nodes'].ptr, out['len'].ptr, out['steps'].ptr, out['keys'].ptr,
                                   ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, b in out.items():
        assert b.intact(), 'guard words of ' + k
    got = {k: b.t.cpu().numpy() for k, b in out.items()}
    got['nodes'], got['keys'] = got['nodes'].reshape(n, W), got['keys'].view(np.uint64)
    return got


def _check(got, want, what, rows=None):
    for k in FIELDS:
        w = want[k] if rows is None else want[k][rows]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        assert np.array_equal(got[k], w), (what, k)


@pytest.mark.parametrize('name', list(DC.CASES))
def test_every_case_bit_for_bit(graph, name):
    _check(_run_entry(graph, DC.CASES[name]), DC.expected(name), name)


def test_chunks_and_item_lists_give_the_rows_of_the_whole_call(graph):
    c, whole = DC.CASES['mixed'], DC.expected('mixed')
    n = DC.n_items('mixed')
    half = n // 2 + 1
    _check(_run_entry(graph, c, 0, half), whole, 'first half', slice(0, half))
    _check(_run_entry(graph, c, half, n - half), whole, 'second half', slice(half, n))
    ids = np.random.default_rng(1).permutation(n)[:40]
    got = _run_entry(graph, c, item_ids=ids.tolist() + [n, -1, 10 ** 12])
    _check({k: v[:40] for k, v in got.items()}, whole, 'item_ids', ids)
    assert not got['nodes'][40:].any() and got['len'][40:].tolist() == [0] * 3 and got['steps'][40:].tolist() == [0] * 3
    from subgnn_amd import tape
    assert got['keys'][40:].tolist() == [tape.set_key_np([])] * 3
    # the many case in two chunks on either side of the grid's edge
    c, whole = DC.CASES['many'], DC.expected('many')
    n = DC.n_items('many')
    _check(_run_entry(graph, c, DC.GRID_CAP - 1, n - DC.GRID_CAP + 1), whole, 'many, tail', slice(DC.GRID_CAP - 1, n))


def test_another_seed_or_stream_changes_the_sets(graph):
    c, whole = DC.CASES['mixed'], DC.expected('mixed')
    for kw in (dict(seed=DC.SEED + 1), dict(stream=DC.STREAM + 1)):
        got = _run_entry(graph, c, **kw)
        assert not np.array_equal(got['keys'], whole['keys']) and np.array_equal(got['len'] == 0, whole['len'] == 0)


def _ops_case(name):
    """A case as ops.seeded_walk_sets takes it: the seeds that are node ids, the width the largest size."""
    c = dict(DC.CASES[name])
    c['seeds'] = np.array([s for s in c['seeds'] if 1 <= s <= DC.MAX_ID], dtype=np.int32)
    assert c['width'] == int(c['sizes'].max())
    rowptr, col = DC.graph()
    return c, DC.sample(rowptr, col, seed=DC.SEED, stream=DC.STREAM, **c)


@pytest.mark.parametrize('name', ['mixed', 'size 65', 'restart_thr 0'])
def test_ops_gives_the_same(graph, name):
    from subgnn_amd import ops
    c, want = _ops_case(name)
    seeds = torch.from_numpy(c['seeds']).to(DEV)
    kw = dict(sizes=c['sizes'].tolist(), per_seed=c['per_seed'], restart=c['restart_thr'] / 2.0 ** 32, seed=DC.SEED, stream_id=DC.STREAM)
    assert ops.restart_threshold(kw['restart']) == c['restart_thr']
    results = [ops.seeded_walk_sets(graph, seeds, **kw)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        results.append(ops.seeded_walk_sets(graph, seeds, **kw))
    side.synchronize()
    torch.cuda.synchronize()
    n = len(want['len'])
    for o in results:
        assert o.nodes.dtype == o.lengths.dtype == o.steps.dtype == torch.int32 and o.keys.dtype == torch.int64
        got = {'nodes': o.nodes.cpu().numpy(), 'len': o.lengths.cpu().numpy(), 'steps': o.steps.cpu().numpy(),
               'keys': o.keys.cpu().numpy().view(np.uint64)}
        _check(got, want, name + ' (ops)')
    # sets: the rows as a Ragged (every seed is a node: none is empty), keyed as ops.set_keys keys them
    o = results[0]
    rows = [want['nodes'][i, :want['len'][i]].tolist() for i in range(n)]
    assert o.sets.n == n and o.sets.to_lists() == rows and o.sets.max_len == int(want['len'].max())
    assert torch.equal(ops.set_keys(o.sets), o.keys)
    # chunks and an item list, the list with ids that are no items: their rows are empty and ``sets`` leaves them out
    half = n // 2
    a, b = ops.seeded_walk_sets(graph, seeds, n_items=half, **kw), ops.seeded_walk_sets(graph, seeds, item_base=half, **kw)
    assert torch.equal(torch.cat([a.nodes, b.nodes]), o.nodes) and torch.equal(torch.cat([a.keys, b.keys]), o.keys)
    ids = np.random.default_rng(2).permutation(n)[:9].tolist()
    picked = ops.seeded_walk_sets(graph, seeds, item_ids=torch.tensor(ids[:4] + [n, -1] + ids[4:], device=DEV), **kw)
    keep = [0, 1, 2, 3, 6, 7, 8, 9, 10]
    assert picked.lengths.tolist() == [int(want['len'][q]) for q in ids[:4]] + [0, 0] + [int(want['len'][q]) for q in ids[4:]]
    assert torch.equal(picked.nodes[keep], o.nodes[ids]) and torch.equal(picked.keys[keep], o.keys[ids])
    assert picked.sets.to_lists() == [rows[q] for q in ids] and torch.equal(ops.set_keys(picked.sets), picked.keys[keep])
    empty = ops.seeded_walk_sets(graph, seeds, item_base=n, **kw)
    assert empty.nodes.shape == (0, c['width']) and empty.sets.n == 0
    with pytest.raises(ValueError, match='ids outside'):
        ops.seeded_walk_sets(graph, torch.tensor([1, DC.MAX_ID + 1], dtype=torch.int32, device=DEV), (4,))


def test_refused_calls_write_nothing(graph):
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    c = DC.CASES['size 3']
    seeds, sizes = _dev(c['seeds'], torch.int32), _dev(c['sizes'], torch.int32)
    ids = _dev([0, 1], torch.int64)
    w = [Guarded(64, torch.int32, -7), Guarded(8, torch.int32, -7), Guarded(8, torch.int32, -7), Guarded(8, torch.int64, -7)]
    R, C, S, Z, I, st = ops._ptr(graph.rowptr), ops._ptr(graph.col_sorted), ops._ptr(seeds), ops._ptr(sizes), ops._ptr(ids), ops._stream()
    n_seeds, M = len(c['seeds']), graph.max_id

    def call(rowptr=R, col=C, max_id=M, seeds=S, n_seeds=n_seeds, sizes=Z, per_seed=2, width=3, thr=0, max_steps=5, item_base=0,
             item_ids=None, n_items=2, outs=None):
        o = [b.ptr for b in w] if outs is None else outs
        return lib.sgnn_seeded_walk_sets(rowptr, col, max_id, seeds, n_seeds, sizes, per_seed, width, thr, max_steps, DC.SEED,
                                         DC.STREAM, item_base, item_ids, n_items, o[0], o[1], o[2], o[3], st)
    refused = [
        call(max_id=-1), call(n_seeds=-1), call(n_items=-1), call(item_base=-1), call(max_steps=-1),       # negative counts
        call(width=0), call(width=DC.MAX_SIZE + 1), call(per_seed=0), call(per_seed=-2),
        call(thr=2 ** 32 + 1), call(n_items=2 ** 31), call(max_steps=2 ** 31),
        call(item_base=2 * n_seeds - 1, n_items=2), call(item_base=2 * n_seeds + 1, n_items=0),            # beyond n_seeds * per_seed
        call(rowptr=None), call(col=None), call(seeds=None), call(sizes=None),                             # null pointers with work
    ] + [call(outs=[None if j == i else b.ptr for j, b in enumerate(w)]) for i in range(4)]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert all(b.untouched() for b in w)
    # no items: nothing is written, and that is no error, whatever the pointers
    assert call(n_items=0) == 0 and call(n_items=0, item_ids=I) == 0
    assert lib.sgnn_seeded_walk_sets(None, None, M, None, n_seeds, None, 2, 3, 0, 5, 0, 0, 0, None, 0, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in w)
    # the same call, accepted: with an item list the item_base does not count
    assert call(item_ids=I, item_base=10 ** 9, thr=c['restart_thr'], max_steps=c['max_steps']) == 0
    torch.cuda.synchronize()
    want = DC.expected('size 3')
    assert w[1].t[:2].tolist() == want['len'][:2].tolist() and all(b.intact() for b in w)

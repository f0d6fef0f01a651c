"""CPU: the host side of the seeded walk sets and of subgnn_amd/discover.py -- the numpy definition's cases reach every outcome
of a walk and every lane-boundary size, its sets are what the header promises (seed inside, ascending, connected, keyed by
content), chunks and item lists reproduce the whole call, the neighbour draw is uniform, the kernel's limits are the restated
ones, the header's declarations, the argument checks of the entry and of ops.seeded_walk_sets, the CLI's argument rules and
line format, and the rank order.  No GPU."""
import os
import re
import types

import numpy as np
import pytest

import discover_cases as DC

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _rows(name):
    """(item, seed, size, members, steps) of every item of a case."""
    c, e = DC.CASES[name], DC.expected(name)
    for q in range(DC.n_items(name)):
        size = min(max(int(c['sizes'][q % c['per_seed']]), 1), c['width'])
        yield q, int(c['seeds'][q // c['per_seed']]), size, e['nodes'][q, :e['len'][q]].tolist(), int(e['steps'][q])


def test_the_graph_is_what_the_cases_need():
    rowptr, col = DC.graph()
    assert len(rowptr) == DC.MAX_ID + 2 <= 402 and rowptr[0] == rowptr[1] == 0 and rowptr[-1] == len(col)
    deg = np.diff(rowptr)
    assert deg[DC.HUB] >= 300 and all(deg[v] == 4 for v in DC.K5) and deg[DC.PATH[0]] == 1 and deg[DC.PATH[4]] == 2
    assert col[rowptr[DC.LOOP]:rowptr[DC.LOOP + 1]].tolist() == [DC.LOOP]
    assert deg[DC.BARE] == 0 and deg[DC.MAX_ID] == 0 and [int(deg[v]) for v in DC.TRIPLE] == [1, 2, 1]
    assert 3.5 <= float(np.mean(deg[DC.SPARSE]) - 1) <= 4.5                         # without the hub's edge
    rows = np.repeat(np.arange(DC.MAX_ID + 1), deg)
    assert bool(((np.diff(col) > 0) | (np.diff(rows) > 0)).all()) and col.min() >= 1 and col.max() <= DC.MAX_ID
    pairs = set(zip(rows.tolist(), col.tolist()))
    assert all((b, a) in pairs for a, b in pairs)                                   # every edge in both rows


def test_the_cases_reach_every_outcome():
    seen = set()
    for name in DC.CASES:
        c = DC.CASES[name]
        for q, s, size, members, steps in _rows(name):
            if not 1 <= s <= DC.MAX_ID:
                assert members == [] and steps == 0
                seen.add('seed out of range')
            elif DC.degree(s) == 0:
                assert members == [s] and steps == 0
                seen.add('degree 0')
            elif len(members) == size:
                seen.add('full size')
                if size >= 63:
                    seen.add('full size %d' % size)
            elif steps == c['max_steps']:
                seen.add('stopped by max_steps')
            else:
                raise AssertionError((name, q, 'neither full nor out of steps'))
            if int(c['sizes'][q % c['per_seed']]) != size:
                seen.add('clamped')
    assert seen == {'seed out of range', 'degree 0', 'full size', 'stopped by max_steps', 'clamped'} | \
        {'full size %d' % n for n in DC.SIZES if n >= 63}
    # a component smaller than the size is exhausted: the walk holds all of it and runs out of steps
    e, c = DC.expected('size 64'), DC.CASES['size 64']
    for q, s, size, members, steps in _rows('size 64'):
        if s == DC.TRIPLE[0]:
            assert members == DC.TRIPLE and steps == c['max_steps']
        if s == DC.LOOP:
            assert members == [DC.LOOP] and steps == c['max_steps']
    assert e['nodes'].shape == (2 * len(DC.SEEDS), 64)
    # the clamped sizes walk as 1, 4, 4, 2
    assert [size for _q, _s, size, _m, _t in list(_rows('clamped'))[:4]] == [1, 4, 4, 2]
    assert DC.n_items('many') > DC.GRID_CAP


@pytest.mark.parametrize('name', list(DC.CASES))
def test_every_set_of_the_definition_is_a_connected_set_around_its_seed(name):
    from subgnn_amd import tape
    rowptr, col = DC.graph()
    e = DC.expected(name)
    assert e['nodes'].dtype == e['len'].dtype == e['steps'].dtype == np.int32 and e['keys'].dtype == np.uint64
    every = 1 if DC.n_items(name) < 1000 else 37
    for q, s, size, members, steps in _rows(name):
        assert not e['nodes'][q, len(members):].any()
        if not members or q % every:
            continue
        assert s in members and len(members) <= size and members == sorted(set(members))
        assert DC.connected(rowptr, col, members), (name, q)
        assert int(e['keys'][q]) == tape.set_key_np(members)
    assert int(DC.expected('size 1')['keys'][-1]) == tape.set_key_np([])              # (seed -5: the empty set)


def test_a_certain_restart_never_leaves_the_seed():
    name = 'restart_thr %d' % (1 << 32)
    for q, s, size, members, steps in _rows(name):
        if 1 <= s <= DC.MAX_ID and DC.degree(s) > 0:
            assert members == [s] and steps == DC.CASES[name]['max_steps']
    assert any(len(m) > 1 for _q, _s, _n, m, _t in _rows('restart_thr 0'))


def test_chunks_and_item_lists_give_the_rows_of_the_whole_call():
    rowptr, col = DC.graph()
    c, whole = DC.CASES['mixed'], DC.expected('mixed')
    n = DC.n_items('mixed')
    half = n // 2 + 1
    a = DC.sample(rowptr, col, seed=DC.SEED, stream=DC.STREAM, item_base=0, n_items=half, **c)
    b = DC.sample(rowptr, col, seed=DC.SEED, stream=DC.STREAM, item_base=half, n_items=n - half, **c)
    ids = np.random.default_rng(1).permutation(n)[:40].tolist() + [n, -1, 10 ** 12]
    picked = DC.sample(rowptr, col, seed=DC.SEED, stream=DC.STREAM, item_ids=ids, **c)
    for k in whole:
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
        assert np.array_equal(picked[k][:40], whole[k][ids[:40]]), k
    assert picked['len'][40:].tolist() == [0, 0, 0] and picked['steps'][40:].tolist() == [0, 0, 0]
    # another tape seed or stream gives other sets
    other = DC.sample(rowptr, col, seed=DC.SEED + 1, stream=DC.STREAM, **c)
    assert not np.array_equal(other['keys'], whole['keys'])
    other = DC.sample(rowptr, col, seed=DC.SEED, stream=DC.STREAM + 1, **c)
    assert not np.array_equal(other['keys'], whole['keys'])


def test_the_neighbour_draw_is_uniform():
    """One step without restart from a node of degree 4, 4096 times: every neighbour is taken 1024 times in the mean, with
    sigma = sqrt(4096 * 1/4 * 3/4) = 27.7; 900 .. 1150 is about +-4.5 sigma."""
    rowptr, col = DC.graph()
    s = DC.K5[0]
    e = DC.sample(rowptr, col, np.array([s], dtype=np.int32), np.full(4096, 2, dtype=np.int32), 4096, 2, 0, 1, DC.SEED, DC.STREAM)
    assert e['len'].tolist() == [2] * 4096 and e['steps'].tolist() == [1] * 4096
    taken = e['nodes'].sum(axis=1) - s
    counts = [int((taken == v).sum()) for v in DC.K5[1:]]
    print('neighbours taken:', counts)
    assert sum(counts) == 4096 and all(900 <= k <= 1150 for k in counts), counts


def test_the_restated_limits_are_the_sources():
    txt = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'seeded_sets.hip')).read()
    assert int(re.search(r'#define SGNN_SEEDED_MAX_SIZE (\d+)', txt).group(1)) == DC.MAX_SIZE == max(DC.SIZES) == 256
    assert int(re.search(r'#define SGNN_SEEDED_GRID_CAP (\d+)', txt).group(1)) == DC.GRID_CAP
    assert re.search(r'sgnn_grid_for\(n_items, 1, SGNN_SEEDED_GRID_CAP\)\), dim3\(SGNN_WAVE\)', txt)      # one item per workgroup
    from subgnn_amd import ops, tape
    assert ops.SEEDED_MAX_SIZE == DC.MAX_SIZE and tape.STREAM_DISCOVER == 13
    assert DC.THR_DEFAULT == ops.restart_threshold(0.15)


def test_the_new_symbols_are_declared_and_bound():
    from subgnn_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    assert re.search(r'\bint64_t sgnn_seeded_walk_max_size\s*\(void\)', txt) and re.search(r'\bint sgnn_seeded_walk_sets\s*\(', txt)
    assert 'sgnn_seeded_walk_max_size' in _lib.SIGNATURES and len(_lib.SIGNATURES['sgnn_seeded_walk_sets'][1]) == 20
    assert '#define SGNN_ABI_VERSION 14' in txt
    lib = _lib.load()
    assert lib.sgnn_abi_version() == 14 and lib.sgnn_seeded_walk_max_size() == DC.MAX_SIZE
    # refused on the host, before any launch (no pointer is read): the arguments after the graph's are
    # (seeds, n_seeds, sizes, per_seed, width, restart_thr, max_steps, seed, stream, item_base, item_ids, n_items, outputs x 4, stream)
    call = lambda *a: lib.sgnn_seeded_walk_sets(None, None, 10, None, *a, None, None, None, None, None)
    assert call(2, None, 3, 8, 0, 5, 0, 0, 0, None, 0) == 0                             # nothing to do
    assert call(-1, None, 3, 8, 0, 5, 0, 0, 0, None, 0) == -1                           # negative counts
    assert call(2, None, 3, 8, 0, -5, 0, 0, 0, None, 0) == -1
    assert call(2, None, 3, 8, 0, 5, 0, 0, -1, None, 0) == -1
    assert call(2, None, 3, 8, 0, 5, 0, 0, 0, None, -1) == -1
    assert call(2, None, 3, 0, 0, 5, 0, 0, 0, None, 0) == -1                            # width
    assert call(2, None, 3, 257, 0, 5, 0, 0, 0, None, 0) == -1
    assert call(2, None, 0, 8, 0, 5, 0, 0, 0, None, 0) == -1                            # per_seed
    assert call(2, None, 3, 8, 2 ** 32 + 1, 5, 0, 0, 0, None, 0) == -1                  # restart_thr
    assert call(2, None, 3, 8, 2 ** 32, 5, 0, 0, 0, None, 0) == 0
    assert call(2, None, 3, 8, 0, 5, 0, 0, 0, None, 2 ** 31) == -1                      # n_items
    assert call(2, None, 3, 8, 0, 5, 0, 0, 6, None, 1) == -1                            # items beyond n_seeds * per_seed
    assert call(2, None, 3, 8, 0, 5, 0, 0, 7, None, 0) == -1
    assert call(2, None, 3, 8, 0, 5, 0, 0, 6, None, 0) == 0
    assert call(2, None, 3, 8, 0, 5, 0, 0, 0, None, 6) == -1                            # null pointers with work to do
    assert lib.sgnn_seeded_walk_sets(None, None, -1, None, 2, None, 3, 8, 0, 5, 0, 0, 0, None, 0, None, None, None, None, None) == -1


def _fake(dtype, n, dim=1):
    """What ops._req reads of a tensor, without a device."""
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, is_contiguous=lambda: True, numel=lambda: n, dim=lambda: dim,
                                 min=lambda: 1, max=lambda: 5)


def test_seeded_walk_sets_checks_its_arguments_before_any_library_call(monkeypatch):
    import torch
    from subgnn_amd import ops, _lib

    def no_call():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_call)
    g = types.SimpleNamespace(max_id=9, device='cpu')
    seeds = _fake(torch.int32, 3)
    for kw in (dict(sizes=()), dict(sizes=(0,)), dict(sizes=(4, 257)), dict(sizes=(2.5,)), dict(sizes=(True,)),
               dict(sizes=(4,), per_seed=0), dict(sizes=(4,), per_seed=1.5), dict(sizes=(4,), restart=-0.1),
               dict(sizes=(4,), restart=1.5), dict(sizes=(4,), restart=float('nan')), dict(sizes=(4,), max_steps=-1),
               dict(sizes=(4,), max_steps=2 ** 31), dict(sizes=(4,), item_base=-1), dict(sizes=(4,), n_items=-1),
               dict(sizes=(4,), item_base=2, n_items=2), dict(sizes=(4, 4), item_base=7),
               dict(sizes=(4,), item_ids=_fake(torch.int64, 2), n_items=2), dict(sizes=(4,), item_ids=_fake(torch.int64, 2), item_base=1),
               dict(sizes=(4,), item_ids=_fake(torch.int64, 4, dim=2))):
        with pytest.raises(ValueError):
            ops.seeded_walk_sets(g, seeds, **kw)
    with pytest.raises(ValueError, match='ids outside 1 .. 4'):
        ops.seeded_walk_sets(types.SimpleNamespace(max_id=4, device='cpu'), seeds, (4,))
    with pytest.raises(ValueError, match='one-dimensional'):
        ops.seeded_walk_sets(g, _fake(torch.int32, 4, dim=2), (4,))
    for bad in (dict(seeds=_fake(torch.int64, 3)), dict(seeds=seeds, item_ids=_fake(torch.int32, 2))):
        with pytest.raises(TypeError):
            ops.seeded_walk_sets(g, sizes=(4,), **bad)
    with pytest.raises(AssertionError, match='the library was loaded'):               # what is well formed goes on to the library
        ops.seeded_walk_sets(g, seeds, (4, 8), per_seed=3, restart=1.0, max_steps=0, item_base=2, n_items=7)
    assert [ops.restart_threshold(p) for p in (0, 0.5, 1, 1.0 - 2.0 ** -40)] == [0, 2 ** 31, 2 ** 32, 2 ** 32 - 1]


# ---- ranking ----------------------------------------------------------------------------------------------------------------------
def test_the_rank_order_ties_and_nan():
    from subgnn_amd import discover
    nan = float('nan')
    score = [0.5, 2.0, nan, 2.0, -1.0, 2.0, nan]
    item = [9, 30, 1, 20, 4, 25, 0]
    order = discover.rank_order(score, item).tolist()
    assert order == [3, 5, 1, 0, 4, 6, 2]                              # descending score, ties by ascending item, NaN last (by item)
    assert discover.rank_order([], []).tolist() == []
    assert discover.rank_order(np.array([1.0, 1.0], dtype=np.float32), [5, 3]).tolist() == [1, 0]
    # ten items per seed: the ranked candidates belong to seeds 2, 2, 3, 0, 0, 0, 0.  At most n of every seed, then the first N
    seed_index = [q // 10 for q in item]
    assert [seed_index[u] for u in order] == [2, 2, 3, 0, 0, 0, 0]
    assert discover.select(order, seed_index).tolist() == order
    assert discover.select(order, seed_index, top=3).tolist() == [3, 5, 1]
    assert discover.select(order, seed_index, top_per_seed=2).tolist() == [3, 5, 1, 0, 4]
    assert discover.select(order, seed_index, top_per_seed=1).tolist() == [3, 1, 0]
    assert discover.select(order, seed_index, top=2, top_per_seed=1).tolist() == [3, 1]
    assert discover.select([], [], top=3, top_per_seed=1).tolist() == []


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
BASE = ['-config_path', 'c.json', '-restoreModelPath', 'run', '-seeds', 'in.txt', '-out', 'out.txt']


def test_cli_argument_rules():
    from subgnn_amd import discover
    a = discover.parse_args(BASE)
    assert (a.seeds, a.target, a.sizes, a.per_seed, a.restart, a.max_steps, a.draws, a.top, a.top_per_seed, a.novel, a.batch_size,
            a.sample_seed, a.restoreModelName) == ('in.txt', None, [8], 16, 0.15, None, 1, 100, None, False, None, None, None)
    a = discover.parse_args(BASE[:4] + ['-seeds', 'all', '-out', 'o.txt', '-target', 'lab', '-sizes', '5,10,20', '-per_seed', '6',
                                        '-restart', '0', '-max_steps', '0', '-draws', '4', '-top', '3', '-top_per_seed', '2', '-novel',
                                        '-batch_size', '8', '-sample_seed', '7'])
    assert (a.seeds, a.target, a.sizes, a.per_seed, a.restart, a.max_steps, a.draws, a.top, a.top_per_seed, a.novel, a.batch_size,
            a.sample_seed) == ('all', 'lab', [5, 10, 20], 6, 0.0, 0, 4, 3, 2, True, 8, 7)
    for bad in (['-draws', '0'], ['-top', '0'], ['-top_per_seed', '0'], ['-batch_size', '-2'], ['-per_seed', '0'], ['-draws', 'x'],
                ['-sizes', '0'], ['-sizes', '4,257'], ['-sizes', '4,,5'], ['-sizes', 'a'], ['-restart', '1.5'], ['-restart', '-0.1'],
                ['-restart', 'nan'], ['-max_steps', '-1']):
        with pytest.raises(SystemExit):
            discover.parse_args(BASE + bad)
    with pytest.raises(SystemExit):                                   # distinct files
        discover.parse_args(BASE[:-1] + ['in.txt'])
    with pytest.raises(SystemExit):
        discover.parse_args(BASE[2:])


def test_cli_line_format():
    import torch
    from subgnn_amd import discover
    assert discover.HEADER == 'rank\tseed\tscore\tscore_std\tprob\tsubgraph\tlabel\tknown'
    x = np.float32(0.1)
    line = discover.format_line(0, 17, x, np.float32(0.0), np.float32(0.25), [3, 17, 40], ['a'], True)
    assert line == '0\t17\t0.100000001\t0\t0.25\t3-17-40\ta\t1'
    assert np.float32(float(line.split('\t')[2])) == x                # 9 digits: a float32 survives the round trip
    assert discover.format_line(2, np.int64(4), 1.5, 0.5, 0.125, [4], ['a', 'b'], np.bool_(False)) == '2\t4\t1.5\t0.5\t0.125\t4\ta-b\t0'

    class P:
        @staticmethod
        def names_of(row):
            return ['L%d' % int(row)]

    res = {'seed': torch.tensor([5, 2]), 'score': torch.tensor([1.0, 0.25]), 'score_std': torch.zeros(2), 'prob': torch.tensor([0.5, 0.2]),
           'known': torch.tensor([False, True]), 'labels': torch.tensor([1, 0]), 'subgraphs': [[5, 6], [1, 2, 9]]}
    assert discover.lines_of(P, res) == ['0\t5\t1\t0\t0.5\t5-6\tL1\t0', '1\t2\t0.25\t0\t0.200000003\t1-2-9\tL0\t1']
    for bad in (dict(per_seed=0), dict(draws=0), dict(top=0), dict(top_per_seed=1.5), dict(batch_size=0), dict(max_variants=0)):
        with pytest.raises(ValueError):
            discover.discover(None, [1], **bad)

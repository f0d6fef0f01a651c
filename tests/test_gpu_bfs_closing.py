"""-m gpu: the closing form of the set search (ops.bfs_min_hops_to_sets(until='sets'): sgnn_bfs_min_hops_to_sets_closing) and the
component labels it rests on (DeviceGraph.component_labels: sgnn_graph_component_labels).  "Equal" is torch.equal against the
default form run to its end; where a dense hop table is cheap also against ops.bfs_hops + ops.min_hops_to_sets."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ops():
    from subgnn_amd import ops
    return ops


def _graph(pairs, n):
    """Undirected graph on ids 1..n from 1-based pairs -> (DeviceGraph, rowptr, col)."""
    from subgnn_amd import synthetic
    ops = _ops()
    e = np.asarray(pairs, dtype=np.int64).reshape(-1, 2) - 1
    rowptr, col = synthetic.sorted_csr(e, n)
    return ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV), rowptr, col


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int32)).to(DEV)


def _both(dg, src, sets, **kw):
    """-> (values, status as a list) of the closing form"""
    ops = _ops()
    w, st = ops.bfs_min_hops_to_sets(dg, src, sets, want_status=True, until='sets', **kw)
    return w, st.tolist()


def _full(dg, src, sets, max_hops=64):
    ops = _ops()
    ref, st = ops.bfs_min_hops_to_sets(dg, src, sets, max_hops=max_hops, want_status=True)
    st = st.tolist()
    assert st[1] == 0
    assert torch.equal(ref, ops.min_hops_to_sets(ops.bfs_hops(dg, src, max_hops=max_hops), sets))
    return ref, st


# ---- labels ----------------------------------------------------------------------------------------------------------------

def _union_find_labels(pairs, n):
    parent = list(range(n + 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(n + 1)], dtype=np.int32)


def _label_cases():
    rng = np.random.default_rng(7)
    rand = rng.integers(1, 2001, (1500, 2))                                   # many components, isolated ids
    stars = [(1, i) for i in range(2, 40)] + [(100, i) for i in range(40, 100)] + [(39, 99)]      # two stars joined at leaves
    chain = [(i, i + 1) for i in range(1, 300)]
    return {'random': (rand, 2000), 'stars': (stars, 120), 'chain': (chain, 300)}


@pytest.mark.parametrize('case', ['random', 'stars', 'chain'])
def test_component_labels_equal_a_host_union_find(case):
    pairs, n = _label_cases()[case]
    dg, _, _ = _graph(pairs, n)
    got = dg.component_labels()
    assert got.dtype == torch.int32 and got.shape == (n + 1,)
    want = _union_find_labels(pairs, n)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(got[0]) == 0                                                   # the pad id labels itself
    assert dg.component_labels() is got                                       # built once per graph
    if case == 'random':
        assert len(set(want.tolist())) > 100 and (want[1:] == np.arange(1, n + 1)).sum() > 100
    if case == 'stars':
        assert set(want[1:101].tolist()) == {1} and want[110] == 110


# ---- closure really happens -------------------------------------------------------------------------------------------------

def test_the_search_closes_before_the_graph_is_done():
    """BA n = 20 000, m = 4: node depth 6 from the 183 sources, every set has its hops at level 4 (174 of the 300 sets are
    still open before it)."""
    from subgnn_amd import synthetic
    ops = _ops()
    n = 20000
    rowptr, col = synthetic.sorted_csr(synthetic.barabasi_albert_edges(n, 4, seed=9), n)
    dg = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV)
    sets = ops.Ragged.from_lists(synthetic.bfs_subgraphs(rowptr, col, 300, 20, seed=5), DEV)
    src = _t(np.random.default_rng(3).choice(n, 183, replace=False) + 1)
    ref, st = _full(dg, src, sets, 32)
    assert st[0] == 6                                                         # the default form still runs the graph's depth
    w, cs = _both(dg, src, sets, max_hops=32)
    assert torch.equal(w, ref)
    if cs[2] and cs[2] <= 4:                                                  # level 4 pulled
        assert cs[:2] == [4, 0], cs
    else:
        assert cs[1] == 0 and 4 <= cs[0] <= 5, cs
    # the forms the pass runs: levels and push levels from the first search's status
    w, cs = _both(dg, src, sets, max_hops=4 + 3, push_levels=st[2])
    assert torch.equal(w, ref) and cs[:2] == [4, 0]
    w, cs = _both(dg, src, sets, max_hops=4 + 3, push_levels=1)              # every level from 2 on pulls
    assert torch.equal(w, ref) and cs[:3] == [4, 0, 2]


# ---- chain ------------------------------------------------------------------------------------------------------------------

def test_chain_closes_near_the_sources_unless_a_set_holds_the_far_end():
    dg, _, _ = _graph([(i, i + 1) for i in range(1, 64)], 64)
    ops = _ops()
    src = _t([1, 2])
    near = [[2, 3], [3], [1, 4], [4]]
    sets = ops.Ragged.from_lists(near, DEV)
    ref, st = _full(dg, src, sets)
    assert st[0] == 63
    w, cs = _both(dg, src, sets, max_hops=64)
    assert torch.equal(w, ref) and cs[1] == 0 and 2 <= cs[0] <= 3, cs
    sets = ops.Ragged.from_lists(near + [[64]], DEV)
    ref, st = _full(dg, src, sets)
    w, cs = _both(dg, src, sets, max_hops=64)
    assert torch.equal(w, ref) and cs[:2] == [63, 0] and st[0] == 63
    assert ref[4].tolist() == [63.0, 62.0]


# ---- disconnected graph -----------------------------------------------------------------------------------------------------

def test_disconnected_graph_every_kind_of_set():
    """Two components (a chain 1..30, a ring 41..60 with a tail 60..70), isolated ids 31..40 and 71..80; sources of both
    components and an isolated one in the same word."""
    ops = _ops()
    pairs = [(i, i + 1) for i in range(1, 30)] + [(i, i + 1) for i in range(41, 70)] + [(41, 60)]
    dg, _, _ = _graph(pairs, 80)
    src = _t([1, 45, 35, 15, 70])                         # chain end, ring, isolated, chain middle, tail end
    sets_l = [[3, 4],                                      # inside the first sources' component
              [50, 51],                                    # in the other component
              [5, 50],                                     # spanning two components: all 0
              [33],                                        # an isolated member
              [35],                                        # the isolated source itself
              [],                                          # empty
              [10, 12], [12, 29],                          # share a member; the first closes levels before the second
              [2, 33],                                     # a component and an isolated id: all 0
              [66, 68]]
    sets = ops.Ragged.from_lists(sets_l, DEV)
    ref, st = _full(dg, src, sets)
    w, cs = _both(dg, src, sets, max_hops=64)
    assert torch.equal(w, ref) and cs[1] == 0 and cs[0] < st[0], (cs, st)
    r = ref.cpu().numpy()
    assert r[0].tolist() == [2, 0, 0, 11, 0] and r[1].tolist() == [0, 5, 0, 0, 19]
    assert not r[2].any() and not r[3].any() and not r[4].any() and not r[5].any() and not r[8].any()
    assert r[6].tolist() == [9, 0, 0, 3, 0] and r[7].tolist() == [11, 0, 0, 3, 0]
    for alpha in (0, 1):
        for cap in (-1, 1):
            w, cs = _both(dg, src, sets, max_hops=64, pull_alpha=alpha, push_levels=cap)
            assert torch.equal(w, ref) and cs[1] == 0, (alpha, cap)
    # nothing is wanted at all: closed before the first level
    sets = ops.Ragged.from_lists([[5, 50], [], [33]], DEV)
    w, cs = _both(dg, src, sets, max_hops=64)
    assert not w.any() and cs[:2] == [0, 0]
    assert torch.equal(w, _full(dg, src, sets)[0])


# ---- source counts: row strides 1, 1, 2 and 4 ------------------------------------------------------------------------------------

_star_cache = []


def _star_with_tail():
    """A star of 600 leaves (ids 2..601 around 1: a list the pull levels park for the whole workgroup) whose leaves carry a
    BA tail (ids 602..3000); sets of leaves and tail nodes, and in front of them the centre alone."""
    if not _star_cache:
        from subgnn_amd import synthetic
        n = 3000
        ba = synthetic.barabasi_albert_edges(n - 601, 3, seed=4) + 601          # 0-based ids 601.. = 1-based 602..3000
        pairs = [(1, i) for i in range(2, 602)] + [(int(a) + 1, int(b) + 1) for a, b in ba]
        pairs += [(i, 602 + 4 * (i - 2)) for i in range(2, 602)]                # every leaf has one tail neighbour
        rng = np.random.default_rng(12)
        sets_l = [[1]] + [rng.integers(2, n + 1, int(rng.integers(1, 12))).tolist() for _ in range(150)] + [[], [2, 3000]]
        _star_cache.append((pairs, n, sets_l))
    return _star_cache[0]


@pytest.mark.parametrize('n_src', [1, 64, 65, 183])
def test_source_counts_on_a_star_with_a_tail(n_src):
    ops = _ops()
    pairs, n, sets_l = _star_with_tail()
    dg, rowptr, _ = _graph(pairs, n)
    assert rowptr[2] - rowptr[1] >= 600
    src = _t(np.random.default_rng(n_src).choice(np.arange(602, n + 1), n_src, replace=False))
    # with and without the centre alone as a set (the pull levels park its list for the whole workgroup)
    for first in (0, 1):
        sets = ops.Ragged.from_lists(sets_l[first:], DEV)
        ref, st = _full(dg, src, sets)
        for cap in (1, 2):
            w, cs = _both(dg, src, sets, max_hops=32, pull_alpha=1 << 30, push_levels=cap)
            assert torch.equal(w, ref), (first, cap)
            assert cs[1] == 0 and cs[0] <= st[0] and cs[2] == 2, cs          # (alpha 2^30: pulls from level 2 on)


# ---- direction and caps -----------------------------------------------------------------------------------------------------

def test_values_do_not_depend_on_direction_or_push_cap():
    from subgnn_amd import synthetic
    ops = _ops()
    n = 6000
    rowptr, col = synthetic.sorted_csr(synthetic.barabasi_albert_edges(n - 50, 6, seed=9), n)      # ids n-49..n are isolated
    dg = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV)
    src = np.random.default_rng(70).integers(1, n + 1 - 50, 70).astype(np.int32)
    src[0] = n                                                                  # an isolated source
    src = _t(src)
    rng = np.random.default_rng(1)
    sets_l = [rng.integers(1, n + 1 - 50, int(rng.integers(1, 30))).tolist() for _ in range(400)]
    sets_l[5] = []
    sets_l[6] = [n - 3, 17]
    sets = ops.Ragged.from_lists(sets_l, DEV)
    ref, st = _full(dg, src, sets, 32)
    closing = set()
    for alpha in (0, 1, 256, 1 << 30):
        for cap in (-1, 1, 2, 3):
            w, cs = _both(dg, src, sets, max_hops=32, pull_alpha=alpha, push_levels=cap)
            assert torch.equal(w, ref), (alpha, cap)
            assert cs[1] == 0 and cs[0] <= st[0]
            if alpha == 0:
                assert cs[2] == 0                                               # closes in push mode
            closing.add(cs[0])
    assert len(closing) == 1 and closing.pop() < st[0]                          # the closing level is a property of the search


# ---- max_hops ---------------------------------------------------------------------------------------------------------------

def test_level_cap_at_around_and_below_the_closing_level():
    from subgnn_amd import synthetic
    ops = _ops()
    n = 20000
    rowptr, col = synthetic.sorted_csr(synthetic.barabasi_albert_edges(n, 4, seed=9), n)
    dg = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV)
    sets = ops.Ragged.from_lists(synthetic.bfs_subgraphs(rowptr, col, 300, 20, seed=5), DEV)
    src = _t(np.random.default_rng(3).choice(n, 183, replace=False) + 1)
    ref, _ = ops.bfs_min_hops_to_sets(dg, src, sets, max_hops=32, want_status=True)
    c = 4
    for push in (-1, 1):
        w, cs = _both(dg, src, sets, max_hops=c, push_levels=push)
        assert cs[:2] == [c, 0] and torch.equal(w, ref), push                 # the cap is the closing level
        w, cs = _both(dg, src, sets, max_hops=c - 1, push_levels=push)
        assert cs[:2] == [c - 1, 1], push                                      # one level short
        assert not torch.equal(w, ref)
        w, cs = _both(dg, src, sets, max_hops=c + 3, push_levels=push)
        assert cs[:2] == [c, 0] and torch.equal(w, ref), push


# ---- model level ------------------------------------------------------------------------------------------------------------

def _same(x, y, where=''):
    if isinstance(x, torch.Tensor):
        assert torch.equal(x, y), where
    elif isinstance(x, dict):
        assert set(x) == set(y), where
        for k in x:
            _same(x[k], y[k], '%s/%s' % (where, k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), where
        for i, (p, q) in enumerate(zip(x, y)):
            _same(p, q, '%s/%d' % (where, i))
    elif hasattr(x, 'dense'):
        _same(x.dense(), y.dense(), where)


def _pass_models(capturable):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
    from bench import ALL_DENSITY_HP
    from subgnn_amd import synthetic, optim
    from subgnn_amd.SubGNN import SubGNN
    ops = _ops()
    n, S = 20000, 500
    rowptr, col = synthetic.sorted_csr(synthetic.barabasi_albert_edges(n, 4, seed=9), n)
    g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV)
    subs = synthetic.bfs_subgraphs(rowptr, col, S, 20, seed=5)
    hp = dict(ALL_DENSITY_HP, lin_dropout=0.0, lstm_dropout=0.0)
    emb = torch.randn(n, hp['node_embed_size'], generator=torch.Generator().manual_seed(0)).to(DEV)
    labels = torch.randint(0, 3, (S,), generator=torch.Generator().manual_seed(0))
    out = []
    for until in ('sets', 'nodes'):
        torch.manual_seed(0)
        m = SubGNN.from_memory(dict(hp, position_search_until=until), g, {'train': subs, 'val': [], 'test': []},
                               {'train': labels, 'val': labels[:0], 'test': labels[:0]}, emb.clone(), num_classes=3)
        m.train()
        out.append((m, optim.ClipAdam(m.parameters(), hp['learning_rate'], max_norm=hp['grad_clip'], capturable=capturable)))
    return out


def test_prepared_state_is_the_same_with_either_search_eager():
    from subgnn_amd import hotpath
    (ms, _), (mn, _) = _pass_models(False)
    for k in range(3):                                      # the first pass at the cap, then hinted ones
        a, b = hotpath.prepare_pass(ms, 'train'), hotpath.prepare_pass(mn, 'train')
        torch.cuda.synchronize()
        if k:                                               # the hint settles at closing level + margin + 1 enqueued levels
            assert a.bfs_checks and all(enq == ms._bfs_level_hint[key] + hotpath.BFS_LEVEL_MARGIN + 1 and int(host[0]) == ms._bfs_level_hint[key]
                                        for key, host, _, _, enq, _ in a.bfs_checks)
        _same(a.attrs, b.attrs, 'attrs %d' % k)
        _same(a.per_split, b.per_split, 'per_split %d' % k)
        hotpath.install_pass(ms, a)
        hotpath.install_pass(mn, b)
    L = ms.hparams['n_layers']
    assert all(ms._bfs_level_hint[('P_out', 'train', l)] < mn._bfs_level_hint[('P_out', 'train', l)] for l in range(L))
    assert not ms.__dict__.get('_bfs_redone') and not mn.__dict__.get('_bfs_redone')
    ms.hparams['position_search_until'] = 'neither'
    with pytest.raises(ValueError):
        hotpath.prepare_pass(ms, 'train')


def test_prepared_state_is_the_same_with_either_search_recorded():
    from subgnn_amd import hotpath
    (ms, os_), (mn, on) = _pass_models(True)
    ps, pn = hotpath.GraphedPasses(ms, os_, 'train', warmup=2), hotpath.GraphedPasses(mn, on, 'train', warmup=2)
    for k in range(6):                                      # two eager passes, a recording per slot, two replays
        ls, _ = ps.step()
        ln, _ = pn.step()
        torch.cuda.synchronize()
        assert torch.equal(ls, ln), k
    assert ps.recordings == 2 and pn.recordings == 2
    for i in range(2):
        _same(ps.slots[i].state.attrs, pn.slots[i].state.attrs, 'slot %d attrs' % i)
        _same(ps.slots[i].state.per_split, pn.slots[i].state.per_split, 'slot %d per_split' % i)
    for (name, a), (_, b) in zip(ms.named_parameters(), mn.named_parameters()):
        assert torch.equal(a, b), name

"""GPU: ops.subgraph_properties (csrc/subgraph_props.hip) and subgnn_amd.subgraph_properties against networkx, exactly: the
structural cases and tier edges of tests/subgraph_props_cases.py, the reference's own recipe outputs (tests/golden/recipes.npz)
and the dataset driver."""
import json
import os

import networkx as nx
import numpy as np
import pytest
import torch

import subgraph_props_cases as SC

from subgnn_amd import ops
from subgnn_amd import prepare_dataset as pd
from subgnn_amd import subgraph_properties as SP
from subgnn_amd.graph import networkx_order_csr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_GRAPHS = {}


def device_graph(name):
    if name not in _GRAPHS:
        g = SC.graph(name)
        order = np.nonzero(np.diff(g.rowptr) > 0)[0].astype(np.int32)          # the ids that are nodes: G.nodes
        dg = ops.DeviceGraph(g.rowptr, g.col, order, DEV)
        assert dg.simple_rows == g.simple_rows and dg.n_nodes == g.G.number_of_nodes() and dg.max_id == g.max_id
        _GRAPHS[name] = dg
    return _GRAPHS[name]


def run(graph_name, cases, want_core=True):
    dg = device_graph(graph_name)
    sets = ops.Ragged.from_lists([c.nodes for c in cases], DEV)
    counts, core = ops.subgraph_properties(dg, sets, want_core=want_core)
    torch.cuda.synchronize()
    ptr = sets.ptr.cpu().tolist()
    core = core.cpu().tolist() if core is not None else None
    return counts.cpu().numpy(), [core[ptr[i]:ptr[i + 1]] for i in range(len(cases))] if core is not None else None


def check(cases, counts, core):
    for i, c in enumerate(cases):
        want_counts, want_core = SC.expected(c.name)
        print(c.name, SC.tier(len(c.nodes)), 'counts', counts[i].tolist(), 'want', want_counts)
        assert counts[i].tolist() == want_counts, (c.name, counts[i].tolist(), want_counts)
        if core is not None:
            bad = [(p, a, b) for p, (a, b) in enumerate(zip(core[i], want_core)) if a != b]
            assert not bad, (c.name, bad[:10])


@pytest.mark.parametrize('graph_name', ['zoo', 'zoo_repeats'])
def test_structural_cases(graph_name):
    cases = SC.cases_of(graph_name)
    counts, core = run(graph_name, cases)
    check(cases, counts, core)
    # one set at a time too: a launch of a single wavefront
    for c in cases[:6]:
        k, cr = run(graph_name, [c])
        check([c], k, cr)


def test_values_on_the_structural_cases_and_self_loops():
    g, dg = SC.graph('zoo'), device_graph('zoo')
    cases = SC.cases_of('zoo')
    lists = [c.nodes for c in cases]
    for prop in ('density', 'cut_ratio', 'cc'):
        got = SP.values(dg, lists, prop)
        for c, v in zip(cases, got):
            w = SC.oracle_value(g.G, c.nodes, prop)
            assert (np.isnan(v) and np.isnan(w)) or v == w, (c.name, prop, v, w)
    whole = next(i for i, c in enumerate(cases) if c.name == 'whole-graph')
    assert np.isnan(SP.values(dg, lists, 'cut_ratio')[whole])                   # N - n = 0
    first_loop = next(i for i, c in enumerate(cases) if SC.expected(c.name)[0][2] > 0)
    with pytest.raises(ValueError, match='subgraph %d ' % first_loop):
        SP.values(dg, lists, 'coreness')
    got = SP.values(dg, ops.Ragged.from_lists(lists, DEV), 'coreness', ignore_self_loops=True)
    K = nx.Graph(g.G)
    K.remove_edges_from(list(nx.selfloop_edges(K)))
    for c, v in zip(cases, got):
        w = SC.oracle_value(K, c.nodes, 'coreness')
        assert (np.isnan(v) and np.isnan(w)) or v == w, (c.name, v, w)


def test_a_hub_list_is_searched_not_streamed():
    from subgnn_amd import _lib
    c = next(x for x in SC.cases() if x.name == 'hub-list')
    deg = np.diff(SC.graph('ba').rowptr)
    assert deg[c.nodes[0]] >= _lib.load().sgnn_degree_sequence_search_threshold() == SC.SEARCH_THRESHOLD
    counts, core = run('ba', [c])
    check([c], counts, core)


@pytest.mark.parametrize('graph_name', ['ba', 'ba_repeats'])
def test_tier_edges_and_every_tier_in_one_call_twice(graph_name):
    cases = SC.cases_of(graph_name)
    assert {SC.tier(len(c.nodes)) for c in cases} == set(SC.TIERS)
    first = run(graph_name, cases)
    check(cases, *first)
    # again, in another order and on memory the first call has used: neither LDS nor the workspace carries anything over
    again = run(graph_name, cases[::-1])
    check(cases[::-1], *again)
    counts, core = run(graph_name, cases, want_core=False)
    assert core is None and np.array_equal(counts, first[0])


def test_each_tier_alone():
    for t in SC.TIERS:
        cases = [c for c in SC.cases_of('ba') if SC.tier(len(c.nodes)) == t][:3]
        counts, core = run('ba', cases)
        check(cases, counts, core)


def test_bad_arguments_return_the_error_code():
    from subgnn_amd import _lib
    lib = _lib.load()
    dg = device_graph('zoo')
    big = ops.Ragged.from_lists([list(range(1, 41)) * 60], DEV)                 # 2400 entries: the workspace tier
    out = torch.empty((1, 6), dtype=torch.int64, device=DEV)
    p = lambda t: t.data_ptr()
    assert lib.sgnn_subgraph_properties(None, None, 0, 0, 1, None, None, 0, 1, 0, None, None, None, 0, None) == -1
    # a set beyond the LDS tier without a workspace
    assert lib.sgnn_subgraph_properties(p(dg.rowptr), p(dg.col_sorted), dg.nnz, dg.max_id, 1, p(big.ptr), p(big.nodes), 1, 2400, 2400,
                                        p(out), None, None, 0, None) == -1
    assert lib.sgnn_subgraph_properties_workspace_bytes(2400) == 2400 * 44 + 64
    counts, core = ops.subgraph_properties(dg, big)
    want, want_core = SC.oracle_counts(SC.graph('zoo').G, list(range(1, 41)) * 60)
    assert counts.cpu().tolist() == [want] and core.cpu().tolist() == want_core


def _recipe_device(z, name):
    t = name + '/'
    kw = json.loads(str(z[t + 'kwargs']))
    rowptr, col, order = networkx_order_csr(z[t + 'edges'])                     # 0-based file ids -> 1-based device ids
    dg = ops.DeviceGraph(rowptr, col, order, DEV)
    subs = [[int(v) + 1 for v in row if v != -1] for row in z[t + 'subgraphs']]
    return kw, dg, subs, [str(l) for l in z[t + 'labels']]


@pytest.mark.parametrize('name', ['density', 'cut_ratio', 'coreness', 'cc', 'density_b'])
def test_labels_are_the_references_on_its_recipe_outputs(name):
    z = np.load(os.path.join(GOLDEN_DIR, 'recipes.npz'), allow_pickle=False)
    kw, dg, subs, stored = _recipe_device(z, name)
    assert dg.n_nodes == len(z[name + '/nodes'])
    letters, vals = SP.labels(dg, subs, kw['desired_property'], kw['n_bins'])
    print(name, 'sizes', min(map(len, subs)), max(map(len, subs)), 'agree', sum(a == b for a, b in zip(letters, stored)), len(stored))
    assert letters == stored
    letters_r, _ = SP.labels(dg, ops.Ragged.from_lists(subs, DEV), kw['desired_property'], kw['n_bins'])
    assert letters_r == stored


def test_label_dataset_returns_the_labels_write_dataset_wrote(tmp_path):
    out, info = pd.write_dataset(str(tmp_path / 'ds'), 'density', n=300, n_subgraphs=40)
    src = os.path.join(str(out), 'subgraphs.pth')
    before = open(src).read()
    path, summary = SP.label_dataset(str(out), 'density', device=DEV)
    assert path == os.path.join(str(out), 'subgraphs_density.pth') and open(src).read() == before
    old = [l.split('\t') for l in before.splitlines(True)]
    new = [l.split('\t') for l in open(path)]
    assert len(new) == len(old) > 0
    assert [l[0] for l in new] == [l[0] for l in old] and [l[2:] for l in new] == [l[2:] for l in old]
    assert [l[1] for l in new] == [l[1] for l in old]
    assert summary['histogram'] == {k: [l[1] for l in old].count(k) for k in sorted({l[1] for l in old})}
    assert summary['sets_with_dropped_ids'] == 0 and summary['n_subgraphs'] == len(old)
    assert SP.main([str(out), '--property', 'cc', '--out', str(tmp_path / 'cc.pth')]) == 0
    assert len(open(tmp_path / 'cc.pth').read().splitlines()) == len(old)

"""CPU: the cases of tests/test_gpu_subgraph_props.py reach every tier and branch of subgraph_props.hip, the host expressions of
subgnn_amd.subgraph_properties on integer counts are networkx's values bit for bit, the binning is prepare_dataset.labels_of's,
and label_dataset round-trips a dataset directory (the device call stubbed by the networkx counts)."""
import json
import math
import os
import re

import networkx as nx
import numpy as np
import pytest

import subgraph_props_cases as SC

from subgnn_amd import prepare_dataset as pd
from subgnn_amd import subgraph_properties as SP

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GOLDEN_DIR = os.path.join(REPO, 'tests', 'golden')
RECIPES = ('density', 'cut_ratio', 'coreness', 'cc', 'density_b')


def _same(a, b):
    """bit-equal floats (nan == nan)"""
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1, a) == math.copysign(1, b))


def test_constants_are_the_kernels():
    # the library's tiering has one definition (id_table.h), and the kernel files use it instead of bounds of their own
    src = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'id_table.h')).read()
    assert int(re.search(r'#define SGNN_SET_WAVE_MAX (\d+)', src).group(1)) == SC.WAVE_MAX
    assert int(re.search(r'#define SGNN_SET_LDS_MAX (\d+)', src).group(1)) == SC.LDS_MAX
    for name in ('subgraph_props.hip', 'graph_sets.hip', 'degree_sequence.hip'):
        user = open(os.path.join(REPO, 'subgnn_amd', 'csrc', name)).read()
        assert '#include "id_table.h"' in user and 'SGNN_SET_LDS_MAX' in user
        assert not re.search(r'#define (SP_WAVE_MAX|SP_LDS_MAX|CC_MAX|DSB_MAX|PB_MAX)\b', user), name
    ds = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'degree_sequence.hip')).read()
    assert int(re.search(r'#define DS_SEARCH (\d+)', ds).group(1)) == SC.SEARCH_THRESHOLD
    from subgnn_amd import ops
    assert ops.CC_LDS_MAX == SC.LDS_MAX


def test_every_tier_and_branch_is_reached():
    tiers, reached = set(), set()
    names = [c.name for c in SC.cases()]
    assert len(set(names)) == len(names)
    for c in SC.cases():
        tiers.add(SC.tier(len(c.nodes)))
        reached |= SC.branches(c)
    assert tiers == set(SC.TIERS)
    assert reached == set(SC.BRANCHES), set(SC.BRANCHES) ^ reached
    sizes = {len(c.nodes) for c in SC.cases()}
    assert {SC.WAVE_MAX - 1, SC.WAVE_MAX, SC.WAVE_MAX + 1, SC.LDS_MAX, SC.LDS_MAX + 1} <= sizes
    # rows that repeat an id, dropped ids and repeats are met in every tier (the wave and the workgroup forms differ there)
    for t in SC.TIERS:
        here = [SC.branches(c) for c in SC.cases() if SC.tier(len(c.nodes)) == t]
        for b in ('rows_not_simple', 'repeat', 'dropped_pad', 'dropped_beyond_max_id', 'dropped_empty_row', 'self_loop'):
            assert any(b in s for s in here), (t, b)
    c65 = next(c for c in SC.cases() if c.name == 'n65-64-distinct')
    assert len(c65.nodes) == 65 and len(set(c65.nodes)) == 64


def test_structural_cases_are_what_their_names_say():
    want = {'K1': (1, 0, 1, 0), 'K2': (2, 1, 1, 2), 'K5': (5, 10, 1, 20), 'star6': (6, 5, 1, 6), 'path4': (4, 3, 1, 4),
            'cycle5': (5, 5, 1, 10), 'two-K4-joined': (8, 13, 1, 24), 'two-triangles-and-isolated': (7, 6, 3, 12),
            'empty': (0, 0, 0, 0), 'only-dropped': (0, 0, 0, 0), 'repeats': (4, 6, 1, 12)}
    for name, (n, m, cc, cs) in want.items():
        counts, core = SC.expected(name)
        assert (counts[0], counts[1], counts[4], counts[5]) == (n, m, cc, cs), name
    assert SC.expected('K5')[1] == [4] * 5 and SC.expected('star6')[1] == [1] * 6 and SC.expected('cycle5')[1] == [2] * 5
    assert SC.expected('dropped-inside')[1] == [-1, 3, 3, -1, 3, -1, 3, 3]
    assert SC.expected('self-loop')[0][2] == 1
    assert not SC.graph('zoo_repeats').simple_rows and not SC.graph('ba_repeats').simple_rows and SC.graph('ba').simple_rows


@pytest.mark.parametrize('graph_name', ['zoo', 'zoo_repeats', 'ba', 'ba_repeats'])
def test_host_expressions_equal_networkx_bit_for_bit(graph_name):
    g = SC.graph(graph_name)
    cs = SC.cases_of(graph_name)
    counts = np.asarray([SC.expected(c.name)[0] for c in cs], dtype=np.int64)
    N = g.G.number_of_nodes()
    for prop in ('density', 'cut_ratio', 'cc'):
        got = SP.values_from_counts(counts, prop, N)
        for c, v in zip(cs, got):
            w = SC.oracle_value(g.G, c.nodes, prop)
            assert _same(v, w), (c.name, prop, v, w)
    assert SP.values_from_counts(counts, 'cc', N).dtype == np.int64
    loops = [i for i, c in enumerate(cs) if counts[i, 2] > 0]
    clean = [i for i in range(len(cs)) if i not in loops]
    got = SP.values_from_counts(counts[clean], 'coreness', N)
    for i, v in zip(clean, got):
        assert _same(v, SC.oracle_value(g.G, cs[i].nodes, 'coreness')), cs[i].name
    if loops:
        # networkx refuses these; so does values() -- naming the first -- unless told to leave the loops out
        with pytest.raises(nx.NetworkXException):
            pd.coreness(g.G, cs[loops[0]].nodes)
        with pytest.raises(ValueError, match='subgraph %d ' % loops[0]):
            SP.values_from_counts(counts, 'coreness', N)
        got = SP.values_from_counts(counts, 'coreness', N, ignore_self_loops=True)
        K = nx.Graph(g.G)
        K.remove_edges_from(list(nx.selfloop_edges(K)))
        for c, v in zip(cs, got):
            assert _same(v, SC.oracle_value(K, c.nodes, 'coreness')), c.name


def _recipe(z, name):
    t = name + '/'
    kw = json.loads(str(z[t + 'kwargs']))
    G = nx.Graph()
    G.add_nodes_from(int(v) for v in z[t + 'nodes'])
    G.add_edges_from((int(u), int(v)) for u, v in z[t + 'edges'])
    subs = [[int(v) for v in row if v != -1] for row in z[t + 'subgraphs']]
    return kw, G, subs, [str(l) for l in z[t + 'labels']]


@pytest.mark.parametrize('name', RECIPES)
def test_binning_is_labels_of_on_the_recipe_fixtures(name):
    z = np.load(os.path.join(GOLDEN_DIR, 'recipes.npz'), allow_pickle=False)
    kw, G, subs, stored = _recipe(z, name)
    prop = kw['desired_property']
    want, vals = pd.labels_of(G, subs, prop, kw['n_bins'])
    assert want == stored                                           # networkx on the fixture reproduces the reference's labels
    counts = np.asarray([SC.oracle_counts(G, s)[0] for s in subs], dtype=np.int64)
    got = SP.values_from_counts(counts, prop, G.number_of_nodes())
    assert all(_same(a, b) for a, b in zip(got, vals))
    assert SP.letters_of(got, prop, kw['n_bins']) == stored


def test_label_dataset_round_trips_through_read_subgraphs(tmp_path, monkeypatch):
    from subgnn_amd.subgraph_utils import read_subgraphs
    G = nx.barabasi_albert_graph(60, 3, seed=2)
    nx.write_edgelist(G, str(tmp_path / 'edge_list.txt'), data=False)
    rng = np.random.RandomState(4)
    subs = [SC.bfs_prefix(G, int(rng.randint(60)), int(rng.randint(4, 12))) for _ in range(30)]
    subs[5] = subs[5] + [75, 90]                                    # ids that are no nodes of the graph
    splits = ['train'] * 20 + ['val'] * 4 + ['test'] * 6
    with open(tmp_path / 'subgraphs.pth', 'w') as f:
        for s, sp in zip(subs, splits):
            f.write('\t'.join(['-'.join(str(v) for v in s), 'X', sp, '\n']))
    before = open(tmp_path / 'subgraphs.pth').read()

    def nx_counts(g, lists):                                        # the device call, by networkx (device ids are file ids + 1)
        assert g.n_nodes == G.number_of_nodes() and g.max_id == max(G.nodes) + 1
        return np.asarray([SC.oracle_counts(G, [v - 1 for v in s])[0] for s in lists], dtype=np.int64)

    monkeypatch.setattr(SP, 'counts', nx_counts)
    for prop in SP.PROPERTIES:
        path, summary = SP.label_dataset(str(tmp_path), prop, device='cpu')
        assert path == str(tmp_path / ('subgraphs_%s.pth' % prop))
        assert open(tmp_path / 'subgraphs.pth').read() == before    # the input is never overwritten
        want, vals = pd.labels_of(G, subs, prop, 3)
        lines = [l.split('\t') for l in open(path)]
        assert [l[0] for l in lines] == ['-'.join(str(v) for v in s) for s in subs]
        assert [l[1] for l in lines] == want and [l[2] for l in lines] == splits
        assert summary['histogram'] == {k: want.count(k) for k in sorted(set(want))}
        assert summary['value_min'] == min(vals) and summary['value_max'] == max(vals)
        assert summary['sets_with_dropped_ids'] == 1 and summary['n_subgraphs'] == 30
        tr, trl, va, val, te, tel = read_subgraphs(path)
        assert tr == subs[:20] and len(va) + len(te) == 10
    with pytest.raises(ValueError):
        SP.label_dataset(str(tmp_path), 'density', out=str(tmp_path / 'subgraphs.pth'), device='cpu')
    with pytest.raises(ValueError):
        SP.values_from_counts(np.zeros((1, 6)), 'diameter', 10)

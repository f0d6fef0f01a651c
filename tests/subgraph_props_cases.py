"""Test helpers of the subgraph-property kernel (subgnn_amd/csrc/subgraph_props.hip through ``ops.subgraph_properties``): the
graphs and sets tests/test_gpu_subgraph_props.py runs, what networkx says about them, and a restatement of the kernel's tier
dispatch and of the branches a set reaches, so that tests/test_subgraph_props_host.py can say without a GPU that every tier
and every branch is reached by some case.  numpy + networkx only; nothing here reads the GPU.

Ids are the device's: 1-based, 0 = PAD.  A graph is (max_id, rowptr, col, G): the CSR the DeviceGraph is built from and the
networkx graph of its distinct edges (nodes = the ids with a non-empty row), which is the oracle."""
import functools
import warnings
from collections import namedtuple

import networkx as nx
import numpy as np

# ---- the constants the dispatch depends on (the host test reads the #defines out of csrc/id_table.h and compares) ------------
WAVE_MAX = 64                           # #define SGNN_SET_WAVE_MAX 64: entries one wavefront takes
LDS_MAX = 2048                          # #define SGNN_SET_LDS_MAX 2048: entries the workgroup form keeps in LDS (== ops.CC_LDS_MAX)
SEARCH_THRESHOLD = 512                  # sgnn_degree_sequence_search_threshold(): a list this long is a "hub" list

TIERS = ('wave', 'lds', 'workspace')
BRANCHES = ('empty_set', 'only_dropped', 'dropped_pad', 'dropped_beyond_max_id', 'dropped_empty_row', 'repeat', 'self_loop',
            'rows_not_simple', 'hub_list', 'whole_graph', 'isolated_member', 'components>1', 'core>1', 'pairs_rounds>1')


def tier(n_entries):
    """The kernel that owns a set, by its number of ENTRIES (dropped ids and repeats included)."""
    return 'wave' if n_entries <= WAVE_MAX else ('lds' if n_entries <= LDS_MAX else 'workspace')


Graph = namedtuple('Graph', 'max_id rowptr col G simple_rows')
Case = namedtuple('Case', 'name graph nodes')


def make_graph(max_id, edges, keep_repeats=False):
    """edges: (u, v) pairs, undirected, 1-based; a pair listed twice stays twice in both rows when ``keep_repeats``; a self
    loop is one entry of its row (what graph.networkx_order_csr writes)."""
    rows = [[] for _ in range(max_id + 1)]
    for u, v in edges:
        rows[u].append(v)
        if u != v:
            rows[v].append(u)
    rows = [sorted(r) if keep_repeats else sorted(set(r)) for r in rows]
    rowptr = np.zeros(max_id + 2, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.asarray([x for r in rows for x in r], dtype=np.int32)
    G = nx.Graph()
    G.add_edges_from((u, v) for u, v in edges)
    simple = all(len(r) == len(set(r)) for r in rows)
    return Graph(max_id, rowptr, col, G, simple)


# ---- the graphs ---------------------------------------------------------------------------------------------------------------
def _clique(ids):
    return [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]]


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == 'zoo':
        # K5 1-5 | star 6 (7-11) | path 12-15 | cycle 16-20 | two K4 21-24, 25-28 joined by 24-25 | triangles 29-31, 32-34 |
        # K2 35-36 | 37 with a self loop, tied to 38 | 39: no edges (an empty row) | 40 tied to 1; max_id = 40
        e = _clique([1, 2, 3, 4, 5]) + [(6, k) for k in range(7, 12)] + [(12, 13), (13, 14), (14, 15)]
        e += [(16, 17), (17, 18), (18, 19), (19, 20), (20, 16)]
        e += _clique([21, 22, 23, 24]) + _clique([25, 26, 27, 28]) + [(24, 25)]
        e += _clique([29, 30, 31]) + _clique([32, 33, 34]) + [(35, 36), (37, 37), (37, 38), (40, 1)]
        e += [(5, 6), (11, 12), (15, 16), (20, 21), (28, 29), (34, 35), (36, 38)]      # ties between the pieces: boundary edges
        return make_graph(40, e)
    if name == 'zoo_repeats':
        # the zoo with some pairs listed twice or three times: rows that repeat an id (DeviceGraph.simple_rows False)
        z = graph('zoo')
        e = list(z.G.edges())
        e += [(1, 2), (1, 2), (3, 4), (6, 7), (24, 25), (5, 6), (28, 29), (13, 14), (37, 38), (16, 20)]
        return make_graph(40, e, keep_repeats=True)
    if name in ('ba', 'ba_repeats'):
        # Barabasi-Albert, 3000 nodes, m = 4, plus a hub (id 3001) tied to 600 nodes: a list beyond the search threshold;
        # ids 3002 and 3003 have no edges, max_id = 3003
        B = nx.barabasi_albert_graph(3000, 4, seed=5)
        e = [(u + 1, v + 1) for u, v in B.edges()] + [(3001, k) for k in range(1, 1201, 2)]
        if name == 'ba_repeats':
            rng = np.random.RandomState(11)
            pick = rng.choice(len(e), size=len(e) // 15, replace=False)
            e += [e[i] for i in pick] + [e[i] for i in pick[:50]] + [(int(v), int(v)) for v in rng.choice(3000, 40, replace=False) + 1]
        return make_graph(3003, e, keep_repeats=(name == 'ba_repeats'))
    raise KeyError(name)


def bfs_prefix(G, root, k):
    """The first k nodes of a breadth-first search from ``root`` (a connected, locally dense set)."""
    out = [root]
    for _, v in nx.bfs_edges(G, root):
        if len(out) >= k:
            break
        out.append(v)
    return out[:k]


def _structural():
    z = 'zoo'
    return [
        Case('K1', z, [3]), Case('K2', z, [35, 36]), Case('K5', z, [1, 2, 3, 4, 5]), Case('star6', z, [6, 7, 8, 9, 10, 11]),
        Case('path4', z, [12, 13, 14, 15]), Case('cycle5', z, [16, 17, 18, 19, 20]),
        Case('two-K4-joined', z, list(range(21, 29))),
        Case('two-triangles-and-isolated', z, [29, 30, 31, 32, 33, 34, 36]),
        Case('whole-graph', z, [v for v in range(1, 41) if v != 39]),
        Case('empty', z, []), Case('only-dropped', z, [0, 41, 39, 0]),
        Case('repeats', z, [1, 2, 2, 3, 1, 4, 4, 4]),
        Case('dropped-inside', z, [0, 1, 2, 41, 3, 39, 4, 2]),
        Case('self-loop', z, [37, 38, 36]),
        Case('rows-repeat-K5', 'zoo_repeats', [1, 2, 3, 4, 5, 6, 7]),
        Case('rows-repeat-K4s', 'zoo_repeats', list(range(21, 30)) + [37, 38]),
    ]


def _hub_set():
    b = graph('ba')
    return [3001] + list(range(1, 20, 2)) + list(range(2, 20, 2))[:9]        # the hub, ten of its neighbours, nine others


def _mixed(base, n_entries, max_id):
    """``base`` stretched to n_entries with PAD, an id beyond max_id, an id with an empty row and repeats sprinkled in."""
    out = list(base)
    extra = [0, max_id + 1, max_id, base[0], base[len(base) // 2], 0, base[-1]]
    i = 0
    while len(out) < n_entries:
        out.insert((7 * i + 3) % (len(out) + 1), extra[i % len(extra)])
        i += 1
    return out[:n_entries]


def _tier_edges():
    b, r = graph('ba'), graph('ba_repeats')
    c = [Case('hub-list', 'ba', _hub_set())]
    for k, root in ((63, 10), (64, 200), (65, 1500)):
        c.append(Case('n%d' % k, 'ba', bfs_prefix(b.G, root, k)))
    s64 = bfs_prefix(b.G, 77, 64)
    c.append(Case('n65-64-distinct', 'ba', s64[:40] + [s64[7]] + s64[40:]))
    c.append(Case('n%d-last-lds' % LDS_MAX, 'ba', bfs_prefix(b.G, 3, LDS_MAX)))
    c.append(Case('n%d-first-workspace' % (LDS_MAX + 1), 'ba', bfs_prefix(b.G, 2999, LDS_MAX + 1)))
    c.append(Case('n2600-workspace', 'ba', bfs_prefix(b.G, 3001, 2600)))
    c.append(Case('n300-mixed', 'ba', _mixed(bfs_prefix(b.G, 41, 280), 300, b.max_id)))
    c.append(Case('n2200-mixed', 'ba', _mixed(bfs_prefix(b.G, 42, 2100), 2200, b.max_id)))
    c.append(Case('rows-repeat-n20', 'ba_repeats', bfs_prefix(r.G, 500, 20)))
    c.append(Case('rows-repeat-n100', 'ba_repeats', bfs_prefix(r.G, 9, 100)))
    c.append(Case('rows-repeat-n2100', 'ba_repeats', _mixed(bfs_prefix(r.G, 1000, 2090), 2100, r.max_id)))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_structural() + _tier_edges())


def cases_of(graph_name):
    return [c for c in cases() if c.graph == graph_name]


# ---- what networkx says ----------------------------------------------------------------------------------------------------------
def oracle_counts(G, nodes):
    """-> (the six counts, core number per position; -1 for an entry that is no node of G)."""
    H = G.subgraph(nodes)
    members = set(H.nodes)
    loops = list(nx.selfloop_edges(H))
    boundary = len(list(nx.edge_boundary(G, members, set(G.nodes).difference(members))))
    K = nx.Graph(H)
    K.remove_edges_from(list(nx.selfloop_edges(K)))
    core = nx.core_number(K)
    counts = [H.number_of_nodes(), H.number_of_edges() - len(loops), len(loops), boundary, nx.number_connected_components(H),
              sum(core.values())]
    return counts, [core.get(v, -1) for v in nodes]


@functools.lru_cache(maxsize=None)
def expected(case_name):
    c = next(x for x in cases() if x.name == case_name)
    return oracle_counts(graph(c.graph).G, c.nodes)


def oracle_value(G, nodes, prop):
    """``prepare_dataset.PROPERTY[prop]``, with nan where the reference's expression divides by zero or averages nothing."""
    from subgnn_amd import prepare_dataset as pd
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return pd.PROPERTY[prop](G, nodes)
    except ZeroDivisionError:
        return float('nan')


def branches(c):
    """The branches of the kernel (and of the host expressions) the set of case ``c`` reaches."""
    g = graph(c.graph)
    counts, core = expected(c.name)
    deg = np.diff(g.rowptr)
    is_node = [1 <= v <= g.max_id and deg[v] > 0 for v in c.nodes]
    members = [v for v, ok in zip(c.nodes, is_node) if ok]
    out = set()
    if len(c.nodes) == 0:
        out.add('empty_set')
    if len(c.nodes) and not members:
        out.add('only_dropped')
    if 0 in c.nodes:
        out.add('dropped_pad')
    if any(v > g.max_id for v in c.nodes):
        out.add('dropped_beyond_max_id')
    if any(1 <= v <= g.max_id and deg[v] == 0 for v in c.nodes):
        out.add('dropped_empty_row')
    if len(set(members)) < len(members):
        out.add('repeat')
    if counts[2] > 0:
        out.add('self_loop')
    if not g.simple_rows:
        out.add('rows_not_simple')
    if any(deg[v] >= SEARCH_THRESHOLD for v in members):
        out.add('hub_list')
    if members and counts[0] == g.G.number_of_nodes():
        out.add('whole_graph')
    if 0 in [x for x in core if x >= 0] and counts[0] > 1:
        out.add('isolated_member')
    if counts[4] > 1:
        out.add('components>1')
    if max(core + [0]) > 1:
        out.add('core>1')
    if len(c.nodes) <= WAVE_MAX and len(c.nodes) * (len(c.nodes) - 1) // 2 > 64:
        out.add('pairs_rounds>1')
    return out

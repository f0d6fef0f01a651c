"""ops.subgraph_properties on the benchmark's graph and sets (Barabasi-Albert, 1M nodes, m = 10; 50 000 BFS sets of 20 nodes,
built as bench.py builds them), timed in ONE process beside the two existing launches that make the same membership tests:

    python tools/subgraph_props_probe.py [--rounds 40] [--out profiles/subgraph_props_probe.json]

Every round runs ``ops.subgraph_properties``, ``ops.degree_sequence`` and ``ops.cc_labels`` once each, in turn, between
device events, after warmed calls.  Median, minimum and the 10 % / 90 % quantiles per launch go into the JSON, with the
yardstick (degree_sequence + cc_labels, neither of which this launch changes), the margin of 1.25 x the yardstick and whether
the new launch is inside it, and the label histogram of each of the four properties on those sets.  The counts are checked
against networkx on sampled sets first."""
import argparse
import json
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MARGIN = 1.25


def inputs(n, m, S, NX):
    import numpy as np
    import torch
    from subgnn_amd import ops, synthetic
    edges = synthetic.barabasi_albert_edges(n, m, seed=42)
    rowptr, col = synthetic.sorted_csr(edges, n)
    subs = synthetic.bfs_subgraphs(rowptr, col, S, NX, seed=1000)
    dev = torch.device('cuda:0')
    g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), dev)
    return g, ops.Ragged.from_lists(subs, dev), subs, (rowptr, col)


def check_sample(csr, subs, counts, core, ptr, picks):
    """the sampled sets against networkx (the induced graph and the boundary are read off the CSR rows of the members)"""
    import networkx as nx
    rowptr, col = csr
    for s in picks:
        nodes = subs[s]
        members = set(nodes)
        H = nx.Graph()
        H.add_nodes_from(members)
        boundary = 0
        for v in members:
            for u in set(col[rowptr[v]:rowptr[v + 1]].tolist()):
                if u in members:
                    H.add_edge(v, u)
                elif u != v:
                    boundary += 1
        cn = nx.core_number(H)
        want = [len(members), H.number_of_edges(), 0, boundary, nx.number_connected_components(H), sum(cn.values())]
        assert counts[s].tolist() == want, (s, counts[s].tolist(), want)
        assert core[ptr[s]:ptr[s + 1]].tolist() == [cn[v] for v in nodes], s


def measure(rounds, n, m, S, NX):
    import numpy as np
    import torch
    from subgnn_amd import ops
    from subgnn_amd import subgraph_properties as SP
    g, sets, subs, csr = inputs(n, m, S, NX)
    fns = {'subgraph_properties': lambda: ops.subgraph_properties(g, sets),
           'degree_sequence': lambda: ops.degree_sequence(g, sets),
           'cc_labels': lambda: ops.cc_labels(g, sets)}
    for f in fns.values():
        f(); f()
    counts, core = fns['subgraph_properties']()
    torch.cuda.synchronize()
    counts_h, core_h, ptr = counts.cpu().numpy(), core.cpu().numpy(), sets.ptr.cpu().numpy()
    rng = np.random.default_rng(5)
    picks = [int(v) for v in rng.integers(len(subs), size=200)]
    check_sample(csr, subs, counts_h, core_h, ptr, picks)
    ev = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    times = {}
    for name, pairs in ev.items():
        t = np.array([a.elapsed_time(b) for a, b in pairs])
        times[name] = {'median_ms': float(np.median(t)), 'min_ms': float(t.min()), 'p10_ms': float(np.quantile(t, 0.1)),
                       'p90_ms': float(np.quantile(t, 0.9)), 'rounds': int(t.size)}
    yard = times['degree_sequence']['median_ms'] + times['cc_labels']['median_ms']
    new = times['subgraph_properties']['median_ms']
    hist = {}
    for prop in SP.PROPERTIES:
        vals = SP.values_from_counts(counts_h, prop, g.n_nodes)
        hist[prop] = {'labels': dict(sorted(Counter(SP.letters_of(vals, prop)).items())),
                      'min': float(np.nanmin(vals)), 'max': float(np.nanmax(vals))}
    return {'what': 'tools/subgraph_props_probe.py: ops.subgraph_properties (counts and per-position cores) beside ops.degree_sequence '
                    'and ops.cc_labels on the same sets, one process; %d rounds, each launch once per round in turn, device '
                    'events, ms (the torch allocations of the outputs are inside the events of all three)' % rounds,
            'device': torch.cuda.get_device_name(0), 'graph': {'nodes': n, 'm': m, 'nnz': int(g.nnz)},
            'sets': {'n': sets.n, 'entries_each': NX}, 'sampled_sets_equal_to_networkx': len(picks), 'times': times,
            'yardstick_ms': yard, 'yardstick': 'degree_sequence + cc_labels medians (launches this change does not touch)',
            'margin': MARGIN, 'subgraph_properties_over_yardstick': new / yard, 'within_margin': bool(new <= MARGIN * yard),
            'label_histograms': hist}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--sets', type=int, default=50_000)
    ap.add_argument('--set-nodes', type=int, default=20)
    ap.add_argument('--out', default='profiles/subgraph_props_probe.json')
    a = ap.parse_args()
    r = measure(a.rounds, a.nodes, a.m, a.sets, a.set_nodes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(r, open(a.out, 'w'), indent=1)
    print(json.dumps(r, indent=1))

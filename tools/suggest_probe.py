#!/usr/bin/env python3
"""Add-one-candidate scoring, timed on the model of tools/predict_probe.py (BA 1M nodes / m = 10, prepared on the benchmark's
50k training subgraphs): ``Predictor.suggest(candidates='border')`` on ``k`` fresh BFS subgraphs of 20 nodes beside the route
there was before for the same variants -- the lists ``S + [v]`` written out in Python and sent through ``Predictor.predict`` in
chunks of the same size -- and the device expansion alone (``ops.insertion_sets``), with the number of variants (a one-hop
border on this graph has thousands of ids, so the variants are thousands per request).  Wall clock around device
synchronisations, milliseconds; the median of ``reps`` warm calls.  No threshold: nobody had measured either number.
    python tools/suggest_probe.py [reps] [out.json] [k]"""
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from subgnn_amd import hotpath, ops, suggest, synthetic
from subgnn_amd.SubGNN import SubGNN
from subgnn_amd.predict import Predictor

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = sys.argv[2] if len(sys.argv) > 2 else None
k = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
n, m, S, D = 1_000_000, 10, 50_000, 64
CHUNK = 16384             # variants per prepared chunk, both routes: a chunk's one-hop borders go through one device sort (< 2^31 ids)
dev = torch.device('cuda:0')


def stage(what):
    print('[suggest_probe] ' + what, file=sys.stderr, flush=True)


stage('building the graph')
edges = synthetic.barabasi_albert_edges(n, m, seed=42)
rowptr, col = synthetic.sorted_csr(edges, n)
train = synthetic.bfs_subgraphs(rowptr, col, S, 20, seed=1000)
requests = [[v - 1 for v in s] for s in synthetic.bfs_subgraphs(rowptr, col, k, 20, seed=3000)]      # dataset numbering
stage('preparing the model')
g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), dev)
torch.manual_seed(0)
hp = dict(bench.ALL_DENSITY_HP)
hp['node_embed_size'] = D
labels = torch.randint(0, 3, (S,), generator=torch.Generator().manual_seed(0))
model = SubGNN.from_memory(hp, g, {'train': train, 'val': [], 'test': []},
                           {'train': labels, 'val': labels[:0], 'test': labels[:0]}, torch.randn(n, D, device=dev), num_classes=3)
hotpath.prepare_sparse(model, 'train')
torch.cuda.synchronize()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(fn):
    return round(statistics.median(wall(fn) for _ in range(reps)), 3)


def add_one(lists, borders):
    return [s + [v] for s, b in zip(lists, borders) for v in b]


def predict_lists(lists):
    for lo in range(0, len(lists), CHUNK):
        P.predict(lists[lo:lo + CHUNK])


stage('the candidates')
P = Predictor(model)
P.predict(requests)                                                   # the freeze, the code objects
sets = P.request_sets(requests)
rows, shared = suggest.candidate_rows(P, sets, 'border', 1)
mapped = [[v - 1 for v in s] for s in sets.to_lists()]
borders = [[v - 1 for v in b if v - 1 not in set(s)] for b, s in zip(rows.to_lists(), mapped)]
variants = add_one(mapped, borders)
res = {'graph_nodes': n, 'graph_m': m, 'train_subgraphs': S, 'requests': k, 'subgraph_nodes': 20, 'hops': 1,
       'variants': len(variants), 'variants_per_request': round(len(variants) / k, 1), 'chunk': CHUNK, 'reps': reps}
stage('%d variants; warming' % len(variants))
got = P.suggest(requests, max_variants=CHUNK)
assert int(got['ptr'][-1]) == len(variants)
predict_lists(variants[:CHUNK])
stage('timing suggest')
res['suggest_border_ms'] = med(lambda: P.suggest(requests, max_variants=CHUNK))
stage('timing the list route')
res['candidate_rows_ms'] = med(lambda: suggest.candidate_rows(P, sets, 'border', 1))
res['parent_build_lists_ms'] = med(lambda: add_one(mapped, borders))
res['parent_predict_lists_ms'] = med(lambda: (P.predict(requests), predict_lists(variants)))
res['parent_map_subgraphs_host_ms'] = med(lambda: P.map_subgraphs(variants))
stage('timing the expansion')
res['insertion_sets_ms'] = med(lambda: ops.insertion_sets(sets, rows, shared))
res['predict_base_ms'] = med(lambda: P.predict(requests))
line = json.dumps(res)
print(line)
if out_file:
    with open(out_file, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')

#!/usr/bin/env python3
"""Leave-one-out attribution, timed on the model of tools/predict_probe.py (BA 1M nodes / m = 10, prepared on the benchmark's
50k training subgraphs): ``Predictor.explain(unit='node')`` on ``k`` fresh BFS subgraphs of 20 nodes (20 k variants) beside the
route there was before for the same variants -- the leave-one-out node lists written out in Python and sent through
``Predictor.predict`` -- and the device expansion alone (``ops.occlusion_sets``).  Wall clock around device synchronisations,
milliseconds; the median of ``reps`` warm calls.  No threshold: nobody had measured either number.
    python tools/explain_probe.py [reps] [out.json] [k]"""
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from subgnn_amd import hotpath, ops, synthetic
from subgnn_amd.SubGNN import SubGNN
from subgnn_amd.predict import Predictor

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = sys.argv[2] if len(sys.argv) > 2 else None
k = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
n, m, S, D = 1_000_000, 10, 50_000, 64
dev = torch.device('cuda:0')


def stage(what):
    print('[explain_probe] ' + what, file=sys.stderr, flush=True)


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


def leave_one_out(lists):
    return [s[:i] + s[i + 1:] for s in lists for i in range(len(s)) if len(s) > 1]


stage('timing')
P = Predictor(model)
P.predict(requests)                                                   # the freeze, the code objects
variants = leave_one_out([sorted(set(s)) for s in requests])
res = {'graph_nodes': n, 'graph_m': m, 'train_subgraphs': S, 'requests': k, 'subgraph_nodes': 20, 'variants': len(variants),
       'reps': reps}
P.explain(requests)
P.predict(variants)
res['explain_node_ms'] = med(lambda: P.explain(requests, unit='node'))
res['explain_node_3_draws_ms'] = med(lambda: P.explain(requests, unit='node', draws=3))
res['parent_build_lists_ms'] = med(lambda: leave_one_out([sorted(set(s)) for s in requests]))
res['parent_predict_lists_ms'] = med(lambda: (P.predict(requests), P.predict(variants)))
res['parent_map_subgraphs_host_ms'] = med(lambda: P.map_subgraphs(variants))
sets = P.request_sets(requests)
res['occlusion_sets_ms'] = med(lambda: ops.occlusion_sets(sets, 'node'))
res['predict_base_ms'] = med(lambda: P.predict(requests))
line = json.dumps(res)
print(line)
if out_file:
    with open(out_file, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')

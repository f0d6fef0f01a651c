#!/usr/bin/env python3
"""Prediction on subgraphs outside the dataset, timed on the benchmark's graph (BA 1M nodes / m = 10; a model prepared on the
benchmark's 50k training subgraphs): ``Predictor.predict`` on 1k and on 50k fresh BFS subgraphs -- the first call, which
freezes the widths, hop tables and patch degree sequences, and the calls after it -- and, in the same process, the route
there was before: the lists put in ``test_sub_G`` by hand, ``hotpath.prepare_sparse(model, 'test')`` plus the forward pass over
the split.  Wall clock around device synchronisations, milliseconds; the median of ``reps`` warm calls.  The expectation to
confirm or refute: a warm request does not pay the position search over the whole graph.
    python tools/predict_probe.py [reps] [out.json]"""
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
n, m, S, D = 1_000_000, 10, 50_000, 64
dev = torch.device('cuda:0')
edges = synthetic.barabasi_albert_edges(n, m, seed=42)
rowptr, col = synthetic.sorted_csr(edges, n)
train = synthetic.bfs_subgraphs(rowptr, col, S, 20, seed=1000)
requests = {k: synthetic.bfs_subgraphs(rowptr, col, k, 20, seed=2000 + i) for i, k in enumerate((1000, S))}
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


def as_test_split(lists):
    """The route before predict.py: the lists as the model's test split (every per-split fact kept for 'test' dropped first)."""
    model.test_sub_G = lists
    model.test_sub_G_label = torch.zeros(len(lists), dtype=torch.int64)
    hotpath.forget_split_facts(model, 'test')


def test_split_call():
    hotpath.prepare_sparse(model, 'test')
    model.eval()
    with torch.no_grad():
        model._forward_batch('test', hotpath.full_split_batch(model, 'test'))


P = Predictor(model)
res = {'graph_nodes': n, 'graph_m': m, 'train_subgraphs': S, 'subgraph_nodes': 20, 'reps': reps}
# dataset numbering: model id - 1
shifted = {k: [[v - 1 for v in s] for s in ls] for k, ls in requests.items()}
res['predict_first_call_1000_ms'] = round(wall(lambda: P.predict(shifted[1000])), 3)          # with the freeze
for k in (1000, S):
    P.predict(shifted[k])
    res['predict_warm_%d_ms' % k] = round(statistics.median(wall(lambda: P.predict(shifted[k])) for _ in range(reps)), 3)
    res['prepare_warm_%d_ms' % k] = round(statistics.median(wall(lambda: P.prepare(shifted[k])) for _ in range(reps)), 3)
res['map_subgraphs_host_%d_ms' % S] = round(statistics.median(wall(lambda: P.map_subgraphs(shifted[S])) for _ in range(reps)), 3)
for k in (1000, S):
    as_test_split(requests[k])
    res['test_split_first_call_%d_ms' % k] = round(wall(test_split_call), 3)
    res['test_split_warm_%d_ms' % k] = round(statistics.median(wall(test_split_call) for _ in range(reps)), 3)
line = json.dumps(res)
print(line)
if out_file:
    with open(out_file, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')

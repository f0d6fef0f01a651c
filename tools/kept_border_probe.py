#!/usr/bin/env python3
"""The kept one-hop borders on the benchmark's inputs (50k BFS subgraphs of 20 nodes, BA 1M / 10M): bytes kept, the one-time
build (count launch + prefix sum + size read-back + write launch, HIP events), ms per draw from the kept ids against ms per
fused border + draw call, and a check that both give the same anchors.  Prints one JSON line.
    python tools/kept_border_probe.py [reps]"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from subgnn_amd import ops, synthetic, tape

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n, m, S = 1_000_000, 10, 50_000
edges = synthetic.barabasi_albert_edges(n, m, seed=42)
rowptr, col = synthetic.sorted_csr(edges, n)
subs = synthetic.bfs_subgraphs(rowptr, col, S, 20, seed=1000)
dev = torch.device('cuda:0')
g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), dev)
sets = ops.Ragged.from_lists(subs, dev)
st = tape.stream_id(tape.STREAM_N_BOR, 'train', 0)
a, w, c = ops.khop_border_sample(g, sets, 1, 43, 0, st)
width = c.max().view(1)
ops.khop1_borders_sorted(g, sets, max_bytes=0)            # (code object loaded, allocator warm: count launch only)
torch.cuda.synchronize()
kept = ops.khop1_borders_sorted(g, sets)
torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


fused_ms, (a, w, c) = timed(lambda: ops.khop_border_sample(g, sets, 1, 43, 0, st, width=width))
draw_ms, (a2, w2, c2) = timed(lambda: ops.draw_border_anchors(kept, 43, 0, st, width=width))
print(json.dumps({'sets': sets.n, 'border_ids': int(kept.ptr[-1]), 'largest_border': int(width), 'kept_bytes': kept.nbytes,
                  'build_ms': round(kept.build_ms(), 3), 'fused_call_ms': round(fused_ms, 4), 'draw_from_kept_ms': round(draw_ms, 4),
                  'equal': bool(torch.equal(a, a2) and torch.equal(w, w2) and torch.equal(c, c2))}))

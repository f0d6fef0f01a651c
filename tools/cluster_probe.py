#!/usr/bin/env python3
"""One Lloyd iteration timed at the sizes it is for: ``ops.kmeans_step`` (assignment, per-cluster sums and the finish launch;
l2, float32 normals, the rows' squared norms formed once outside the window as ops.kmeans keeps them) at (N, D, K) =
(50k, 516, 64) and (1M, 128, 256), and beside it, in the same process and alternating with it, two other routes to the same
iteration:
  pieces   what the project already had: ``ops.topk_rows(k = 1)``, then ``index_add_``, ``bincount`` and the division;
  library  ``argmin`` of the (N, K) matrix ``xa + ca - 2 X @ C.T``, then ``index_add_``, ``bincount`` and the division.
Device events around each call, milliseconds; per shape ``rounds`` alternating rounds after two warm calls of each route,
reported as median, min and max; the bytes of the (N, K) matrix the library route needs; and whether the three routes chose the
same centres (rows that differ, and the largest difference of a next centre).
    python tools/cluster_probe.py [rounds] [out.json]"""
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from subgnn_amd import ops

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
SHAPES = [(50_000, 516, 64), (1_000_000, 128, 256)]
METRIC = 'l2'
dev = torch.device('cuda:0')
ops.warm_up(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(ts):
    return {'median_ms': round(statistics.median(ts), 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4)}


def update(X, C, assign, K):
    sums = torch.zeros_like(C).index_add_(0, assign, X)
    counts = torch.bincount(assign, minlength=K)
    return assign, torch.where(counts[:, None] > 0, sums / counts[:, None].float(), C)


res = {'metric': METRIC, 'rounds': rounds, 'shapes': []}
for N, D, K in SHAPES:
    g = torch.Generator(device=dev).manual_seed(N + D + K)
    X = torch.randn(N, D, device=dev, generator=g)
    C = X[torch.randperm(N, device=dev, generator=g)[:K]].contiguous()
    xa, ca = ops.topk_aux(X, METRIC), ops.topk_aux(C, METRIC)

    def ours():
        r = ops.kmeans_step(X, C, METRIC, x_aux=xa, c_aux=ca)
        return r['assign'].long(), r['centers']

    def pieces():
        return update(X, C, ops.topk_rows(X, C, 1, METRIC, q_aux=xa, b_aux=ca)[1][:, 0], K)

    def library():
        return update(X, C, torch.argmin(torch.addmm(xa[:, None] + ca[None, :], X, C.T, alpha=-2.0), dim=1), K)
    routes = [('kmeans_step', ours), ('pieces', pieces), ('library', library)]
    for _, fn in routes:                                               # warm-up: code objects, the library's algorithm choice
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in routes}
    last = {}
    for _ in range(rounds):
        for name, fn in routes:
            t, last[name] = timed(fn)
            times[name].append(t)
    row = {'N': N, 'D': D, 'K': K, 'score_matrix_mb_of_the_library_route': round(4 * N * K / 2 ** 20, 1),
           'workspace_mb_of_kmeans_step': round(ops._lib.load().sgnn_kmeans_workspace_bytes(N, K, D) / 2 ** 20, 1),
           'slots': int(ops._lib.load().sgnn_kmeans_slots(N, K, D))}
    for name, _ in routes:
        row[name] = spread(times[name])
    for name in ('pieces', 'library'):
        row['ratio_%s_over_kmeans_step_at_median' % name] = round(row[name]['median_ms'] / row['kmeans_step']['median_ms'], 3)
        row['rows_assigned_differently_by_%s' % name] = int((last[name][0] != last['kmeans_step'][0]).sum())
        row['largest_centre_difference_to_%s' % name] = float((last[name][1] - last['kmeans_step'][1]).abs().max())
    again = ours()
    row['kmeans_step_repeats_bit_for_bit'] = bool(torch.equal(again[1].view(torch.int32), last['kmeans_step'][1].view(torch.int32)))
    a, b = pieces(), pieces()
    row['pieces_repeat_bit_for_bit'] = bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    res['shapes'].append(row)
    del X, C, xa, ca, last, again, a, b
    torch.cuda.empty_cache()
line = json.dumps(res)
print(line)
if out_file:
    with open(out_file, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')

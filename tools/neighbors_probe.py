#!/usr/bin/env python3
"""The nearest-row search timed at the sizes it is for: ``ops.topk_rows`` (k = 10, cosine, float32 normals, the bank's inverse
norms formed once outside the window as SubgraphIndex keeps them) at (Q, N, H) = (1, 50k, 516), (50k, 50k, 516) and
(1024, 1M, 128), and beside it, in the same process and alternating with it, the route a user had before:
``torch.topk((q * qa) @ (bank * ba).T, k)`` wherever the (Q, N) float32 matrix and the normalised copy fit in ``budget_gb``.
Device events around each call, milliseconds; per shape ``rounds`` alternating rounds after a warm-up of each route, reported
as median, min and max; the score FLOP rate (2 Q N H over the median) for scale.  Where both routes run, the two results are
compared: equal index sets per query up to ties within 1e-5 of the k-th score.
    python tools/neighbors_probe.py [rounds] [out.json] [budget_gb]"""
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from subgnn_amd import ops

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
budget = float(sys.argv[3]) * 2 ** 30 if len(sys.argv) > 3 else 64 * 2 ** 30
SHAPES = [(1, 50_000, 516), (50_000, 50_000, 516), (1024, 1_000_000, 128)]
K, METRIC = 10, 'cosine'
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


res = {'k': K, 'metric': METRIC, 'rounds': rounds, 'shapes': []}
for Q, N, H in SHAPES:
    g = torch.Generator(device=dev).manual_seed(Q + N + H)
    q = torch.randn(Q, H, device=dev, generator=g)
    bank = torch.randn(N, H, device=dev, generator=g)
    ba = ops.topk_aux(bank, METRIC)
    ours = lambda: ops.topk_rows(q, bank, K, metric=METRIC, b_aux=ba)
    fits = 4 * Q * N + 4 * (Q + N) * H <= budget

    def library():
        s = (q * ops.topk_aux(q, METRIC)[:, None]) @ (bank * ba[:, None]).T
        return torch.topk(s, K, dim=1)
    routes = [('topk_rows', ours)] + ([('torch_topk_of_matmul', library)] if fits else [])
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
    row = {'Q': Q, 'N': N, 'H': H, 'score_matrix_gb': round(4 * Q * N / 2 ** 30, 3)}
    for name, _ in routes:
        row[name] = spread(times[name])
        row[name]['score_tflops_at_median'] = round(2.0 * Q * N * H / (row[name]['median_ms'] * 1e-3) / 1e12, 2)
    if fits:
        row['ratio_library_over_topk_rows_at_median'] = round(row['torch_topk_of_matmul']['median_ms'] / row['topk_rows']['median_ms'], 3)
        (s1, i1), (s2, i2) = last['topk_rows'], last['torch_topk_of_matmul']
        same = (i1.sort(dim=1).values == i2.sort(dim=1).values).all(dim=1)
        near_tie = (s1[:, -1] - s2[:, -1]).abs() <= 1e-5
        row['queries_with_equal_index_sets'] = int(same.sum())
        row['queries_differing_beyond_a_near_tie'] = int((~same & ~near_tie).sum())
    else:
        row['torch_topk_of_matmul'] = 'not run: the score matrix does not fit the budget'
    res['shapes'].append(row)
    del q, bank, ba, last
    torch.cuda.empty_cache()
line = json.dumps(res)
print(line)
if out_file:
    with open(out_file, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')

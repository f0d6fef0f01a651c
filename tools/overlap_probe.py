#!/usr/bin/env python3
"""Node-overlap self-search timed at the size it is for: ``ops.overlap_topk`` (Jaccard, k = 10, every set its own row excluded)
over the 50k subgraphs of the synthetic shard (1M-node Barabasi-Albert graph, breadth-first subgraphs of 20 nodes), the queries
being the bank's own sets.  Beside it, in the same process and alternating with it, the same search written with torch: the
sparse incidence matrix of a chunk of queries times the transposed incidence matrix of the bank, made dense chunk by chunk,
Jaccard in float32 from the counts and the sizes, the own row masked, then ``topk``.  Device events around each call (the call
of ops.overlap_topk includes its host round trip), milliseconds; ``rounds`` alternating rounds after one warm call of each,
reported as median, min and max.  Also: the distribution of P (postings walked per query), the share of queries per tier, the
one-time cost of the bank's postings, how many result rows of the torch route differ (rows: its ties go by topk's choice;
scores: none should), and the same call with 4 x the workspace budget, i.e. a quarter of the chunks.
    python tools/overlap_probe.py [rounds] [out.json]"""
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from subgnn_amd import ops, synthetic

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = sys.argv[2] if len(sys.argv) > 2 else None
n, m, S, K, CHUNK = 1_000_000, 10, 50_000, 10, 2048
dev = torch.device('cuda:0')
ops.warm_up(dev)

rowptr, col = synthetic.sorted_csr(synthetic.barabasi_albert_edges(n, m, seed=42), n)
subs = [sorted(set(s)) for s in synthetic.bfs_subgraphs(rowptr, col, S, 20, seed=1000)]
sets = ops.Ragged.from_lists(subs, dev)
torch.cuda.synchronize()
t0 = time.perf_counter()
bank = ops.SetBank(sets)
torch.cuda.synchronize()
bank_ms = (time.perf_counter() - t0) * 1e3
me = torch.arange(S, dtype=torch.int64, device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(ts):
    return {'median_ms': round(statistics.median(ts), 3), 'min_ms': round(min(ts), 3), 'max_ms': round(max(ts), 3)}


def ours():
    return ops.overlap_topk(sets, bank, K, 'jaccard', exclude=me)


def ours_wide():                                                       # what the chunks cost: the same call with 4 x the workspace
    return ops.overlap_topk(sets, bank, K, 'jaccard', exclude=me, ws_budget=4 * ops.OVERLAP_WS_BUDGET)


# the torch route's operands, built once outside the window as the bank's postings are
total = sets.total
row = torch.repeat_interleave(torch.arange(S, device=dev), sets.lengths, output_size=total)
ids = sets.nodes[:total].long()
ones = torch.ones(total, dtype=torch.float32, device=dev)
bank_t = torch.sparse_coo_tensor(torch.stack([ids, row]), ones, (bank.max_id + 1, S)).coalesce()
sizes = sets.lengths.float()


def library():
    rows_out = torch.empty((S, K), dtype=torch.int64, device=dev)
    vals_out = torch.empty((S, K), dtype=torch.float32, device=dev)
    for lo in range(0, S, CHUNK):
        hi = min(lo + CHUNK, S)
        sel = (row >= lo) & (row < hi)
        a = torch.sparse_coo_tensor(torch.stack([row[sel] - lo, ids[sel]]), ones[sel], (hi - lo, bank.max_id + 1))
        inter = torch.sparse.mm(a, bank_t).to_dense()
        jac = inter / (sizes[lo:hi, None] + sizes[None, :] - inter)
        jac[torch.arange(hi - lo, device=dev), torch.arange(lo, hi, device=dev)] = 0.0
        v, i = torch.topk(jac, K, dim=1)
        rows_out[lo:hi] = torch.where(v > 0, i, torch.full_like(i, -1))
        vals_out[lo:hi] = v
    return rows_out, vals_out


routes = [('overlap_topk', ours), ('overlap_topk_4x_workspace', ours_wide), ('torch_sparse_product_topk', library)]
for _, fn in routes:
    fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in routes}
last = {}
for _ in range(rounds):
    for name, fn in routes:
        t, last[name] = timed(fn)
        times[name].append(t)

P = ops.set_postings(sets, bank).cpu().numpy()
lds_max = ops.overlap_lds_max()
rows, inter, touched, scores = last['overlap_topk']
res = {'subgraphs': S, 'graph_nodes': n, 'k': K, 'measure': 'jaccard', 'rounds': rounds, 'torch_chunk_rows': CHUNK,
       'bank_postings_build_ms_once': round(bank_ms, 3),
       'postings_walked_per_query': {'min': int(P.min()), 'median': float(np.median(P)), 'mean': round(float(P.mean()), 1),
                                     'p99': float(np.percentile(P, 99)), 'max': int(P.max())},
       'share_of_queries_per_tier': {'lds': round(float((P <= lds_max).mean()), 6), 'workspace': round(float((P > lds_max).mean()), 6)},
       'workspace_mb': round(48 * int(P[P > lds_max].sum()) / 2 ** 20, 2),
       'rows_met_per_query': {'median': float(np.median(touched.cpu().numpy())), 'max': int(touched.max())},
       'queries_with_k_results': int((rows[:, K - 1] >= 0).sum())}
for name, _ in routes:
    res[name] = spread(times[name])
res['ratio_torch_over_overlap_topk_at_median'] = round(res['torch_sparse_product_topk']['median_ms'] / res['overlap_topk']['median_ms'], 3)
# equal scores go to the smaller row here and to whichever row topk meets in the torch route: the rows differ wherever the k-th
# score is tied (most sets share one hub node with thousands of sets of the same size); the scores must not
res['result_rows_that_differ_from_torch'] = int((last['torch_sparse_product_topk'][0] != rows).any(dim=1).sum())
res['result_rows_whose_scores_differ_from_torch_by_more_than_1e-6'] = int(((last['torch_sparse_product_topk'][1] - scores).abs() > 1e-6).any(dim=1).sum())
res['overlap_topk_4x_workspace_equals_overlap_topk'] = bool(all(torch.equal(a, b) for a, b in zip(last['overlap_topk_4x_workspace'], last['overlap_topk'])))
res['workspace_budget_mb'] = ops.OVERLAP_WS_BUDGET >> 20
print(json.dumps(res))
if out_file:
    with open(out_file, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')

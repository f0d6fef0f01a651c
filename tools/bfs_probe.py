#!/usr/bin/env python3
"""The position channel's multi-source BFS alone on the benchmark graph (BA n=1M m=10, 183 sources, 50k component sets):
ms per search by HIP events for the forms the pass runs (levels and push levels capped from the first search's status) and the
uncapped one -- the full search (until the frontier dies) and the closing one (until every set has its hops) -- with the
closing level, the sets still open after every level (and the nodes they hold) and the launches per search.  The levels the
closing form is given are the pass's: closing level + hotpath.BFS_LEVEL_MARGIN + 1, push levels from the status as
hotpath._bfs_push_levels derives them.

    python tools/bfs_probe.py [--reps 10] [--sets 50000]

Per-level kernel times: run it with --trace under ``rocprofv3 --kernel-trace --output-format csv -d DIR --`` (one search of
each form is then the last thing it does) and hand the trace to

    python tools/bfs_probe.py --levels DIR/.../*_kernel_trace.csv
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = ('full', 'closing')


def levels_from_trace(path):
    """The last len(FORMS) searches of a kernel trace -> {form: [[kernel, us], ...]} in launch order."""
    rows = [r for r in csv.DictReader(open(path)) if 'msbfs_' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    starts = [i for i, r in enumerate(rows) if 'msbfs_init_kernel' in r['Kernel_Name']] + [len(rows)]
    out = {}
    for form, a, b in zip(FORMS, starts[-len(FORMS) - 1:-1], starts[-len(FORMS):]):
        ks = [[r['Kernel_Name'].split('(')[0].replace('msbfs_', '').replace('_kernel', ''),
               round((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3, 1)] for r in rows[a:b]]
        out[form] = {'launches': len(ks), 'kernel_us': round(sum(k[1] for k in ks), 1), 'kernels': ks}
    return out


def launches(form, levels, push_levels):
    """Launches per search as msbfs_run enqueues them."""
    push = levels if push_levels < 0 else max(1, min(push_levels, levels))
    if form == 'full':
        return 2 + 2 * push + (levels - push) + 1                       # init, seed; level + commit | pull; finalize
    return 2 + 1 + 3 * push + 2 * (levels - push) + 1                   # init, seed; reduction of the seeds; level + commit + reduction | pull + reduction; status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sets', type=int, default=50000)
    ap.add_argument('--sources', type=int, default=183)
    ap.add_argument('--trace', action='store_true', help='end with one search of each form (for a kernel trace)')
    ap.add_argument('--levels', help='a rocprofv3 kernel-trace CSV of a --trace run: print the per-level kernel times')
    args = ap.parse_args()
    if args.levels:
        print(json.dumps(levels_from_trace(args.levels)))
        return
    import numpy as np
    import torch
    from subgnn_amd import ops, synthetic, hotpath
    dev = torch.device('cuda:0')
    n = 1_000_000
    edges = synthetic.barabasi_albert_edges(n, 10, seed=42)
    rowptr, col = synthetic.sorted_csr(edges, n)
    g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), dev)
    subs = synthetic.bfs_subgraphs(rowptr, col, args.sets, 20, seed=1000)
    sets = ops.Ragged.from_lists(subs, dev)
    src = torch.from_numpy(np.random.default_rng(2).integers(1, n + 1, args.sources).astype(np.int32)).to(dev)
    ref, st = ops.bfs_min_hops_to_sets(g, src, sets, max_hops=32, want_status=True)
    last, more, first_pull, _ = st.tolist()
    g.component_labels()
    got, cst = ops.bfs_min_hops_to_sets(g, src, sets, max_hops=32, want_status=True, until='sets')
    assert torch.equal(got, ref)
    closing, cmore, cfirst_pull, _ = cst.tolist()
    assert cmore == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(**kw):
        out = ops.bfs_min_hops_to_sets(g, src, sets, **kw)
        assert torch.equal(out, ref), kw
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            ops.bfs_min_hops_to_sets(g, src, sets, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps
    # a set is open after level L while some source's hops to it exceed L
    close_at = ref.max(1).values                                          # per set
    owner = torch.repeat_interleave(torch.arange(sets.n, device=dev), sets.ptr[1:] - sets.ptr[:-1])
    open_nodes = {}
    for L in range(1, closing):
        open_nodes[L] = int(torch.unique(sets.nodes[:owner.numel()][close_at[owner] > L]).numel())
    margin = hotpath.BFS_LEVEL_MARGIN + 1

    def push(first):                                                      # hotpath._bfs_push_levels: never pulled -> all levels
        return -1 if not first else first - 1 + hotpath.BFS_PUSH_MARGIN
    full_kw = dict(max_hops=last + margin, push_levels=push(first_pull))
    close_kw = dict(max_hops=closing + margin, push_levels=push(cfirst_pull), until='sets')
    res = {'levels': last, 'first_pull_level': first_pull, 'closing_level': closing,
           'sets_open_after_level': {L: int((close_at > L).sum()) for L in range(closing)},
           'nodes_of_the_sets_open_after_level': open_nodes,
           'levels_enqueued': {'full': full_kw['max_hops'], 'closing': close_kw['max_hops']},
           'launches_per_search': {'full': launches('full', full_kw['max_hops'], full_kw['push_levels']),
                                   'closing': launches('closing', close_kw['max_hops'], close_kw['push_levels'])},
           'ms_uncapped(32 levels, all may push)': timed(max_hops=32),
           'ms_levels_capped': timed(max_hops=last + 3),
           'ms_levels_and_push_capped(the pass)': timed(**full_kw),
           'ms_push_levels_1': timed(max_hops=last + 3, push_levels=1),
           'ms_always_push': timed(max_hops=last + 3, pull_alpha=0),
           'ms_closing_uncapped(32 levels, all may push)': timed(max_hops=32, until='sets'),
           'ms_closing(the pass)': timed(**close_kw),
           'ms_closing_push_levels_1': timed(max_hops=closing + 3, push_levels=1, until='sets')}
    print(json.dumps(res))
    if args.trace:
        torch.cuda.synchronize()
        for kw in (full_kw, close_kw):
            ops.bfs_min_hops_to_sets(g, src, sets, **kw)
        torch.cuda.synchronize()


if __name__ == '__main__':
    main()

"""fastdtw against exact DTW on the benchmark's own structure-channel inputs (the graph, the 50k BFS components and the 210
patches tools/dtw_probe.py builds; internal and external side), measured in ONE process:

    python tools/dtw_exact_probe.py [--rounds 40] [--out profiles/dtw_exact_probe.json]

Every round runs each function once, in turn ('dtw' = the fastdtw launch with the default predecessor rule, 'dtw_exact' = the
exact one), between device events, after warmed calls; the call is the one hotpath.finish_pass makes (kept x_prep; repeated component rows
grouped on the internal side, not on the external one).  Median, minimum and the 10 % / 90 % quantiles per function and the
ratios to 'dtw' go into the JSON, with how far the values of the two functions are apart (sampled pairs of both are
checked against the CPU oracle first).  A third set of inputs is the external side with strictly increasing patch series:
no column repeats its predecessor, the case the kept cost column of the exact kernel does not help.

Vector instructions per 64 pairs come from a counter run of its own (counters never together with tracing):

    rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU \\
        --output-format csv -d /tmp/dtw_exact_pmc -- python3 tools/dtw_exact_probe.py --counters /tmp/dtw_exact_pmc
    python tools/dtw_exact_probe.py --fold-counters /tmp/dtw_exact_pmc [--out profiles/dtw_exact_probe.json]

(--counters DIR launches both functions on the benchmark's two sides and writes the number of 64-pair tasks per launch into
DIR, the directory the counters go to; --fold-counters needs no GPU: it adds the per-kernel averages to the JSON.)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (('dtw', dict(fn='dtw')), ('dtw_exact', dict(fn='dtw_exact')))
KERNELS = {'dtw': 'dtw_similarity_reg_kernel', 'dtw_exact': 'dtw_exact_reg_kernel'}
TASKS_FILE = 'dtw_exact_tasks.json'


def inputs():
    import numpy as np
    import torch
    from subgnn_amd import ops, synthetic, tape
    n, m, S, NX = 1_000_000, 10, 50_000, 20
    edges = synthetic.barabasi_albert_edges(n, m, seed=42)
    rowptr, col = synthetic.sorted_csr(edges, n)
    subs = synthetic.bfs_subgraphs(rowptr, col, S, NX, seed=1000)
    dev = torch.device('cuda:0')
    g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), dev)
    sets = ops.Ragged.from_lists(subs, dev)
    patches = ops.triangular_walks(g, 0, 210, 50, 0.65, 0, tape.stream_id(tape.STREAM_STRUCT_PATCH))
    a_sets = ops.Ragged.from_padded(patches)
    ai, ae = ops.degree_sequence(g, a_sets)
    ci, ce = ops.degree_sequence(g, sets)
    # the external side with every patch series made strictly increasing (entry + its position in the row): no column repeats
    # its predecessor's value, the case where keeping the cost column buys nothing
    lens = a_sets.ptr[1:] - a_sets.ptr[:-1]
    total = int(a_sets.ptr[-1])
    pos = torch.arange(total, device=dev) - torch.repeat_interleave(a_sets.ptr[:-1], lens)
    ad = ae.clone()
    ad[:total] += pos.to(ad.dtype)
    return NX, sets, a_sets, {'internal': (ci, ai, True), 'external': (ce, ae, False), 'external_distinct_columns': (ce, ad, False)}


def calls(only=None):
    """{side: {function: call}}, {side: 64-pair tasks per launch}; every call warmed twice (grouping and order kept)."""
    import torch
    from subgnn_amd import ops
    NX, sets, a_sets, sides = inputs()
    if only:
        sides = {k: v for k, v in sides.items() if k in only}
    fns, tasks, outs = {}, {}, {}
    for side, (x, y, dedupe) in sides.items():
        fns[side] = {}
        for name, kw in VARIANTS:
            prep = ops.DtwRowPrep()
            f = (lambda x=x, y=y, dedupe=dedupe, prep=prep, kw=kw:
                 ops.dtw_similarity(sets.ptr, x, NX, a_sets.ptr, y, 50, dedupe=dedupe, x_prep=prep, **kw))
            f()
            outs[side, name] = f()
            fns[side][name] = f
            live = prep.grouping.live if dedupe else None
            rows = int(live[1]) if live is not None else sets.n
            tasks[side] = a_sets.n * ((rows + 63) // 64)
    torch.cuda.synchronize()
    import numpy as np
    from oracle import fastdtw_restate as FD
    same = {}
    for side, (x, y, _) in sides.items():
        a, b = outs[side, 'dtw'], outs[side, 'dtw_exact']
        assert bool((a <= b).all()), side                     # fastdtw's warp path is one of the paths
        # the values at the size that is timed: 300 seeded pairs and the pair of the largest gap against the CPU oracle
        xs, ys = ops.Ragged(sets.ptr, x).to_lists(), ops.Ragged(a_sets.ptr, y).to_lists()
        worst = int((b - a).argmax())
        rng = np.random.default_rng(5)
        picks = [(worst // a_sets.n, worst % a_sets.n)] + [(int(rng.integers(sets.n)), int(rng.integers(a_sets.n))) for _ in range(300)]
        ah, bh = a.cpu().numpy(), b.cpu().numpy()
        for r, c in picks:
            if xs[r]:
                assert bh[r, c] == np.float32(1.0 / (1.0 + FD.exact_dtw(xs[r], ys[c], FD.calc_dist))), (side, r, c)
                assert ah[r, c] == np.float32(FD.calc_dtw(xs[r], ys[c], 2)), (side, r, c)
        r, c = picks[0]
        same[side] = {'pairs': a.numel(), 'pairs_where_fastdtw_differs': int((a != b).sum()),
                      'mean_similarity_gap': float((b - a).double().mean()), 'largest_similarity_gap': float((b - a).max()),
                      'largest_gap_pair': {'x': xs[r], 'y': ys[c], 'fastdtw': float(ah[r, c]), 'exact': float(bh[r, c])},
                      'sampled_pairs_equal_to_the_cpu_oracle': len(picks)}
    return fns, tasks, same


def measure(rounds):
    import numpy as np
    import torch
    fns, tasks, same = calls()
    res = {'what': "tools/dtw_exact_probe.py: ops.dtw_similarity as hotpath.finish_pass calls it (kept x_prep) on the benchmark's "
                   "50k components x 210 patches; %d rounds, each function once per round in turn, device events, ms" % rounds,
           'device': torch.cuda.get_device_name(0), 'tasks_of_64_pairs_per_launch': tasks, 'values': same, 'sides': {}}
    for side, fs in fns.items():
        ev = {name: [] for name in fs}
        for _ in range(rounds):
            for name, f in fs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        out = {}
        for name, pairs in ev.items():
            t = np.array([a.elapsed_time(b) for a, b in pairs])
            out[name] = {'median_ms': float(np.median(t)), 'min_ms': float(t.min()), 'p10_ms': float(np.quantile(t, 0.1)),
                         'p90_ms': float(np.quantile(t, 0.9)), 'rounds': int(t.size)}
        for name in out:
            out[name]['median_over_dtw'] = out[name]['median_ms'] / out['dtw']['median_ms']
        res['sides'][side] = out
    tot = {name: sum(res['sides'][s][name]['median_ms'] for s in ('internal', 'external')) for name, _ in VARIANTS}
    res['both_sides_median_ms'] = tot
    res['both_sides_over_dtw'] = {k: v / tot['dtw'] for k, v in tot.items()}
    res['faster'] = min(tot, key=tot.get)
    return res


def run_for_counters(out_dir):
    import torch
    fns, tasks, _ = calls(only=('internal', 'external'))           # the benchmark's own two launches
    for fs in fns.values():
        for f in fs.values():
            f(); f()
    torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, TASKS_FILE), 'w') as fh:
        json.dump(tasks, fh)


def fold_counters(pmc_dir, out):
    """Per kernel of the two functions: counter means per dispatch and vector instructions per 64 pairs.  Every dispatch of
    the counted process (warmed calls included) is one of the two sides' launches, as many of one side as of the other; the
    sides differ in their number of tasks, so the instructions are summed over all dispatches and divided by their tasks."""
    import csv
    tasks = json.load(open(os.path.join(pmc_dir, TASKS_FILE)))
    acc = {}
    for root, _, files in os.walk(pmc_dir):
        for f in files:
            if f.endswith('counter_collection.csv'):
                for row in csv.DictReader(open(os.path.join(root, f), newline='')):
                    for name, pat in KERNELS.items():
                        if pat in row['Kernel_Name']:
                            a = acc.setdefault(name, {}).setdefault(row['Counter_Name'], [0.0, 0])
                            a[0] += float(row['Counter_Value'])
                            a[1] += 1
    res = json.load(open(out)) if os.path.exists(out) else {}
    per_launch_pair = sum(tasks.values())                       # one launch per side: tasks of an (internal, external) pair
    c = {}
    for name, cs in acc.items():
        n = max(v[1] for v in cs.values())
        r = {k: v[0] / v[1] for k, v in cs.items()}
        r['dispatches'] = n
        if 'SQ_INSTS_VALU' in cs:
            # total over all dispatches / total tasks of those dispatches (as many internal as external launches)
            r['valu_instructions_per_64_pairs'] = cs['SQ_INSTS_VALU'][0] / (n / 2 * per_launch_pair)
        if 'SQ_INSTS_SALU' in cs:
            r['salu_instructions_per_64_pairs'] = cs['SQ_INSTS_SALU'][0] / (n / 2 * per_launch_pair)
        c[name] = r
    res['counters'] = {'what': 'rocprofv3 --pmc, a run of its own (tools/dtw_exact_probe.py --counters); means per dispatch over '
                               'the launches of both sides', 'kernels': c}
    json.dump(res, open(out, 'w'), indent=1)
    print(json.dumps(res['counters'], indent=1))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--out', default='profiles/dtw_exact_probe.json')
    ap.add_argument('--counters', metavar='DIR')
    ap.add_argument('--fold-counters', metavar='DIR')
    a = ap.parse_args()
    if a.fold_counters:
        fold_counters(a.fold_counters, a.out)
    elif a.counters:
        run_for_counters(a.counters)
    else:
        r = measure(a.rounds)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(r, open(a.out, 'w'), indent=1)
        print(json.dumps(r, indent=1))

"""The benchmark's two triangular-walk launches between device events, on the benchmark graph: the 125 KB-bitmap kernel
(``kernel=2``), the list kernel at every launch variant, with and without the hub tables, and the wavefront kernel (``kernel=1``)
-- alternating in one process, ``rounds`` times, median in microseconds; every form's walks are compared with the first's.
The walks of a pass do not depend on the number of subgraphs (n_anchor_patches_structure x n_layers x max_sim_epochs patches):
a 6 250-subgraph shard makes the same two launches.
usage: python tools/walks_probe.py [rounds] [OUT.json] [bench.py options] -> one JSON object."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import bench                                                             # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    sys.argv = sys.argv[:1] + ['--subgraphs', '64'] + sys.argv[3:]
    args = bench.parse()
    from subgnn_amd import _lib, anchor_patch_samplers as aps, ops
    from oracle import tape
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    rowptr, col, _, _, _ = bench.build_inputs(args, 0, 1)
    g = ops.DeviceGraph(rowptr, col, np.arange(1, args.nodes + 1, dtype=np.int32), dev)
    hp = bench.ALL_DENSITY_HP
    P = hp['max_sim_epochs'] * hp['n_anchor_patches_structure'] * hp['n_layers']
    L, W, T, beta = hp['sample_walk_len'], hp['n_triangular_walks'], hp['random_walk_len'], hp['rw_beta']
    sid_p, sid_i, sid_b = (tape.stream_id(s) for s in (tape.STREAM_STRUCT_PATCH, tape.STREAM_WALK_INT, tape.STREAM_WALK_BOR))
    hub = g.hub_tables()
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    patches = ops.triangular_walks(g, 0, P, L, beta, 0, sid_p)
    views = aps.patch_node_views(patches)
    inb = aps.in_border_sets(g, views)
    torch.cuda.synchronize()

    forms = {'bitmap_1024_threads': (lambda: ops.triangular_walks(g, 0, P, L, beta, 0, sid_p, kernel=2),
                                     lambda: ops.triangular_walks_both(g, P * W, T, beta, 0, sid_i, sid_b, views, inb, W, kernel=2))}
    n_var = int(lib.sgnn_triangular_walks_variants())
    for v in range(n_var):
        for tables in (True, False):
            forms['lists_variant%d%s' % (v, '' if tables else '_no_hub_tables')] = (
                lambda v=v, t=tables: ops.triangular_walks(g, 0, P, L, beta, 0, sid_p, variant=v, hub_tables=t),
                lambda v=v, t=tables: ops.triangular_walks_both(g, P * W, T, beta, 0, sid_i, sid_b, views, inb, W, variant=v, hub_tables=t))
    forms['wavefront'] = (lambda: ops.triangular_walks(g, 0, P, L, beta, 0, sid_p, kernel=1),
                          lambda: torch.stack([ops.triangular_walks(g, 1, P * W, T, beta, 0, sid_i, patches=views, walks_per_patch=W, kernel=1),
                                               ops.triangular_walks(g, 2, P * W, T, beta, 0, sid_b, patches=views, in_border=inb,
                                                                    walks_per_patch=W, kernel=1)]))
    times = {k: ([], []) for k in forms}
    first, equal = None, True
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds + 2):                                          # two warm rounds
        for k, fns in forms.items():
            outs = []
            for i, fn in enumerate(fns):
                torch.cuda.synchronize()
                e0.record()
                outs.append(fn())
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    times[k][i].append(e0.elapsed_time(e1) * 1000.0)
            if first is None:
                first = outs
            equal = equal and torch.equal(outs[0], first[0]) and torch.equal(outs[1], first[1])
    res = {
        'what': 'tools/walks_probe.py: device-event time in microseconds, median of %d alternating rounds after 2 warm ones (a '
                'wavefront entry of the patch walks is TWO launches and a stack)' % rounds,
        'graph': {'nodes': int(args.nodes), 'nnz': int(g.nnz), 'max_degree': int(deg.max()), 'lists_of_512_or_more': int((deg >= 512).sum()),
                  'hub_tables_words_per_node': int(hub[2]) if hub is not None else None},
        'launches': {'patches': '%d graph walks of %d' % (P, L), 'walks': '%d + %d patch walks of %d in one launch' % (P * W, P * W, T)},
        'patch_steps_taken': int((patches != 0).sum()), 'walk_steps_taken': int((first[1] != 0).sum()),
        'shard_of_6250_subgraphs': 'the same two launches: the number of patches and walks does not depend on the number of subgraphs',
        'variants': {'0': 'the launch rule: patches -> %s, walks -> %s' % tuple(
                         'the bitmap kernel' if lib.sgnn_triangular_walks_rule(n, g.max_id) else 'the list kernel at 512 threads'
                         for n in (P, 2 * P * W)),
                     '1': 'list kernel, 256 threads, 256-chunk ballot cache', '2': '512 threads, 256 chunks', '3': '1024 threads, 256 chunks',
                     '4': '512 threads, 1024 chunks'},
        'median_us': {k: {'patches': round(statistics.median(t[0]), 1), 'walks': round(statistics.median(t[1]), 1)} for k, t in times.items()},
        'min_us': {k: {'patches': round(min(t[0]), 1), 'walks': round(min(t[1]), 1)} for k, t in times.items()},
        'all_forms_equal': bool(equal),
    }
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()

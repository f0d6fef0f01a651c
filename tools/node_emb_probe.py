#!/usr/bin/env python3
"""Node-embedding pre-training on the benchmark graph (BA n = 1M, m = 10: 10M edges): ms per launch by HIP events for the
aggregation forward (layer 1 at the hidden width, layer 2 at 64), its transposed (skewed: hub rows split into chunks)
backward, the negatives, the link loss, Adam over the table, and one whole training epoch (forward, loss, backward, Adam;
no host metrics), at hidden 128 and 256.  Prints algorithmic bytes per second of the aggregation (rows gathered + self rows
+ output rows + indices and weights, each once) and writes the JSON to --out.

    python tools/node_emb_probe.py [--reps 10] [--conv gcn] [--out profiles/node_emb_probe.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def agg_bytes(csr, F):
    n, nnz = csr.n_rows, csr.nnz
    return 4 * F * (nnz + 2 * n) + nnz * (4 + (4 if csr.w is not None else 0)) + 8 * (n + 1) + 4 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--conv', default='gcn')
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--out', default='profiles/node_emb_probe.json')
    args = ap.parse_args()
    from subgnn_amd import ops, synthetic, tape
    from subgnn_amd.train_node_emb import Messages, Trainer, edge_split
    dev = torch.device('cuda:0')
    g = ops.DeviceGraph.from_device_csr(*synthetic.barabasi_albert_csr_device(args.nodes, 10, 42, dev))
    m = Messages(g, args.conv)
    split = edge_split(m.pos_u.numel(), 1)
    res = dict(graph=dict(nodes=g.max_id, edges=int(m.pos_u.numel()), fwd_max_row=m.fwd.max_row, bwd_max_row=m.bwd.max_row,
                          bwd_chunks=m.bwd.n_chunks, chunk=ops.NE_CHUNK()), conv=args.conv, runs={})
    for hidden in (128, 256):
        r = {}
        X = torch.randn(m.fwd.n_rows, hidden, device=dev)
        X2 = torch.randn(m.fwd.n_rows, 64, device=dev)
        b = torch.zeros(hidden, device=dev)
        for name, csr, x, kw in (('agg_fwd_l1', m.fwd, X, dict(bias=b, relu=True, dropout=0.4, seed=1, stream_id=5)),
                                 ('agg_bwd_l1', m.bwd, X, {}), ('agg_fwd_l2', m.fwd, X2, {}), ('agg_bwd_l2', m.bwd, X2, {})):
            ms = timed(lambda: ops.ne_aggregate(csr, x, **kw), args.reps)
            by = agg_bytes(csr, x.shape[1])
            r[name] = dict(ms=ms, gbytes=by / 1e9, tb_per_s=by / ms / 1e9)
        del X2
        tr = Trainer(g, m, split, args.conv, hidden, 64, 1e-3, 5e-4, 0.4, 1)
        n_neg = tr.train_u.numel() // 4
        r['negatives'] = dict(ms=timed(lambda: tr.negatives(n_neg, 'train', 0), args.reps), pairs=n_neg)
        Z = torch.randn(m.fwd.n_rows, 64, device=dev)
        nu, nv = tr.negatives(n_neg, 'train', 0)
        pu, pv = torch.cat([tr.train_u, nu]), torch.cat([tr.train_v, nv])
        r['link_loss'] = dict(ms=timed(lambda: ops.ne_link_loss(Z, pu, pv, tr.train_u.numel()), args.reps), pairs=int(pu.numel()))
        T = tr.params[0]
        gT, mT, vT = torch.zeros_like(T), torch.zeros_like(T), torch.zeros_like(T)
        Tc = T.detach().clone()
        r['adam_table'] = dict(ms=timed(lambda: ops.adam_step(Tc, gT, mT, vT, 1e-3, (0.9, 0.999), 1e-8, 1, weight_decay=5e-4), args.reps),
                               gbytes=T.numel() * 4 * 7 / 1e9)
        del Tc, gT, mT, vT, X
        ep = [0]

        def epoch():
            tr.step(ep[0])
            ep[0] += 1
        r['epoch'] = dict(ms=timed(epoch, args.reps))
        res['runs'][str(hidden)] = r
        del tr
        torch.cuda.empty_cache()
        print(hidden, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res['graph']))


if __name__ == '__main__':
    main()

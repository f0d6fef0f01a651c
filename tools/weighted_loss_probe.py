#!/usr/bin/env python3
"""What a class weight costs in the fused head: ``ops.fused_head`` forward + backward (first-layer GEMMs, the head's two launches,
the weight-gradient contraction and the reduction: everything a training step runs for the head) with ``class_weight=None`` (the
bare launches head_fwd_kernel / head_bwd_kernel) and with a weight row (headw_fwd_kernel / headw_bwd_kernel), single- and
multi-label, at the benchmark's 50k rows and at a batch-sized step.  The two sides alternate inside ONE process; times are device
events around ``--iters`` calls, each round listed and the median of each side reported.

    python tools/weighted_loss_probe.py [--rounds 5] [--iters 200] [--out profiles/weighted_loss_probe.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402

from subgnn_amd import ops                                     # noqa: E402

DEV = 'cuda:0'
# (rows, input width, hidden 1, hidden 2, classes): the benchmark's head over a 50k-subgraph shard, and one batch of 128
SHAPES = {'rows_50k': (50000, 566, 64, 64, 6), 'batch_128': (128, 566, 64, 64, 6)}


def median(v):
    v = sorted(v)
    return v[(len(v) - 1) // 2]


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def sides(shape, multilabel):
    B, H0, H1, H2, K = shape
    g = torch.Generator().manual_seed(B + K)
    mods = [torch.nn.Linear(H0, H1).to(DEV), torch.nn.Linear(H1, H2).to(DEV), torch.nn.Linear(H2, K).to(DEV)]
    x = torch.randn(B, H0, generator=g).to(DEV).requires_grad_(True)
    w = (torch.rand(K, generator=g) * 9.9 + 0.1).to(DEV)
    if multilabel:
        y = (torch.rand(B, K, generator=g) < 0.35).long().to(DEV)
        kw = [dict(targets=y), dict(targets=y, class_weight=w, pos_weight=w)]
    else:
        y = torch.randint(0, K, (B,), generator=g).to(DEV)
        kw = [dict(labels=y), dict(labels=y, class_weight=w)]

    def make(k):
        def step():
            x.grad = None
            for m in mods:
                m.zero_grad(set_to_none=True)
            _, loss, _ = ops.fused_head(x, mods[0], mods[1], mods[2], p=0.0, rng=None, **k)
            loss.backward()
        return step
    return make(kw[0]), make(kw[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('weighted_loss_probe: no GPU (a time is measured on the device or not at all)')
    out = {'what': 'ops.fused_head forward + backward, ms per call by device events over --iters calls; bare = class_weight None '
                   '(head_fwd_kernel / head_bwd_kernel), weighted = a weight row (headw_*; multi-label: weight and pos_weight); '
                   'the sides alternate in one process, medians over the rounds',
           'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'iters': args.iters, 'warmup': args.warmup, 'cases': {}}
    for name, shape in SHAPES.items():
        for ml in (False, True):
            bare, weighted = sides(shape, ml)
            for _ in range(args.warmup):
                bare(), weighted()
            runs = []
            for _ in range(args.rounds):
                runs.append({'bare_ms': round(time_ms(bare, args.iters), 5), 'weighted_ms': round(time_ms(weighted, args.iters), 5)})
            mb, mw = median([r['bare_ms'] for r in runs]), median([r['weighted_ms'] for r in runs])
            key = '%s_%s' % (name, 'multi_label' if ml else 'single_label')
            out['cases'][key] = {'shape_B_H0_H1_H2_K': list(shape), 'bare_ms': mb, 'weighted_ms': mw,
                                 'weighted_over_bare': round(mw / mb, 4), 'runs': runs}
            print(key, json.dumps(out['cases'][key]), flush=True)
    txt = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()

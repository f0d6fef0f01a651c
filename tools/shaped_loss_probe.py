#!/usr/bin/env python3
"""What label smoothing and focal loss cost in the fused head: ``ops.fused_head`` forward + backward (first-layer GEMMs, the head's
two launches, the weight-gradient contraction and the reduction: everything a training step runs for the head) bare, with a weight
row, with label smoothing 0.1 and with focal gamma 2 (single- and multi-label), and the same ShapedLoss on the library route (what
``fused_forward: false`` runs for the head: three library Linear layers with relu between them + loss_weights.ShapedLoss through
autograd), at the benchmark's 50k rows and at a batch-sized step.  The configurations alternate inside ONE process; times are device
events around ``--iters`` calls, each round listed, the median and the min-max spread of each configuration reported.  No ratio is
expected in advance.

    python tools/shaped_loss_probe.py [--rounds 5] [--iters 200] [--out profiles/shaped_loss_probe.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
import torch.nn.functional as F                                # noqa: E402

from subgnn_amd import ops                                     # noqa: E402
from subgnn_amd.loss_weights import ShapedLoss                 # noqa: E402

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


def configurations(shape, multilabel):
    """{name: step} -- every step clears the gradients, runs the head + loss forward and the backward."""
    B, H0, H1, H2, K = shape
    g = torch.Generator().manual_seed(B + K)
    mods = [torch.nn.Linear(H0, H1).to(DEV), torch.nn.Linear(H1, H2).to(DEV), torch.nn.Linear(H2, K).to(DEV)]
    x = torch.randn(B, H0, generator=g).to(DEV).requires_grad_(True)
    w = (torch.rand(K, generator=g) * 9.9 + 0.1).to(DEV)
    if multilabel:
        y = (torch.rand(B, K, generator=g) < 0.35).long().to(DEV)
        rows = dict(class_weight=w, pos_weight=w)
        kernel = {'bare': dict(targets=y), 'weighted': dict(targets=y, **rows), 'focal': dict(targets=y, focal_gamma=2.0, **rows)}
        library = {'focal_library': ShapedLoss(True, focal_gamma=2.0, weight=w, pos_weight=w).to(DEV)}
    else:
        y = torch.randint(0, K, (B,), generator=g).to(DEV)
        kernel = {'bare': dict(labels=y), 'weighted': dict(labels=y, class_weight=w),
                  'smoothing': dict(labels=y, class_weight=w, label_smoothing=0.1), 'focal': dict(labels=y, class_weight=w, focal_gamma=2.0)}
        library = {'smoothing_library': ShapedLoss(False, label_smoothing=0.1, weight=w).to(DEV),
                   'focal_library': ShapedLoss(False, focal_gamma=2.0, weight=w).to(DEV)}

    def clear():
        x.grad = None
        for m in mods:
            m.zero_grad(set_to_none=True)

    def fused(k):
        def step():
            clear()
            _, loss, _ = ops.fused_head(x, mods[0], mods[1], mods[2], p=0.0, rng=None, **k)
            loss.backward()
        return step

    def lib(module):
        def step():
            clear()
            module(mods[2](F.relu(mods[1](F.relu(mods[0](x))))), y).backward()
        return step
    out = {name: fused(k) for name, k in kernel.items()}
    out.update({name: lib(m) for name, m in library.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('shaped_loss_probe: no GPU (a time is measured on the device or not at all)')
    out = {'what': 'head + loss forward + backward, ms per call by device events over --iters calls.  bare / weighted / smoothing '
                   '(eps 0.1) / focal (gamma 2): ops.fused_head (shaped: heads_fwd_kernel / heads_bwd_kernel, with the weight rows); '
                   '*_library: three library Linear layers + loss_weights.ShapedLoss through autograd (the fused_forward: false '
                   'route).  The configurations alternate in one process; median and min-max over the rounds',
           'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'iters': args.iters, 'warmup': args.warmup, 'cases': {}}
    for name, shape in SHAPES.items():
        for ml in (False, True):
            steps = configurations(shape, ml)
            for _ in range(args.warmup):
                for fn in steps.values():
                    fn()
            runs = []
            for _ in range(args.rounds):
                runs.append({k + '_ms': round(time_ms(fn, args.iters), 5) for k, fn in steps.items()})
            case = {'shape_B_H0_H1_H2_K': list(shape)}
            for k in steps:
                v = [r[k + '_ms'] for r in runs]
                case[k + '_ms'] = {'median': median(v), 'min': min(v), 'max': max(v)}
            case['runs'] = runs
            key = '%s_%s' % (name, 'multi_label' if ml else 'single_label')
            out['cases'][key] = case
            print(key, json.dumps(case), flush=True)
    txt = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""What fusing the multi-label loss and accuracy into the head buys on the HPO-NEURO stand-in (subgnn_amd/standins.py:
``hpo_neuro``): ``standins.bench_config('hpo_neuro', ...)`` with hparams['fused_multilabel_loss'] True (BCE with logits + the
exact-match accuracy inside the head's launch) and False (the library calls: type_as, BCEWithLogitsLoss, sigmoid, compare, all,
mean and their autograd), alternating, in ONE process -> ms per recorded and per eager training step and the kernels an eager
step launches, each run listed and the median of each side reported.

    python tools/multilabel_head_probe.py [--rounds 2] [--steps 300] [--out profiles/multilabel_head_probe.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402

from subgnn_amd import standins                                # noqa: E402


def one(fused, steps, warmup):
    r = standins.bench_config('hpo_neuro', steps=steps, warmup=warmup, hp_over={'fused_multilabel_loss': fused})
    return {'fused_multilabel_loss': fused, 'recorded_step_ms': round(r['ms_per_step'], 4),
            'eager_step_ms': round(r['eager']['ms_per_step'], 4), 'kernels_per_eager_step': r['kernels_per_step'],
            'loss': r['loss'], 'loss_recorded': r['loss_graph'], 'prepare_data_s': r['prepare_data_s'],
            'structure_patches': r['config']['structure_patches'], 'workload': r['config']['workload']}


def median(v):
    v = sorted(v)
    return v[(len(v) - 1) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('multilabel_head_probe: no GPU (a time is measured on the device or not at all)')
    runs = []
    for _ in range(args.rounds):
        for fused in (True, False):
            runs.append(one(fused, args.steps, args.warmup))
            print(json.dumps(runs[-1]), flush=True)
    side = {}
    for fused in (True, False):
        mine = [r for r in runs if r['fused_multilabel_loss'] is fused]
        side['fused' if fused else 'library'] = {
            'recorded_step_ms': median([r['recorded_step_ms'] for r in mine]), 'eager_step_ms': median([r['eager_step_ms'] for r in mine]),
            'kernels_per_eager_step': mine[0]['kernels_per_eager_step']}
    out = {'what': "hpo_neuro stand-in, batch of 128, training step = fwd + bwd + clip + Adam; hparams['fused_multilabel_loss'] True "
                   '(fused) against False (library: the path before the multi-label head); medians over the runs of each side',
           'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, **side,
           'recorded_step_ratio_fused_over_library': round(side['fused']['recorded_step_ms'] / side['library']['recorded_step_ms'], 4),
           'eager_step_ratio_fused_over_library': round(side['fused']['eager_step_ms'] / side['library']['eager_step_ms'], 4),
           'runs': runs}
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()

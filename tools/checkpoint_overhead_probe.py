#!/usr/bin/env python3
"""What keeping the best epoch costs: standins.time_epochs on each stand-in with checkpoint_k = 0 and = 1, the two settings
alternating in one process on one prepared model, so that both see the same device and heap state.  Per setting: the median
epoch of every repetition (epochs 2.. of each fit) and the spread between repetitions; for checkpoint_k = 1 also the time of
the epochs that took a snapshot (the device copy, synchronised by the phase timer) and the one-time write when fit returns.

    python tools/checkpoint_overhead_probe.py [--configs density_n,ppi_bp,hpo_metab,em_user] [--epochs 6] [--reps 3] [--out f.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402

from subgnn_amd import standins                                # noqa: E402


def probe(name, epochs, reps, root):
    model, _, _ = standins.build_model(root, name)
    hp = model.hparams
    runs = {0: [], 1: []}
    for rep in range(reps):
        for k in ((0, 1) if rep % 2 == 0 else (1, 0)):
            kw = {'checkpoint_dir': os.path.join(root, 'ck_%s_%d' % (name, rep)), 'checkpoint_k': 1} if k else None
            runs[k].append(standins.time_epochs(model, hp, epochs, trainer_kw=kw))
    out = {}
    for k, rs in runs.items():
        med = [r['epoch_ms'] for r in rs]
        ent = {'epoch_ms_median_per_rep': med, 'epoch_ms': round(statistics.median(med), 3),
               'epoch_ms_spread': round(max(med) - min(med), 3), 'epoch_ms_fastest': min(r['epoch_ms_fastest'] for r in rs)}
        if k:
            kept = [v for r in rs for v in r['checkpoint_ms_of_kept_epochs']]
            ent['snapshot_ms_of_kept_epochs'] = kept
            ent['snapshot_ms_median'] = round(statistics.median(kept), 3) if kept else None
            ent['write_at_end_s'] = [r['checkpoint_write_s'] for r in rs]
        out['checkpoint_k=%d' % k] = ent
    out['delta_epoch_ms'] = round(out['checkpoint_k=1']['epoch_ms'] - out['checkpoint_k=0']['epoch_ms'], 3)
    out['state_bytes'] = sum(t.numel() * t.element_size() for t in model.state_dict().values())
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='density_n,ppi_bp,hpo_metab,em_user')
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'epochs_per_fit': args.epochs, 'reps': args.reps, 'configs': {}}
    with tempfile.TemporaryDirectory() as root:
        for name in args.configs.split(','):
            res['configs'][name] = probe(name, args.epochs, args.reps, os.path.join(root, name))
            print(name, json.dumps(res['configs'][name]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({n: (c['checkpoint_k=0']['epoch_ms'], c['checkpoint_k=1']['epoch_ms'], c['delta_epoch_ms'])
                      for n, c in res['configs'].items()}))


if __name__ == '__main__':
    main()

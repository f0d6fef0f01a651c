#!/usr/bin/env python3
"""What the weight average inside the fused Adam step costs on the PPI-BP and EM-USER stand-ins (subgnn_amd/standins.py).  Four
times per stand-in, taken in ONE process, the variants alternating round by round after a warm-up (device events would hide the
launch gaps of a replayed step: wall time between two synchronisations over ``--steps`` replays, median of the rounds [min - max]):

  a  the replayed training step, ema_decay = 0                     (sgnn_optim_adam)
  b  the replayed training step, ema_decay = 0.999                  (sgnn_optim_adam_ema: the average moves inside the update)
  c  the steps of a, each followed by torch._foreach_lerp_ over all parameters (the average done from outside the recording)
  d  the two exchanges of an epoch (ClipAdam.swap_ema twice: before and after the validation), per pair

``--kernels``: one more run of this file under ``rocprofv3 --kernel-trace --stats`` (a child process of its own, the program after
``--``) for the device times of optim_adam_kernel<false> / <true> and optim_swap_kernel.
``--baseline-tree DIR`` (repeatable runs of another checkout of this project, built, e.g. the parent commit): variant a alone,
timed by the same code in child processes that import the package from DIR, alternating with child processes on this tree
(``--baseline-runs`` each) -- the acceptance of the change with every new hyper-parameter off is that this tree's times lie
within the spread of the other's.

    python tools/ema_probe.py [--configs ppi_bp,em_user] [--kernels] [--baseline-tree DIR [--baseline-runs N] [--skip-variants]]
                              [--out profiles/ema_probe.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = HERE
if '--tree' in sys.argv:                                          # (a child of --baseline-tree: the package of that checkout)
    TREE = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, TREE)
import torch                                                      # noqa: E402

from subgnn_amd import optim, standins                            # noqa: E402
from subgnn_amd.graph_step import CapturedTrainStep               # noqa: E402

DECAY = 0.999


def stats(xs):
    xs = sorted(xs)
    return {'median_ms': round(xs[(len(xs) - 1) // 2], 4), 'min_ms': round(xs[0], 4), 'max_ms': round(xs[-1], 4)}


def batches(model, B):
    while True:
        for idx in model.train_dataloader().index_batches():
            if idx.numel() == B:
                yield idx


def recorded(root, name, **opt_kw):
    """A prepared stand-in, its optimizer and its recorded step (three eager warm-ups and the recording done)."""
    model, _, _ = standins.build_model(root, name)
    hp = model.hparams
    opt = optim.accelerate(model.configure_optimizers(), hp['grad_clip'], capturable=True, **opt_kw)
    cap = CapturedTrainStep(model, opt, hp['batch_size'], hp['grad_clip'])
    it = batches(model, hp['batch_size'])
    model.train()
    for _ in range(5):
        cap.replay(next(it))
    assert cap.graph is not None
    return model, opt, cap, it


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def probe_baseline(name, root, steps, rounds):
    """Variant a alone: what a checkout without the change can run too."""
    _, _, cap, it = recorded(root, name)
    timed(lambda: cap.replay(next(it)), steps)
    return [timed(lambda: cap.replay(next(it)), steps) for _ in range(rounds)]


def probe(name, root, steps, rounds):
    ma, oa, ca, ia = recorded(root, name)
    mb, ob, cb, ib = recorded(root, name, ema_decay=DECAY)
    params = [p for p in oa.all if p.numel()]
    outside = [p.detach().clone() for p in params]                # the average kept from outside the recording

    def a():
        ca.replay(next(ia))

    def b():
        cb.replay(next(ib))

    def c():
        ca.replay(next(ia))
        with torch.no_grad():
            torch._foreach_lerp_(outside, [p.detach() for p in params], 1.0 - DECAY)

    def d():
        ob.swap_ema()
        ob.swap_ema()
    variants = (('a_step', a), ('b_step_ema', b), ('c_step_then_foreach_lerp', c), ('d_two_swaps', d))
    for _, fn in variants:                                        # warm-up: every variant once through
        timed(fn, steps)
    runs = {k: [] for k, _ in variants}
    for _ in range(rounds):
        for k, fn in variants:
            runs[k].append(timed(fn, steps))
    table = ma.node_embeddings.weight
    seen = next(iter(ob.tail.seen.values()), None)
    out = {'batch_size': ma.hparams['batch_size'], 'parameters': len(params), 'table_rows': int(table.shape[0]),
           'table_mb': round(table.numel() * 4 / 2 ** 20, 1),
           'table_rows_stepped_fraction': round(float(seen.float().mean()), 4) if seen is not None else None,
           'steps_per_round': steps, 'rounds': rounds}
    out.update({k: stats(v) for k, v in runs.items()})
    out['ema_in_kernel_over_step_ms'] = round(out['b_step_ema']['median_ms'] - out['a_step']['median_ms'], 4)
    out['ema_foreach_over_step_ms'] = round(out['c_step_then_foreach_lerp']['median_ms'] - out['a_step']['median_ms'], 4)
    return out


def kernel_times(configs, steps):
    """Device time per call of the optimizer kernels, from one rocprofv3 --kernel-trace --stats run of this file."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'ema', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--configs', configs, '--steps', str(steps), '--rounds', '1']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {'error': (r.stdout + r.stderr)[-600:]}
        out = {}
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                nm = row.get('Name', '')
                if 'optim_adam_kernel' in nm or 'optim_swap_kernel' in nm or 'optim_sumsq_kernel' in nm:
                    key = ('optim_adam_kernel<true>' if 'optim_adam_kernel<true>' in nm or 'ILb1' in nm else
                           'optim_adam_kernel<false>' if 'optim_adam_kernel' in nm else
                           'optim_swap_kernel' if 'swap' in nm else 'optim_sumsq_kernel')
                    out[key] = {'calls': int(row['Calls']), 'mean_us': round(float(row['AverageNs']) / 1e3, 2),
                                'min_us': round(float(row['MinNs']) / 1e3, 2), 'max_us': round(float(row['MaxNs']) / 1e3, 2)}
        return out or {'error': 'no optimizer kernel in the stats of ' + d}


def against_baseline(tree, configs, steps, rounds, runs):
    """Variant a in child processes, this tree and ``tree`` alternating -> per config the runs' medians of both sides."""
    res = {name: {'this': [], 'baseline': []} for name in configs}
    for _ in range(runs):
        for side, t in (('baseline', tree), ('this', HERE)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--tree', t, '--baseline-only', '--configs',
                                ','.join(configs), '--steps', str(steps), '--rounds', str(rounds)],
                               capture_output=True, text=True, timeout=900, cwd=t)
            if r.returncode != 0:
                raise RuntimeError('%s child failed: %s' % (side, (r.stdout + r.stderr)[-800:]))
            got = json.loads(r.stdout.strip().splitlines()[-1])
            for name in configs:
                res[name][side].append(stats(got[name])['median_ms'])
    for name in configs:
        b, t = res[name]['baseline'], res[name]['this']
        res[name].update({'baseline_min_ms': min(b), 'baseline_max_ms': max(b), 'this_min_ms': min(t), 'this_max_ms': max(t),
                          'this_within_baseline_spread': [min(b) <= x <= max(b) for x in t]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='ppi_bp,em_user')
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--baseline-tree', default=None)
    ap.add_argument('--baseline-runs', type=int, default=3)
    ap.add_argument('--skip-variants', action='store_true', help='only the comparison with --baseline-tree')
    ap.add_argument('--baseline-only', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    configs = args.configs.split(',')
    with tempfile.TemporaryDirectory() as root:
        if args.baseline_only:
            print(json.dumps({name: probe_baseline(name, os.path.join(root, name), args.steps, args.rounds) for name in configs}))
            return
        res = {'device': torch.cuda.get_device_name(0), 'ema_decay': DECAY, 'configs': {}}
        for name in ([] if args.skip_variants else configs):
            res['configs'][name] = probe(name, os.path.join(root, name), args.steps, args.rounds)
            print(name, json.dumps(res['configs'][name]), flush=True)
    if args.kernels:
        res['kernels_rocprofv3'] = kernel_times(args.configs, args.steps)
        print('kernels', json.dumps(res['kernels_rocprofv3']), flush=True)
    if args.baseline_tree:
        res['step_a_against_baseline'] = against_baseline(os.path.abspath(args.baseline_tree), configs, args.steps, args.rounds,
                                                          args.baseline_runs)
        print('baseline', json.dumps(res['step_a_against_baseline']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Concurrent search trials on one MI355X: a random-sampler study on the PPI-BP and DENSITY stand-ins
(subgnn_amd/standins.py) with a fixed small epoch count, run with K = 1, 2, 4 and 8 worker processes.

For each K: trials per minute (wall clock of the whole study, worker start-up included), the median epoch time inside
a trial (between two of the trial's epoch reports: training + validation), the peak device memory of each worker, and
whether every trial's final metrics are bit-identical to the K = 1 study's (trial n has the same parameters at every K).

Before the measured studies one trial computes the similarity cache its key shares with every later trial (n_layers
and the other keyed parameters are fixed here), so every measured trial reads the same files.  This process never
opens the GPU: the stand-ins are written and their graph metrics computed in a child, the trials run in the workers.

    python tools/search_probe.py [--epochs 3,30] [--trials 8] [--workers 1,2,4,8] [--out profiles/search_probe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from subgnn_amd import search                                  # noqa: E402

SPACE = {
    "batch_size": {"type": "suggest_categorical", "args": [[64, 128]]},
    "learning_rate": {"type": "suggest_float", "args": [1e-4, 1e-3], "kwargs": {"log": True}},
    "grad_clip": {"type": "suggest_float", "args": [0.0, 0.5]},
    "lstm_dropout": {"type": "suggest_float", "args": [0.0, 0.4]},
    "lin_dropout": {"type": "suggest_float", "args": [0.0, 0.4]},
}


def timed_trial(ctx):
    """search.train_trial with the wall time of every epoch report written to trial_<n>/epoch_times.json."""
    stamps = [time.perf_counter()]
    report = ctx.report

    def timed(step, value):
        stamps.append(time.perf_counter())
        return report(step, value)
    ctx.report = timed
    value = search.train_trial(ctx)
    (ctx.dir / 'epoch_times.json').write_text(json.dumps([b - a for a, b in zip(stamps[1:], stamps[2:])]))
    return value


def write_standin(root, name):
    code = ('import sys, torch; sys.path.insert(0, %r); from subgnn_amd import standins, precompute_graph_metrics as pgm; '
            'P = standins.PRESETS[%r]; d, _ = standins.write_standin(%r, %r); '
            'pgm.calculate_stats(d, torch.device("cuda"), shortest_paths=not P["sparse"], ego=not P["sparse"]); print(d)'
            % (REPO, name, str(root), name))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError('writing the %s stand-in failed (%d):\n%s' % (name, r.returncode, r.stderr[-3000:]))
    return Path(r.stdout.strip().splitlines()[-1])


def run_config(name, task, epochs, trials):
    from subgnn_amd.standins import PRESETS
    fix = dict(PRESETS[name]['hp'])
    for k in SPACE:
        fix.pop(k, None)
    fix.update({'max_epochs': epochs, 'compute_similarities': False})
    return {'data': {'task': task}, 'tb': {'dir': 'tensorboard', 'name': 'probe'},
            'optuna': {'opt_n_trials': trials, 'opt_n_cores': 1, 'monitor_metric': 'val_micro_f1',
                       'opt_direction': 'maximize', 'sampler': 'random', 'pruning': False},
            'hyperparams_fix': fix, 'hyperparams_optuna': SPACE}


def probe(name, root, epochs, trials, workers, log):
    d = write_standin(root, name)
    cfg = run_config(name, d.name, epochs, trials)
    warm = dict(cfg, optuna=dict(cfg['optuna'], opt_n_trials=1))
    search.run_study(warm, root / ('%s_warm' % name), n_workers=1, checkpoint_k=0, project_root=root,
                     trial_fn='tools.search_probe:timed_trial', log=log)
    out, ref = {'dataset': d.name, 'epochs': epochs, 'trials': trials, 'runs': []}, None
    for k in workers:
        study = root / ('%s_k%d' % (name, k))
        t0 = time.perf_counter()
        search.run_study(cfg, study, n_workers=k, checkpoint_k=0, project_root=root,
                         trial_fn='tools.search_probe:timed_trial', log=log)
        wall = time.perf_counter() - t0
        s = search.Storage(study / search.STUDY_FILE)
        rows = s.trials()
        s.close()
        ep = sorted(x for t in rows for x in json.loads((Path(t['dir']) / 'epoch_times.json').read_text()))
        finals = {t['number']: (Path(t['dir']) / 'final_metric_scores.json').read_text() for t in rows}
        if ref is None:
            ref = finals
        peak = {}
        for t in rows:
            peak[t['worker']] = max(peak.get(t['worker'], 0), t['device_peak_bytes'] or 0)
        run = {'workers': k, 'wall_s': round(wall, 2), 'trials_per_min': round(60.0 * len(rows) / wall, 2),
               'median_epoch_s': round(ep[len(ep) // 2], 4), 'median_trial_s': round(sorted(t['wall_s'] for t in rows)[len(rows) // 2], 2),
               'peak_device_bytes_per_worker': [peak[w] for w in sorted(peak)],
               'states': sorted({t['state'] for t in rows}),
               'final_metrics_bit_identical_to_k1': finals == ref}
        log(json.dumps(run))
        out['runs'].append(run)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=str, default='3,30', help='epochs per trial: one set of studies per count')
    ap.add_argument('--trials', type=int, default=8)
    ap.add_argument('--workers', type=str, default='1,2,4,8')
    ap.add_argument('--datasets', type=str, default='ppi_bp,density_n')
    ap.add_argument('--out', type=str, default=os.path.join(REPO, 'profiles', 'search_probe.json'))
    a = ap.parse_args()
    log = lambda *m: print(*m, flush=True)
    res = {'what': 'random-sampler study on the stand-ins, K worker processes on one MI355X',
           'omp_num_threads': os.environ.get('OMP_NUM_THREADS'), 'results': {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.datasets.split(','):
            for e in [int(x) for x in a.epochs.split(',')]:
                root = Path(tmp) / ('%s_e%d' % (name, e))
                root.mkdir()
                res['results']['%s_epochs%d' % (name, e)] = probe(name, root, e, a.trials,
                                                                 [int(k) for k in a.workers.split(',')], log)
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(res, indent=2))
    print(json.dumps(res))


if __name__ == '__main__':
    main()

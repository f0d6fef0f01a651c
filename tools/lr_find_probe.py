#!/usr/bin/env python3
"""What ``Trainer.lr_find`` costs on the four stand-ins (subgnn_amd/standins.py): the wall time of a default range test (100
steps, or fewer when the loss diverges) with the step recorded once and replayed (``hip_graph_step``) and with eager steps,
each run twice on one prepared model (the first run pays the lazy initialisations of a process), next to the stand-in's
replayed training step (standins.time_steps).  The expectation for the recorded finder is about steps x replayed step plus
one recording and one snapshot; ``over_expectation_ms`` is the measured time minus steps x replayed step.

    python tools/lr_find_probe.py [--configs density_n,ppi_bp,hpo_metab,em_user] [--out profiles/lr_find_probe.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402

from subgnn_amd import optim, standins, train_config           # noqa: E402


def timed_find(model, hp, recorded):
    tr = train_config.Trainer(hp['max_epochs'], hp['grad_clip'], log=lambda *a: None, hip_graph_step=recorded)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f = tr.lr_find(model)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), f


def probe(name, root):
    model, _, _ = standins.build_model(root, name)
    hp = model.hparams
    out = {'batch_size': hp['batch_size'], 'train_subgraphs': len(model.train_sub_G)}
    for recorded in (True, False):
        runs = [timed_find(model, hp, recorded) for _ in range(2)]
        f = runs[-1][1]
        out['recorded' if recorded else 'eager'] = {'wall_ms_first': round(runs[0][0], 2), 'wall_ms': round(runs[-1][0], 2),
                                                    'steps': f.steps, 'stopped_early': f.stopped_early,
                                                    'suggestion': f.suggestion()}
    # the replayed step of this stand-in (after the finder: it leaves the model as it found it)
    opt = optim.accelerate(model.configure_optimizers(), hp['grad_clip'], capturable=True)
    step_ms, _, _ = standins.time_steps(model, opt, hp, 30, 5, graph=True)
    out['replayed_step_ms'] = round(step_ms, 4)
    rec = out['recorded']
    rec['expected_ms'] = round(rec['steps'] * step_ms, 2)
    rec['over_expectation_ms'] = round(rec['wall_ms'] - rec['expected_ms'], 2)
    rec['ms_per_step'] = round(rec['wall_ms'] / max(1, rec['steps']), 4)
    out['eager']['ms_per_step'] = round(out['eager']['wall_ms'] / max(1, out['eager']['steps']), 4)
    del model, opt
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='density_n,ppi_bp,hpo_metab,em_user')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'num_training': 100, 'configs': {}}
    with tempfile.TemporaryDirectory() as root:
        for name in args.configs.split(','):
            res['configs'][name] = probe(name, os.path.join(root, name))
            print(name, json.dumps(res['configs'][name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

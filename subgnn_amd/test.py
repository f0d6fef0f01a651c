"""Build-owned counterpart of the reference's 10-seed experiment driver (SubGNN/test.py:27-102).

For each seed: train a fresh model (train_config.train_model with ``hyperparams_fix.seed`` set to
the seed, SubGNN/test.py:63-70 -> train.py), run the test split, collect ``test_micro_f1``,
``test_acc``, ``test_auroc`` (SubGNN/test.py:84-86); then write means / standard deviations and the
per-seed lists to ``experiment_results.json`` with the reference's keys (SubGNN/test.py:88-101).
Seeds are 0..n-1, or random in [0, 10^6] with ``-random_seeds`` (SubGNN/test.py:65).

``-restoreModelPath DIR`` (the reference's flag) takes the hyper-parameters from ``DIR/hyperparams.json`` -- a search
trial's directory, e.g. the best trial of ``study_results.json`` -- and the dataset from ``-config_path``.

``-checkpoint_k k`` (k >= 1) keeps each seed's k best epochs by the monitored metric in ``version_<i>`` and tests the best of
them: the reference's protocol (ModelCheckpoint(save_top_k=1), train.py:327-334,389-409).  The default, 0, tests the last
epoch's weights.  ``-no_train`` tests each ``version_<i>``'s best ``epoch*.ckpt`` again without training (test.py:73-82).
"""
import argparse
import copy
import json
import random
from pathlib import Path

import numpy as np

from collections import OrderedDict

from . import checkpoint, config
from .train_config import read_json, train_model


def restored_config(run_config, restore_path):
    """``run_config`` with the hyper-parameters of ``restore_path/hyperparams.json`` fixed and nothing searched."""
    cfg = copy.deepcopy(run_config)
    cfg['hyperparams_fix'] = json.loads((Path(restore_path) / 'hyperparams.json').read_text(), object_pairs_hook=OrderedDict)
    cfg['hyperparams_optuna'] = {}
    return cfg


def run_seeds(run_config, n_seeds=10, random_seeds=False, results_dir=None, log=print, checkpoint_k=0, no_train=False,
              auto_lr_find=False):
    """Returns the experiment_results dict of SubGNN/test.py:52-57.  ``checkpoint_k`` / ``no_train``: see the module's doc;
    ``auto_lr_find``: each seed's training honours the hyper-parameter (train_config.train_model's)."""
    if (checkpoint_k or no_train) and results_dir is None:
        raise ValueError('checkpoints need a results_dir')
    opt_cfg = run_config.get('optuna', {})
    monitor = opt_cfg.get('monitor_metric', 'val_micro_f1')
    mode = 'max' if opt_cfg.get('opt_direction', 'maximize') == 'maximize' else 'min'
    exp = {"test_acc_mean": 0, "test_acc_sd": 0, "test_micro_f1_mean": 0, "test_micro_f1_sd": 0,
           "test_auroc_mean": 0, "test_auroc_sd": 0, "test_acc": [], "test_micro_f1": [], "test_auroc": [],
           "call": {"task": run_config['data']['task'], "n_seeds": n_seeds, "random_seeds": bool(random_seeds)}}
    for rnd in range(n_seeds):
        seed = random.randint(0, 1000000) if random_seeds else rnd
        log('Running Round %d\nSeed used:  %d' % (rnd + 1, seed))
        cfg = copy.deepcopy(run_config)
        cfg['hyperparams_fix']['seed'] = seed
        out = Path(results_dir) / ('version_%d' % rnd) if results_dir is not None else None
        if no_train:
            name = checkpoint.best_checkpoint(out, monitor, mode)
            if name is None:
                raise FileNotFoundError('no epoch*.ckpt in %s' % (out,))
            _, model, _ = train_model(cfg, restore_path=out, restore_name=name, no_train=True, log=lambda *a: None)
        elif checkpoint_k:
            _, model, _ = train_model(cfg, results_dir=out, log=lambda *a: None, checkpoint_k=checkpoint_k, run_test=True,
                                      auto_lr_find=auto_lr_find)
        else:
            _, model, trainer = train_model(cfg, results_dir=out, log=lambda *a: None, auto_lr_find=auto_lr_find)
            trainer.test(model)
        res = model.test_results
        for k in ('test_micro_f1', 'test_acc', 'test_auroc'):
            exp[k].append(float(res[k]))
    for k in ('test_acc', 'test_micro_f1', 'test_auroc'):
        exp[k + '_mean'] = float(np.mean(exp[k]))
        exp[k + '_sd'] = float(np.std(exp[k]))
    log('OVERALL RESULTS:')
    log(exp)
    if results_dir is not None:
        Path(results_dir).mkdir(parents=True, exist_ok=True)
        with open(Path(results_dir) / 'experiment_results.json', 'w') as f:
            json.dump(exp, f, indent=4)
    return exp


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Train and test SubGNN on MI355X for several seeds')
    ap.add_argument('-config_path', type=str, required=True, help='reference-format config.json')
    ap.add_argument('-project_root', type=str, default=None)
    ap.add_argument('-results_dir', type=str, default='tensorboard_test/sg')
    ap.add_argument('-n_seeds', type=int, default=10)
    ap.add_argument('-random_seeds', action='store_true')
    ap.add_argument('-checkpoint_k', type=int, default=0, help='test each seed from its best of k kept epochs (0: the last epoch)')
    ap.add_argument('-no_train', action='store_true', help="test each version_<i>'s best epoch*.ckpt without training")
    ap.add_argument('-auto_lr_find', action='store_true',
                    help='honour the hyper-parameter auto_lr_find: a learning-rate range test before each seed trains')
    ap.add_argument('-restoreModelPath', type=str, default=None,
                    help='directory whose hyperparams.json is used (a search trial); the dataset comes from -config_path')
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.project_root:
        config.PROJECT_ROOT = Path(args.project_root)
    run_config = read_json(args.config_path)
    if args.restoreModelPath:
        run_config = restored_config(run_config, args.restoreModelPath)
    return run_seeds(run_config, args.n_seeds, args.random_seeds,
                     Path(config.PROJECT_ROOT) / args.results_dir, checkpoint_k=args.checkpoint_k, no_train=args.no_train,
                     auto_lr_find=args.auto_lr_find)


if __name__ == '__main__':
    main()

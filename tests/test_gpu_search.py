"""-m gpu: the hyper-parameter search (subgnn_amd/search.py) end to end on the ``tiny`` fixture -- concurrent trial
processes, their agreement with one process and with a standalone run, median pruning, resuming a study, the device
memory a worker holds across trials, and the seed sweep on the best trial."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from helpers import write_dataset_from_golden

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

SPACE = {
    "batch_size": {"type": "suggest_categorical", "args": [[8, 16]]},
    "learning_rate": {"type": "suggest_float", "args": [5e-3, 1e-2], "kwargs": {"log": True}},
    "grad_clip": {"type": "suggest_float", "args": [0.5, 1.0]},
    "n_layers": {"type": "suggest_int", "args": [1, 2]},
}


def _config(tiny, root, name, space=SPACE, n_trials=4, max_epochs=4, **opt):
    fix = dict(tiny.hp)
    for k in space:
        fix.pop(k, None)
    fix.update({'max_epochs': max_epochs, 'seed': 3, 'lin_dropout': 0.0, 'compute_similarities': False})
    o = {"opt_n_trials": n_trials, "opt_n_cores": 1, "monitor_metric": "val_micro_f1", "opt_direction": "maximize",
         "sampler": "random", "pruning": False}
    o.update(opt)
    cfg = {"data": {"task": "ds"}, "tb": {"tb_logging": False, "dir": "tensorboard", "name": name}, "optuna": o,
           "hyperparams_fix": fix, "hyperparams_optuna": space}
    path = root / ('%s.json' % name)
    path.write_text(json.dumps(cfg))
    return path


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, cwd=REPO, env=env, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _search(root, cfg_path, n_workers, study=None, timeout=900):
    args = ['-m', 'subgnn_amd.search', '-config_path', str(cfg_path), '-project_root', str(root), '-n_workers', str(n_workers)]
    if study is not None:
        args += ['-study_path', str(study)]
    return _run(args, timeout)


def _trials(study):
    from subgnn_amd import search
    s = search.Storage(study / search.STUDY_FILE)
    try:
        return s.trials()
    finally:
        s.close()


@pytest.fixture(scope='module')
def studies(tmp_path_factory):
    """The same 4-trial random study with two workers and with one."""
    from conftest import load_golden
    tiny = load_golden('tiny')
    root = tmp_path_factory.mktemp('search')
    write_dataset_from_golden(tiny, root, 'ds')
    cfg = _config(tiny, root, 'rand')
    _search(root, cfg, 2)
    _search(root, cfg, 1, study=root / 'one')
    return root, cfg, root / 'tensorboard' / 'rand', root / 'one'


def test_two_workers_complete_and_match_one_worker(studies):
    from subgnn_amd import checkpoint
    root, cfg, two, one = studies
    res = json.loads((two / 'study_results.json').read_text())
    t2, t1 = _trials(two), _trials(one)
    assert [t['state'] for t in t2] == ['COMPLETE'] * 4 and [t['state'] for t in t1] == ['COMPLETE'] * 4
    assert {t['worker'] for t in t2} <= {0, 1}
    for t in t2:
        d = two / ('trial_%d' % t['number'])
        names = os.listdir(d)
        assert {'hyperparams.json', 'final_metric_scores.json', checkpoint.LAST} <= set(names)
        assert len([n for n in names if n.startswith('epoch') and n.endswith('.ckpt')]) == 3
        assert checkpoint.load(d / checkpoint.LAST)[checkpoint.RESUME_KEY]['next_epoch'] == 4
        assert len(t['intermediate']) == 4 and t['value'] == max(t['intermediate'].values())
    best = max(t2, key=lambda t: (t['value'], -t['number']))
    assert res['best_trial']['number'] == best['number'] and res['best_trial']['value'] == best['value']
    assert [t['state'] for t in res['trials']] == ['COMPLETE'] * 4
    # one worker: the same parameters and, bit for bit, the same values and final metrics per trial number
    assert [(t['number'], t['params']) for t in t2] == [(t['number'], t['params']) for t in t1]
    assert [t['value'] for t in t2] == [t['value'] for t in t1]
    assert [t['intermediate'] for t in t2] == [t['intermediate'] for t in t1]
    for t in t2:
        n = 'trial_%d' % t['number']
        assert (two / n / 'final_metric_scores.json').read_text() == (one / n / 'final_metric_scores.json').read_text()


def test_worker_memory_does_not_grow_across_trials(studies):
    _, _, _, one = studies
    t = _trials(one)
    assert all(x['worker'] == 0 for x in t) and all(x['device_bytes'] is not None for x in t)
    assert t[3]['device_bytes'] <= t[1]['device_bytes'] + (16 << 20)
    assert all(x['device_peak_bytes'] >= x['device_bytes'] for x in t)


def test_trial_matches_a_standalone_run(studies):
    """Two trials with the same similarity key: one computed the shared files, the other read them (or both raced to
    compute); each reproduces bit for bit in a standalone run from a copy of its directory (the dataset's own cache)."""
    from subgnn_amd import search
    root, cfg, two, _ = studies
    t = _trials(two)
    by_key = {}
    for x in t:
        by_key.setdefault(search.cache_key(search.merged_hyperparams(json.loads(cfg.read_text()), x['params'])), []).append(x)
    pair = next(v for v in by_key.values() if len(v) >= 2)[:2]       # (4 trials, 2 values of n_layers: one key repeats)
    for x in pair:
        src = two / ('trial_%d' % x['number'])
        dst = root / ('standalone_%d' % x['number'])
        shutil.copytree(src, dst)
        _run(['-m', 'subgnn_amd.train_config', '-config_path', str(cfg), '-project_root', str(root),
              '-restoreModelPath', str(dst)])
        assert (dst / 'final_metric_scores.json').read_text() == (src / 'final_metric_scores.json').read_text()
    sims = os.listdir(root / 'ds' / 'similarities')
    assert any(n.startswith('search_') for n in sims) and any(n.endswith('.npy') for n in sims)


def test_seed_sweep_on_the_best_trial(studies):
    root, cfg, two, _ = studies
    best = json.loads((two / 'study_results.json').read_text())['best_trial']
    _run(['-m', 'subgnn_amd.test', '-restoreModelPath', best['dir'], '-config_path', str(cfg), '-project_root', str(root),
          '-n_seeds', '2', '-results_dir', 'sweep'])
    exp = json.loads((root / 'sweep' / 'experiment_results.json').read_text())
    assert len(exp['test_micro_f1']) == 2 and exp['call']['n_seeds'] == 2
    hp = json.loads((root / 'sweep' / 'version_0' / 'hyperparams.json').read_text())
    want = json.loads((root / 'tensorboard' / 'rand' / ('trial_%d' % best['number']) / 'hyperparams.json').read_text())
    assert {k: hp[k] for k in best['params']} == {k: want[k] for k in best['params']} and hp['seed'] == 0


def test_pruning_stops_a_trial_that_cannot_learn(tiny, tmp_path):
    """A grid over the learning rate with 0 last in the seed's order: the five learning trials complete, then the
    lr = 0 trial (val_loss stuck at the initial model's) is worse than their median and stops early."""
    from subgnn_amd import checkpoint, search
    write_dataset_from_golden(tiny, tmp_path, 'ds')
    space = {"learning_rate": {"type": "suggest_float", "args": [0.0, 0.02]}}
    grid = {"learning_rate": [0.012, 0.011, 0.01, 0.009, 0.008, 0.0]}
    seed = next(s for s in range(1000) if search.GridSampler(search.parse_space({'hyperparams_optuna': space}), grid, s)
                .order[-1] == 5)
    cfg = _config(tiny, tmp_path, 'prune', space=space, n_trials=10, sampler='grid', grid_search_space=grid,
                  sampler_seed=seed, pruning=True, monitor_metric='val_loss', opt_direction='minimize')
    _search(tmp_path, cfg, 1)
    study = tmp_path / 'tensorboard' / 'prune'
    t = _trials(study)
    assert len(t) == 6 and [x['state'] for x in t[:5]] == ['COMPLETE'] * 5
    assert t[5]['params']['learning_rate'] == 0.0 and t[5]['state'] == 'PRUNED'
    stopped = len(t[5]['intermediate'])
    assert stopped < 4
    st = checkpoint.load(study / 'trial_5' / checkpoint.LAST)[checkpoint.RESUME_KEY]
    assert st['next_epoch'] == stopped and len(st['history']) == stopped
    assert json.loads((study / 'study_results.json').read_text())['best_trial']['number'] < 5


def test_resume_adds_trials_and_leaves_earlier_ones(tiny, tmp_path):
    write_dataset_from_golden(tiny, tmp_path, 'ds')
    cfg = _config(tiny, tmp_path, 'res', n_trials=2, max_epochs=2)
    _search(tmp_path, cfg, 1)
    study = tmp_path / 'tensorboard' / 'res'
    before = _trials(study)
    files = {p: (study / p).read_bytes() for n in (0, 1) for p in [os.path.join('trial_%d' % n, f)
                                                                   for f in os.listdir(study / ('trial_%d' % n))]}
    _search(tmp_path, cfg, 1)
    after = _trials(study)
    assert [x['number'] for x in after] == [0, 1, 2, 3] and all(x['state'] == 'COMPLETE' for x in after)
    assert after[:2] == before
    assert all((study / p).read_bytes() == b for p, b in files.items())
    assert len(json.loads((study / 'study_results.json').read_text())['trials']) == 4

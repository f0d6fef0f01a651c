"""Host-only checks of the hyper-parameter search (subgnn_amd/search.py): the space and the samplers, the median pruner,
the study storage and its resume, the similarity-cache key, the worker processes (with a CPU-only trial function) and
the command lines that reach the search."""
import json
import math
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

from subgnn_amd import search

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
TESTS = os.path.dirname(os.path.abspath(__file__))


def _config(space, n_trials=4, sampler='random', direction='maximize', monitor='val_micro_f1', pruning=False, **opt):
    o = {'opt_n_trials': n_trials, 'opt_n_cores': 1, 'monitor_metric': monitor, 'opt_direction': direction,
         'sampler': sampler, 'pruning': pruning}
    o.update(opt)
    return {'data': {'task': 'ds'}, 'tb': {'dir': 'tb', 'name': 'st'}, 'optuna': o,
            'hyperparams_fix': {'max_epochs': 3, 'seed': 1}, 'hyperparams_optuna': space}


SPACE = OrderedDict([
    ('batch_size', {'type': 'suggest_categorical', 'args': [[8, 16, 32]]}),
    ('learning_rate', {'type': 'suggest_float', 'args': [1e-4, 1e-2], 'kwargs': {'log': True}}),
    ('grad_clip', {'type': 'suggest_float', 'args': [0.0, 0.5]}),
    ('n_layers', {'type': 'suggest_int', 'args': [1, 7], 'kwargs': {'step': 2}}),
    ('walks', {'type': 'suggest_int', 'args': [2, 64], 'kwargs': {'log': True}}),
    ('drop', {'type': 'suggest_uniform', 'args': [0.1, 0.3]}),
    ('lr2', {'type': 'suggest_loguniform', 'args': [1e-5, 1e-1]}),
    ('q', {'type': 'suggest_discrete_uniform', 'args': [0.0, 1.0, 0.25]}),
])


# -- a CPU-only trial function for the worker processes (imported there by name) ---------------------------------------------
def fake_trial(ctx):
    """value = a function of the parameters; ``run_config['fake']``: {'exit_at': n} ends the worker with status 3 at trial n,
    {'raise_at': n} raises, {'steps': s} reports s epochs (value + step / 100) through ctx.report, stopping when told to."""
    fake = ctx.run_config.get('fake', {})
    if fake.get('exit_at') == ctx.number:
        sys.stdout.flush()
        os._exit(3)
    if fake.get('raise_at') == ctx.number:
        raise RuntimeError('trial %d raises' % ctx.number)
    v = float(sum(float(x) for x in ctx.params.values() if isinstance(x, (int, float))))
    if fake.get('per_trial'):
        v = float(fake['per_trial'][str(ctx.number)])
    ctx.dir.mkdir(parents=True, exist_ok=True)
    (ctx.dir / 'hyperparams.json').write_text(json.dumps(ctx.hp))
    for s in range(fake.get('steps', 0)):
        if ctx.report(s, v + s / 100.0):
            break
    return v


def _study(tmp_path, cfg, n_workers=1, name='st'):
    sys.path.insert(0, TESTS) if TESTS not in sys.path else None
    return search.run_study(cfg, tmp_path / name, n_workers=n_workers, trial_fn='test_search_host:fake_trial',
                            project_root=tmp_path, log=lambda *a: None)


def _trials(tmp_path, name='st'):
    s = search.Storage(tmp_path / name / search.STUDY_FILE)
    try:
        return s.trials()
    finally:
        s.close()


# -- space and the random sampler -------------------------------------------------------------------------------------------
def test_random_sampler_bounds_steps_and_log_scale():
    space = search.parse_space(_config(SPACE))
    smp = search.RandomSampler(space, seed=5)
    draws = [smp.sample(n, [], 'maximize')[0] for n in range(2000)]
    for d in draws:
        assert d['batch_size'] in (8, 16, 32)
        assert 1e-4 <= d['learning_rate'] <= 1e-2 and 0.0 <= d['grad_clip'] <= 0.5
        assert d['n_layers'] in (1, 3, 5, 7) and isinstance(d['n_layers'], int)
        assert 2 <= d['walks'] <= 64 and isinstance(d['walks'], int)
        assert 0.1 <= d['drop'] <= 0.3 and 1e-5 <= d['lr2'] <= 1e-1
        assert d['q'] in (0.0, 0.25, 0.5, 0.75, 1.0)
    assert {d['batch_size'] for d in draws} == {8, 16, 32}
    assert {d['n_layers'] for d in draws} == {1, 3, 5, 7}
    assert {d['q'] for d in draws} == {0.0, 0.25, 0.5, 0.75, 1.0}
    # log scale: log(x) uniform -> its mean near the log-space midpoint (the linear midpoint would be far above)
    ml = np.mean([math.log(d['learning_rate']) for d in draws])
    assert abs(ml - 0.5 * (math.log(1e-4) + math.log(1e-2))) < 0.1
    ml2 = np.mean([math.log(d['lr2']) for d in draws])           # (suggest_loguniform is log scale)
    assert abs(ml2 - 0.5 * (math.log(1e-5) + math.log(1e-1))) < 0.15
    assert min(d['walks'] for d in draws) == 2 and max(d['walks'] for d in draws) == 64


def test_unknown_type_and_bad_arguments_raise():
    with pytest.raises(ValueError, match='depth'):
        search.parse_space(_config({'depth': {'type': 'suggest_integer', 'args': [1, 2]}}))
    with pytest.raises(ValueError, match='depth'):
        search.parse_space(_config({'depth': {'type': 'suggest_int', 'args': [1]}}))
    with pytest.raises(ValueError):
        search.parse_space(_config({'x': {'type': 'suggest_float', 'args': [0.0, 1.0], 'kwargs': {'log': True}}}))


def test_random_params_depend_only_on_seed_number_and_name(tmp_path):
    space = search.parse_space(_config(SPACE))
    smp = search.RandomSampler(space, seed=11)
    fwd = [smp.sample(n, [], 'maximize')[0] for n in range(12)]
    rev = {n: smp.sample(n, [{'number': 0}], 'maximize')[0] for n in reversed(range(12))}
    assert all(fwd[n] == rev[n] for n in range(12))
    # another process
    code = ('import json, sys; sys.path.insert(0, %r); from subgnn_amd import search; from collections import OrderedDict; '
            'sp = search.parse_space({"hyperparams_optuna": json.loads(sys.argv[1], object_pairs_hook=OrderedDict)}); '
            's = search.RandomSampler(sp, seed=11); print(json.dumps([s.sample(n, [], "maximize")[0] for n in (7, 3, 11)]))'
            % REPO)
    out = subprocess.run([sys.executable, '-c', code, json.dumps(SPACE)], capture_output=True, text=True, check=True)
    other = json.loads(out.stdout)
    assert other == [json.loads(json.dumps(fwd[n])) for n in (7, 3, 11)]
    assert fwd[0] != search.RandomSampler(space, seed=12).sample(0, [], 'maximize')[0]


def test_random_study_same_trials_with_one_or_two_workers(tmp_path):
    cfg = _config(SPACE, n_trials=6)
    _study(tmp_path, cfg, 1, 'one')
    _study(tmp_path, cfg, 2, 'two')
    a, b = _trials(tmp_path, 'one'), _trials(tmp_path, 'two')
    assert [t['state'] for t in a] == ['COMPLETE'] * 6 and [t['state'] for t in b] == ['COMPLETE'] * 6
    assert [(t['number'], t['params'], t['value']) for t in a] == [(t['number'], t['params'], t['value']) for t in b]
    assert {t['worker'] for t in b} <= {0, 1}


# -- grid -------------------------------------------------------------------------------------------------------------------
GRID_SPACE = OrderedDict([('a', {'type': 'suggest_categorical', 'args': [[1, 2, 3]]}),
                          ('b', {'type': 'suggest_float', 'args': [0.0, 1.0]})])
GRID = {'a': [1, 2, 3], 'b': [0.0, 0.5]}


def test_grid_every_combination_once_with_two_workers(tmp_path):
    cfg = _config(GRID_SPACE, n_trials=10, sampler='grid', grid_search_space=GRID)
    res = _study(tmp_path, cfg, 2)
    combos = sorted((t['params']['a'], t['params']['b']) for t in res['trials'])
    assert combos == sorted((a, b) for a in GRID['a'] for b in GRID['b'])
    assert all(t['state'] == 'COMPLETE' for t in res['trials'])
    # the order is fixed by the seed
    order = [search.GridSampler(search.parse_space(cfg), GRID, 0).sample(0, [], 'maximize')[0] for _ in range(2)]
    assert order[0] == order[1]


def test_grid_ends_when_exhausted_across_invocations(tmp_path):
    cfg = _config(GRID_SPACE, n_trials=4, sampler='grid', grid_search_space=GRID)
    _study(tmp_path, cfg)
    assert len(_trials(tmp_path)) == 4
    _study(tmp_path, cfg)
    t = _trials(tmp_path)
    assert len(t) == 6 and len({(x['params']['a'], x['params']['b']) for x in t}) == 6
    _study(tmp_path, cfg)
    assert len(_trials(tmp_path)) == 6


def test_grid_missing_parameter_raises(tmp_path):
    cfg = _config(GRID_SPACE, sampler='grid', grid_search_space={'a': [1, 2]})
    with pytest.raises(ValueError, match="'?b'?"):
        search.make_sampler(cfg, search.parse_space(cfg))
    with pytest.raises(ValueError):
        _study(tmp_path, cfg)
    assert not (tmp_path / 'st' / search.STUDY_FILE).exists()


# -- TPE --------------------------------------------------------------------------------------------------------------------
def _tpe_run(seed, n=60, sampler_cls=search.TPESampler):
    space = search.parse_space(_config({'x': {'type': 'suggest_float', 'args': [0.0, 1.0]}}))
    smp = sampler_cls(space, seed=seed)
    trials = []
    for k in range(n):
        p, _ = smp.sample(k, trials, 'maximize')
        trials.append({'number': k, 'state': 'COMPLETE', 'params': p, 'value': -(p['x'] - 0.3) ** 2, 'intermediate': {}})
    return [t['params']['x'] for t in trials]


def test_tpe_concentrates_near_the_optimum_and_repeats():
    xs = _tpe_run(4)
    rnd = _tpe_run(4, sampler_cls=search.RandomSampler)
    assert xs[:10] == rnd[:10]                                    # the 10 start-up trials are random
    assert all(0.0 <= x <= 1.0 for x in xs)
    assert np.median(np.abs(np.asarray(xs[-20:]) - 0.3)) < np.median(np.abs(np.asarray(rnd[-20:]) - 0.3))
    assert np.median(np.abs(np.asarray(xs[-20:]) - 0.3)) < 0.1
    assert _tpe_run(4) == xs


def test_tpe_int_log_step_and_categorical_stay_legal():
    space = search.parse_space(_config(OrderedDict([
        ('c', {'type': 'suggest_categorical', 'args': [['u', 'v', 'w']]}),
        ('i', {'type': 'suggest_int', 'args': [1, 9], 'kwargs': {'step': 2}}),
        ('l', {'type': 'suggest_int', 'args': [2, 200], 'kwargs': {'log': True}}),
        ('f', {'type': 'suggest_float', 'args': [1e-4, 1.0], 'kwargs': {'log': True}}),
        ('q', {'type': 'suggest_discrete_uniform', 'args': [0.0, 1.0, 0.1]})])))
    smp = search.TPESampler(space, seed=0)
    trials = []
    for k in range(40):
        p, _ = smp.sample(k, trials, 'minimize')
        assert p['c'] in ('u', 'v', 'w') and p['i'] in (1, 3, 5, 7, 9) and 2 <= p['l'] <= 200 and 1e-4 <= p['f'] <= 1.0
        assert abs(p['q'] * 10 - round(p['q'] * 10)) < 1e-9 and 0.0 <= p['q'] <= 1.0
        v = (p['c'] != 'v') + abs(p['i'] - 5) + abs(math.log(p['f']))
        trials.append({'number': k, 'state': 'COMPLETE', 'params': p, 'value': v, 'intermediate': {}})
    late = [t['params']['c'] for t in trials[-15:]]
    assert late.count('v') > 5


def test_tpe_gamma_and_weights():
    assert [search.default_gamma(n) for n in (1, 10, 11, 100, 250, 1000)] == [1, 1, 2, 10, 25, 25]
    w = search.default_weights(30)
    assert len(w) == 30 and np.all(w[-25:] == 1.0) and w[0] == pytest.approx(1 / 30)
    wt, mu, sg = search.parzen_estimator([0.2, 0.8], 0.0, 1.0)
    assert list(mu) == [0.2, 0.5, 0.8] and wt.sum() == pytest.approx(1.0)
    assert sg[1] == 1.0 and sg[0] == pytest.approx(0.3) and sg[2] == pytest.approx(0.3)


# -- median pruner ----------------------------------------------------------------------------------------------------------
def test_median_pruner_hand_computed():
    done = [{'0': 0.1, '1': 0.5}, {'0': 0.2, '1': 0.6}, {'0': 0.3, '1': 0.7}, {'0': 0.4}, {'0': 0.5, '1': float('nan')}]
    mp = search.median_should_prune
    # fewer than 5 complete: never
    assert not mp('maximize', {'0': -10.0}, 0, done[:4])
    # maximize, step 0: median of 0.1..0.5 = 0.3
    assert mp('maximize', {'0': 0.29}, 0, done) and not mp('maximize', {'0': 0.3}, 0, done)
    # minimize: worse = larger
    assert mp('minimize', {'0': 0.31}, 0, done) and not mp('minimize', {'0': 0.3}, 0, done)
    # step 1: only 3 completed trials reached it with a number (nan-median of 0.5, 0.6, 0.7, nan = 0.6); the best so far
    # counts, not the last value
    assert mp('maximize', {'0': 0.1, '1': 0.55}, 1, done)
    assert not mp('maximize', {'0': 0.65, '1': 0.1}, 1, done)
    assert not mp('minimize', {'0': 0.9, '1': 0.55}, 1, done) and mp('minimize', {'0': 0.9, '1': 0.61}, 1, done)
    # a step no completed trial reached prunes nothing
    assert not mp('maximize', {'0': 0.0, '1': 0.0, '2': 0.0}, 2, done)


def test_pruning_in_a_study(tmp_path):
    vals = {'0': 0.5, '1': 0.6, '2': 0.7, '3': 0.8, '4': 0.9, '5': 0.1, '6': 0.95}
    cfg = _config(SPACE, n_trials=7, pruning=True)
    cfg['fake'] = {'steps': 4, 'per_trial': vals}
    _study(tmp_path, cfg)
    t = _trials(tmp_path)
    assert [x['state'] for x in t] == ['COMPLETE'] * 5 + ['PRUNED', 'COMPLETE']
    assert list(t[5]['intermediate']) == ['0']                    # stopped after the first report
    assert len(t[6]['intermediate']) == 4


# -- storage ----------------------------------------------------------------------------------------------------------------
def test_resume_marks_running_fail_and_continues_numbering(tmp_path):
    cfg = _config(SPACE, n_trials=3)
    d = tmp_path / 'st'
    d.mkdir()
    s = search.Storage(d / search.STUDY_FILE)
    s.check_study('maximize', 'val_micro_f1', 'random')
    inv = s.begin_invocation(5)
    smp = search.make_sampler(cfg, search.parse_space(cfg))
    assert s.claim(inv, smp, 'maximize', d)[0] == 0
    assert s.claim(inv, smp, 'maximize', d)[0] == 1
    s.close()                                                      # (a killed invocation: both left RUNNING)
    res = _study(tmp_path, cfg)
    t = _trials(tmp_path)
    assert [(x['number'], x['state']) for x in t] == [(0, 'FAIL'), (1, 'FAIL'), (2, 'COMPLETE'), (3, 'COMPLETE'),
                                                      (4, 'COMPLETE')]
    assert t[2]['params'] == smp.sample(2, [], 'maximize')[0]
    assert res['best_trial']['number'] in (2, 3, 4)
    _study(tmp_path, cfg)
    assert len(_trials(tmp_path)) == 8


@pytest.mark.parametrize('change', [{'opt_direction': 'minimize'}, {'monitor_metric': 'val_loss'}, {'sampler': 'tpe'}])
def test_changed_study_settings_raise(tmp_path, change):
    cfg = _config(SPACE, n_trials=1)
    _study(tmp_path, cfg)
    cfg['optuna'].update(change)
    with pytest.raises(ValueError, match='stored study'):
        _study(tmp_path, cfg)


def test_study_results_best_is_complete_and_lowest_number_on_ties(tmp_path):
    vals = {'0': 0.5, '1': 0.9, '2': 0.9, '3': 0.2}
    cfg = _config(SPACE, n_trials=4, direction='maximize')
    cfg['fake'] = {'per_trial': vals}
    res = _study(tmp_path, cfg)
    saved = json.loads((tmp_path / 'st' / 'study_results.json').read_text())
    assert saved['best_trial']['number'] == 1 == res['best_trial']['number']
    assert saved['direction'] == 'maximize' and saved['sampler'] == 'random' and saved['monitor'] == 'val_micro_f1'
    assert [t['number'] for t in saved['trials']] == [0, 1, 2, 3] and saved['trials'][1]['dir'].endswith('trial_1')
    trials = [{'number': 0, 'state': 'PRUNED', 'value': 0.1}, {'number': 1, 'state': 'COMPLETE', 'value': 0.3},
              {'number': 2, 'state': 'COMPLETE', 'value': 0.3}, {'number': 3, 'state': 'FAIL', 'value': None}]
    assert search.best_trial(trials, 'minimize')['number'] == 1
    assert search.best_trial(trials[:1], 'minimize') is None


# -- the similarity-cache key -----------------------------------------------------------------------------------------------
def test_cache_key_ignores_exactly_the_training_only_parameters(tiny):
    base = dict(tiny.hp)
    k0 = search.cache_key(base)
    for name in ('learning_rate', 'grad_clip', 'batch_size', 'max_epochs', 'lin_dropout', 'lstm_dropout', 'trainable_cc',
                 'auto_lr_find', 'linear_hidden_dim_1', 'linear_hidden_dim_2', 'lstm_n_layers', 'compute_similarities'):
        changed = dict(base, **{name: (not base[name]) if isinstance(base.get(name), bool) else 7777})
        assert search.cache_key(changed) == k0, name
    for name in ('n_anchor_patches_structure', 'n_layers', 'rw_beta', 'seed', 'dtw_tie_order', 'max_sim_epochs',
                 'sample_walk_len', 'n_triangular_walks', 'random_walk_len', 'neigh_sample_border_size', 'use_structure',
                 'structure_patch_type', 'embedding_type'):
        v = base.get(name)
        changed = dict(base, **{name: (not v) if isinstance(v, bool) else (v + 1 if isinstance(v, (int, float)) else 'other')})
        assert search.cache_key(changed) != k0, name
    assert search.cache_key(dict(base, some_new_parameter=1)) != k0   # (unknown parameters are in the key)
    assert search.cache_key(OrderedDict(reversed(list(base.items())))) == k0


def test_similarity_files_are_written_whole_with_np_save_bytes(tmp_path):
    from subgnn_amd.SubGNN import _save_npy
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    np.save(tmp_path / 'ref.npy', a)
    _save_npy(tmp_path / 'x.npy', a)
    assert (tmp_path / 'x.npy').read_bytes() == (tmp_path / 'ref.npy').read_bytes()
    assert sorted(os.listdir(tmp_path)) == ['ref.npy', 'x.npy']


# -- workers ----------------------------------------------------------------------------------------------------------------
def test_worker_exit_stops_the_study(tmp_path):
    cfg = _config(SPACE, n_trials=5)
    cfg['fake'] = {'exit_at': 1}
    with pytest.raises(search.StudyFailed, match='status 3'):
        _study(tmp_path, cfg)
    t = _trials(tmp_path)
    assert [(x['number'], x['state']) for x in t] == [(0, 'COMPLETE'), (1, 'FAIL')]
    assert (tmp_path / 'st' / 'study_results.json').exists() and (tmp_path / 'st' / 'worker_0.log').exists()
    # the command: non-zero, naming the worker's status and its log
    cfg_path = tmp_path / 'cfg.json'
    cfg_path.write_text(json.dumps(cfg))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, TESTS]))
    r = subprocess.run([sys.executable, '-m', 'subgnn_amd.search', '-config_path', str(cfg_path), '-study_path',
                        str(tmp_path / 'cli'), '-trial_fn', 'test_search_host:fake_trial'],
                       capture_output=True, text=True, env=env, cwd=REPO)
    assert r.returncode != 0 and 'status 3' in r.stderr and 'worker_0.log' in r.stderr
    assert [(x['number'], x['state']) for x in _trials(tmp_path, 'cli')] == [(0, 'COMPLETE'), (1, 'FAIL')]


def test_trial_that_raises_is_fail_and_stops_the_study(tmp_path):
    cfg = _config(SPACE, n_trials=5)
    cfg['fake'] = {'raise_at': 2}
    with pytest.raises(search.StudyFailed, match='status 1'):
        _study(tmp_path, cfg)
    t = _trials(tmp_path)
    assert [x['state'] for x in t] == ['COMPLETE', 'COMPLETE', 'FAIL'] and 'raises' in t[2]['error']
    assert 'RuntimeError' in (tmp_path / 'st' / 'worker_0.log').read_text()


def test_worker_count_limit(tmp_path):
    with pytest.raises(ValueError, match='n_workers'):
        _study(tmp_path, _config(SPACE), n_workers=9)
    with pytest.raises(ValueError, match='n_workers'):
        _study(tmp_path, _config(SPACE), n_workers=0)


# -- command lines ----------------------------------------------------------------------------------------------------------
def test_cli_parsing(tmp_path):
    from subgnn_amd import train_config
    from subgnn_amd import test as sweep
    a = search.parse_args(['-config_path', 'c.json', '-n_workers', '2', '-study_path', 'p'])
    assert (a.config_path, a.n_workers, a.study_path, a.checkpoint_k) == ('c.json', 2, 'p', 3)
    a = train_config.parse_args(['-config_path', 'c.json', '-search', '-n_workers', '4', '-checkpoint_k', '2'])
    assert a.search and a.n_workers == 4 and a.checkpoint_k == 2 and a.study_path is None
    a = train_config.parse_args(['-config_path', 'c.json'])
    assert not a.search and a.n_workers is None
    for bad in (['-search', '-restoreModelPath', 'd'], ['-n_workers', '2'], ['-study_path', 'p']):
        with pytest.raises(SystemExit):
            train_config.parse_args(['-config_path', 'c.json'] + bad)
    a = sweep.parse_args(['-config_path', 'c.json', '-restoreModelPath', 'st/trial_3', '-n_seeds', '2'])
    assert a.restoreModelPath == 'st/trial_3' and a.n_seeds == 2
    assert sweep.parse_args(['-config_path', 'c.json']).restoreModelPath is None
    # the sweep's config: the trial's hyper-parameters, nothing searched, the config's dataset
    (tmp_path / 'hyperparams.json').write_text(json.dumps({'learning_rate': 0.003, 'n_layers': 2, 'seed': 9}))
    rc = sweep.restored_config(_config(SPACE), tmp_path)
    assert rc['hyperparams_fix'] == {'learning_rate': 0.003, 'n_layers': 2, 'seed': 9} and rc['hyperparams_optuna'] == {}
    assert rc['data'] == {'task': 'ds'}


def test_default_study_dir(tmp_path):
    cfg = _config(SPACE)
    assert search.default_study_dir(cfg, tmp_path) == tmp_path / 'tb' / 'st'
    cfg['tb']['local'] = True
    assert str(search.default_study_dir(cfg, tmp_path)) == os.path.join('tb', 'st')


def test_fixed_trial_takes_positional_step_and_q():
    from subgnn_amd.train_config import FixedTrial, get_hyperparams
    cfg = _config(SPACE)
    hp = get_hyperparams(cfg, FixedTrial())
    assert hp['q'] == 0.0 and hp['n_layers'] == 1 and hp['batch_size'] == 8
    params = search.RandomSampler(search.parse_space(cfg), 3).sample(4, [], 'maximize')[0]
    assert get_hyperparams(cfg, FixedTrial(params)) == search.merged_hyperparams(cfg, params)

"""-m gpu: checkpoints on the tiny fixture -- the best epoch is the one kept and keeping it changes nothing, a run resumed in a
fresh process continues bit for bit, a seed sweep and the training driver test from the best checkpoint (in process and from
the files alone), the reference's checkpoint format loads both ways, and a resume into another model or optimizer is refused."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from helpers import T, assert_close, write_dataset_from_golden

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _config(tiny, tmp_path, **over):
    from subgnn_amd import config
    if not (tmp_path / 'ds').exists():
        write_dataset_from_golden(tiny, tmp_path, 'ds')
        if over.get('node_embed_size', 8) != 8:                           # (a wider table: the sizes the fused LSTM takes)
            g = torch.Generator().manual_seed(5)
            n = len(tiny['embeddings']) - 1
            torch.save(torch.randn(n, over['node_embed_size'], generator=g), tmp_path / 'ds' / 'gin_embeddings.pth')
    config.PROJECT_ROOT = tmp_path
    fix = dict(tiny.hp)
    fix.update({'max_epochs': 6, 'seed': 3, 'lin_dropout': 0.3, 'batch_size': 4, 'learning_rate': 0.01,
                'compute_similarities': True})
    fix.update(over)
    rc = {'data': {'task': 'ds'}, 'optuna': {'monitor_metric': 'val_micro_f1', 'opt_direction': 'maximize'},
          'hyperparams_fix': fix}
    path = tmp_path / ('config_%d.json' % len(list(tmp_path.glob('config_*.json'))))
    path.write_text(json.dumps(rc))
    return rc, path


def _train(rc, out=None, **kw):
    from subgnn_amd import train_config
    return train_config.train_model(rc, results_dir=out, log=lambda *a: None, **kw)


def _child(module, *args):
    r = subprocess.run([sys.executable, '-m', module] + [str(a) for a in args], cwd=REPO, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _epoch_files(d):
    return sorted(n for n in os.listdir(d) if n.startswith('epoch') and n.endswith('.ckpt'))


def _same(a, b, where='root'):
    """Bitwise equality of nested checkpoint contents (NaN equals NaN)."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, where
        a, b = a.cpu(), b.cpu()
        assert torch.equal(a, b) or (a.is_floating_point() and torch.equal(torch.isnan(a), torch.isnan(b))
                                     and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])), where
    elif isinstance(a, dict):
        assert set(a) == set(b), (where, set(a) ^ set(b))
        for k in a:
            _same(a[k], b[k], '%s.%s' % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (where, i))
    elif isinstance(a, float) or hasattr(a, 'dtype'):
        assert float(a) == float(b) or (math.isnan(float(a)) and math.isnan(float(b))), (where, a, b)
    else:
        assert a == b, (where, a, b)


def test_best_epoch_is_the_one_kept(tiny, tmp_path):
    from subgnn_amd import checkpoint
    rc, _ = _config(tiny, tmp_path)
    _, model, trainer = _train(rc, tmp_path / 'k1', checkpoint_k=1)
    files = _epoch_files(tmp_path / 'k1')
    assert len(files) == 1 and (tmp_path / 'k1' / checkpoint.LAST).exists()
    vals = [h['val_micro_f1'] for h in trainer.history]
    best = vals.index(max(vals))
    ck = torch.load(tmp_path / 'k1' / files[0], weights_only=True)         # (a plain load: tensors, numbers and strings only)
    assert ck['epoch'] == best and files[0].startswith('epoch=%d-val_micro_f1=%.2f-' % (best, vals[best]))
    assert {'epoch', 'global_step', 'state_dict', 'optimizer_states'} <= set(ck)
    assert all(not t.is_cuda for t in ck['state_dict'].values())
    # the same seed stopped after that epoch has exactly these weights
    rc2, _ = _config(tiny, tmp_path, max_epochs=best + 1)
    _, stopped, tr2 = _train(rc2)
    own = stopped.state_dict()
    assert set(own) == set(ck['state_dict'])
    for k, v in own.items():
        assert torch.equal(v.cpu(), ck['state_dict'][k]), k
    assert ck['global_step'] == tr2.global_step
    # loading into the trained model copies into its tensors (a recorded step keeps reading them)
    ptrs = {k: v.data_ptr() for k, v in model.state_dict().items()}
    checkpoint.load_checkpoint(model, tmp_path / 'k1' / files[0])
    for k, v in model.state_dict().items():
        assert v.data_ptr() == ptrs[k] and torch.equal(v.cpu(), ck['state_dict'][k]), k
    # k = 3: the three best, the earliest first among equal values
    _, _, tr3 = _train(rc, tmp_path / 'k3', checkpoint_k=3)
    vals = [h['val_micro_f1'] for h in tr3.history]
    want = sorted(sorted(range(len(vals)), key=lambda e: (-vals[e], e))[:3])
    got = sorted(torch.load(tmp_path / 'k3' / f, weights_only=True)['epoch'] for f in _epoch_files(tmp_path / 'k3'))
    assert got == want, (vals, got)


def test_checkpointing_does_not_perturb_training(tiny, tmp_path):
    rc, _ = _config(tiny, tmp_path)
    runs = []
    for k in (0, 1):
        _, m, tr = _train(rc, tmp_path / ('k%d' % k), checkpoint_k=k)
        runs.append((tr.history, m.metric_scores, {n: v.detach().cpu() for n, v in m.state_dict().items()}))
    assert not (tmp_path / 'k0' / 'last.ckpt').exists() and _epoch_files(tmp_path / 'k0') == []
    _same(runs[0], runs[1])


RESUME_CASES = {
    'replayed': {},
    'eager': {'hip_graph_step': False},
    'resampled': {'resample_anchor_patches': True},
    'lstm2_dropout_fused': {'lstm_n_layers': 2, 'lstm_dropout': 0.3, 'node_embed_size': 32},
    'lstm2_dropout_library': {'lstm_n_layers': 2, 'lstm_dropout': 0.3},
}


@pytest.mark.parametrize('case', list(RESUME_CASES))
def test_resume_in_a_fresh_process_is_bit_exact(tiny, tmp_path, case):
    from subgnn_amd import ops
    over = RESUME_CASES[case]
    rc3, cfg3 = _config(tiny, tmp_path, max_epochs=3, **over)
    _train(rc3, tmp_path / 'resumed', checkpoint_k=1)
    D = over.get('node_embed_size', 8)
    assert case != 'lstm2_dropout_fused' or ops.lstm_supported(D, D)
    if over.get('lstm_dropout') and not ops.lstm_supported(D, D):
        # the library LSTM's dropout state cannot be restored: refused, never continued on another trajectory
        with pytest.raises(ValueError, match='lstm_dropout'):
            _train(rc3, restore_path=tmp_path / 'resumed', resume=True, max_epochs=6)
        return
    rc, _ = _config(tiny, tmp_path, **over)
    _train(rc, tmp_path / 'straight', checkpoint_k=1)
    _child('subgnn_amd.train_config', '-config_path', cfg3, '-project_root', tmp_path,
           '-restoreModelPath', tmp_path / 'resumed', '-resume', '-max_epochs', 6)
    a = torch.load(tmp_path / 'straight' / 'last.ckpt', weights_only=False)
    b = torch.load(tmp_path / 'resumed' / 'last.ckpt', weights_only=False)
    _same(a['state_dict'], b['state_dict'], 'state_dict')
    _same(a['optimizer_states'], b['optimizer_states'], 'optimizer')      # every moment and step count
    ra, rb = a['subgnn_amd_resume'], b['subgnn_amd_resume']
    assert ra['next_epoch'] == rb['next_epoch'] == 6 and a['global_step'] == b['global_step']
    for k in ('history', 'metric_scores', 'best', 'head_rng', 'resample_epoch'):
        _same(ra[k], rb[k], k)
    assert [e['epoch'] for e in ra['top_k']] == [e['epoch'] for e in rb['top_k']]
    assert _epoch_files(tmp_path / 'straight') == _epoch_files(tmp_path / 'resumed')


def test_seed_sweep_tests_the_best_checkpoint(tiny, tmp_path):
    from subgnn_amd import checkpoint, train_config
    from subgnn_amd import test as sweep
    rc, cfg = _config(tiny, tmp_path, max_epochs=4)
    exp = sweep.run_seeds(rc, n_seeds=2, results_dir=tmp_path / 'sweep', log=lambda *a: None, checkpoint_k=1)
    for i in range(2):
        d = tmp_path / 'sweep' / ('version_%d' % i)
        files = _epoch_files(d)
        assert len(files) == 1
        hp = json.loads((d / 'hyperparams.json').read_text())
        assert hp['seed'] == i
        model, _ = train_config.build_model(rc, hp=hp)
        model.prepare_data()
        checkpoint.load_checkpoint(model, d / files[0])
        train_config.Trainer(1, log=lambda *a: None).test(model)
        for k in ('test_micro_f1', 'test_acc', 'test_auroc'):
            assert float(model.test_results[k]) == exp[k][i], (i, k)
    _child('subgnn_amd.test', '-config_path', cfg, '-project_root', tmp_path, '-results_dir', 'sweep', '-n_seeds', 2,
           '-checkpoint_k', 1, '-no_train')
    again = json.loads((tmp_path / 'sweep' / 'experiment_results.json').read_text())
    for k in ('test_micro_f1', 'test_acc', 'test_auroc'):
        assert again[k] == exp[k], k


def test_driver_tests_a_restored_model_without_training(tiny, tmp_path):
    rc, cfg = _config(tiny, tmp_path, max_epochs=4)
    _, model, trainer = _train(rc, tmp_path / 'run', checkpoint_k=1, run_test=True)
    in_process = json.loads((tmp_path / 'run' / 'test_results.json').read_text())
    assert in_process['test_micro_f1'] == float(model.test_results['test_micro_f1'])
    (tmp_path / 'run' / 'test_results.json').unlink()
    name = _epoch_files(tmp_path / 'run')[0]
    assert trainer.best_checkpoint_path().name == name
    _child('subgnn_amd.train_config', '-config_path', cfg, '-project_root', tmp_path, '-restoreModelPath', tmp_path / 'run',
           '-restoreModelName', name, '-noTrain')
    assert json.loads((tmp_path / 'run' / 'test_results.json').read_text()) == in_process


def test_reference_format_loads_both_ways(tiny, tmp_path):
    from test_gpu_model import _inject, _model
    from subgnn_amd import checkpoint
    from subgnn_amd.SubGNN import SubGNN, dataset_paths
    g, t = tiny, 'g11_sum/'
    hp = json.loads(str(g[t + 'hparams']))
    m = _model(g, tmp_path, hp)
    sd = {k[len(t) + 3:]: T(g[k]) for k in g.files if k.startswith(t + 'sd/')}
    sd['not_in_the_model.weight'] = torch.zeros(3)
    pl = {'epoch': 4, 'global_step': 20, 'state_dict': sd}                  # a Lightning file without optimizer_states
    checkpoint.load_checkpoint(m, pl)
    _inject(m, g, t, m.hparams)
    m.train()
    logits = m._forward_batch('train', m.make_batch('train', g[t + 'idx']))
    assert_close(logits, g[t + 'logits'], 'logits after load_checkpoint')
    del sd['lin3.weight']
    with pytest.raises(RuntimeError, match='lin3.weight'):
        checkpoint.load_checkpoint(m, pl)
    # ours, read by the reference's loader (train.py:233-271) into a model built from hyperparams.json
    rc, _ = _config(tiny, tmp_path / 'run', max_epochs=2)
    _train(rc, tmp_path / 'run' / 'out', checkpoint_k=1)
    name = _epoch_files(tmp_path / 'run' / 'out')[0]
    hp = json.loads((tmp_path / 'run' / 'out' / 'hyperparams.json').read_text())
    fresh = SubGNN(hp, **dataset_paths('ds'))
    ck = torch.load(tmp_path / 'run' / 'out' / name)
    own = fresh.state_dict()
    fresh.load_state_dict({k: v for k, v in ck['state_dict'].items() if k in own})
    for k, v in fresh.state_dict().items():
        assert torch.equal(v.cpu(), ck['state_dict'][k]), k


def test_resume_refuses_another_model_or_optimizer(tiny, tmp_path):
    from subgnn_amd import train_config
    rc, _ = _config(tiny, tmp_path, max_epochs=1)
    _train(rc, tmp_path / 'base', checkpoint_k=1)
    last = tmp_path / 'base' / 'last.ckpt'
    for over, what in (({'n_layers': 1}, 'cannot resume'), ({'linear_hidden_dim_1': 12}, "'lin.weight' is")):
        rco, _ = _config(tiny, tmp_path, max_epochs=2, **over)
        m, _ = train_config.build_model(rco)
        with pytest.raises(ValueError, match=what):
            train_config.Trainer(2, log=lambda *a: None).fit(m, resume_from=last)
    # a torch Adam the trainer does not replace (weight decay) against ClipAdam, both ways
    rce, _ = _config(tiny, tmp_path, max_epochs=1, hip_graph_step=False)
    m, hp = train_config.build_model(rce)
    m.configure_optimizers = lambda: torch.optim.Adam(m.parameters(), lr=hp['learning_rate'], weight_decay=1e-6)
    train_config.Trainer(1, log=lambda *a: None, hip_graph_step=False, checkpoint_dir=tmp_path / 'adam', checkpoint_k=1).fit(m)
    m2, _ = train_config.build_model(rce)
    with pytest.raises(ValueError, match='torch.optim.adam.Adam state'):
        train_config.Trainer(2, log=lambda *a: None, hip_graph_step=False).fit(m2, resume_from=tmp_path / 'adam' / 'last.ckpt')
    m3, _ = train_config.build_model(rce)
    m3.configure_optimizers = lambda: torch.optim.Adam(m3.parameters(), lr=hp['learning_rate'], weight_decay=1e-6)
    with pytest.raises(ValueError, match='ClipAdam state'):
        train_config.Trainer(2, log=lambda *a: None).fit(m3, resume_from=last)

"""-m gpu: the learning-rate range test (subgnn_amd/lr_find.py) on the tiny fixture -- ClipAdam reading its rate from a device
table equals host rates bit for bit, one recording replays a whole schedule, Trainer.lr_find equals a plain loop of the steps it
runs, leaves the model as it was, and a fit with the finder equals a fit at the suggested rate (fresh, resumed, from the CLI)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import write_dataset_from_golden

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
QUIET = (lambda *a: None)


def _rc(tiny, root, **over):
    from subgnn_amd import config
    if not (root / 'ds').exists():
        write_dataset_from_golden(tiny, root, 'ds')
    config.PROJECT_ROOT = root
    fix = dict(tiny.hp)
    fix.update({'max_epochs': 4, 'seed': 3, 'lin_dropout': 0.3, 'batch_size': 2, 'learning_rate': 0.01, 'grad_clip': 1.0,
                'compute_similarities': True})
    fix.update(over)
    return {'data': {'task': 'ds'}, 'optuna': {'monitor_metric': 'val_micro_f1', 'opt_direction': 'maximize'},
            'hyperparams_fix': fix}


def _model(rc, prepare=True):
    from subgnn_amd import train_config
    m, _ = train_config.build_model(rc)
    if prepare:
        m.prepare_data()
    return m


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


# -- 1. the device table equals host rates ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [None, 1.0])
@pytest.mark.parametrize('capturable', [False, True])
@pytest.mark.parametrize('rates', [[1e-3, 3e-2, 7e-4], [2e-2, 5e-3]])        # (a table shorter than the steps: its last entry)
def test_table_equals_host_rates(clip, capturable, rates):
    from subgnn_amd.optim import ClipAdam
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(7)
    shapes = [(300, 16), (3,), (17,), (1,), (5, 9)]                           # a row-skip table and small, odd tensors
    base = [torch.randn(s, generator=g) for s in shapes]
    pa = [b.clone().to(dev).requires_grad_(True) for b in base]
    pb = [b.clone().to(dev).requires_grad_(True) for b in base]
    table = torch.tensor(rates, dtype=torch.float32, device=dev)
    oa = ClipAdam(pa, 0.5, max_norm=clip, big_bytes=4096, capturable=capturable, lr_schedule=table)
    ob = ClipAdam(pb, 0.5, max_norm=clip, big_bytes=4096, capturable=capturable)
    assert oa.big and oa.tail.seen                                            # (the table takes the row-skip path)
    for s in range(3):
        grads = [torch.randn(sh, generator=g) * 3 for sh in shapes]
        grads[0][torch.rand(300, generator=g) < 0.6] = 0                      # untouched rows
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.to(dev), gr.to(dev).clone()
        ob.lr = float(np.float32(rates[min(s, len(rates) - 1)]))
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
        sa, sb = oa.state[id(p)], ob.state[id(q)]
        assert torch.equal(sa['exp_avg'], sb['exp_avg']) and torch.equal(sa['exp_avg_sq'], sb['exp_avg_sq'])
    assert not torch.equal(pa[1], base[1].to(dev))


def test_scheduled_step_refuses_tensors_at_different_counts():
    from subgnn_amd.optim import ClipAdam
    dev = torch.device('cuda')
    ps = [torch.zeros(8, device=dev, requires_grad=True), torch.zeros(4, device=dev, requires_grad=True)]
    opt = ClipAdam(ps, 0.1, lr_schedule=torch.full((4,), 0.1, device=dev))
    ps[0].grad = torch.ones(8, device=dev)
    opt.step()                                                                # only the first: its count is 1, the other's 0
    ps[0].grad, ps[1].grad = torch.ones(8, device=dev), torch.ones(4, device=dev)
    with pytest.raises(ValueError):
        opt.step()
    with pytest.raises(ValueError):
        ClipAdam(ps, 0.1, lr_schedule=torch.full((4,), 0.1))                  # a host table
    from subgnn_amd import optim
    with pytest.raises(ValueError):                                           # an optimizer accelerate leaves as torch's
        optim.accelerate(torch.optim.SGD(ps, lr=0.1), lr_schedule=torch.full((4,), 0.1, device=dev))


# -- 2. one recording replays the whole schedule --------------------------------------------------------------------------------
def test_one_recording_replays_a_schedule(tiny, tmp_path, monkeypatch):
    from subgnn_amd import checkpoint, graph_step, optim
    rc = _rc(tiny, tmp_path)
    m1, m2 = _model(rc), _model(rc)
    dev = m1.device
    rates = np.float32([1e-4, 3e-3, 1e-2, 2e-3, 4e-2, 5e-4, 8e-3])
    n_rec = []
    real = graph_step.record
    monkeypatch.setattr(graph_step, 'record', lambda *a, **k: (n_rec.append(1), real(*a, **k))[1])
    o1 = optim.accelerate(m1.configure_optimizers(), 1.0, capturable=True, lr_schedule=torch.from_numpy(rates).to(dev))
    o2 = optim.accelerate(m2.configure_optimizers(), 1.0, capturable=False)
    cap = graph_step.CapturedTrainStep(m1, o1, 2, 1.0)
    m1.train()
    m2.train()
    g = torch.Generator().manual_seed(4)
    batches = [torch.randperm(len(m1.train_sub_G), generator=g)[:2] for _ in rates]
    gens = checkpoint.generator_states(dev)
    l1 = []
    for idx in batches:                                     # 3 eager warm-ups, the recording, replays
        l1.append(cap.replay(idx)[0].clone())
        assert not cap.stale()
    assert len(n_rec) == 1 and cap.graph is not None
    checkpoint.set_generator_states(gens, dev)              # (the same draws for the eager twin)
    for k, idx in enumerate(batches):
        o2.lr = float(rates[k])
        l2 = graph_step.train_step(m2, o2, m2.make_batch('train', idx.to(dev), trim=False), 1.0)[0]
        assert torch.equal(l1[k], l2), k
    _same_state(m1, m2)


# -- 3. the finder equals a plain loop ------------------------------------------------------------------------------------------
def _plain_loop(m, recorded, epochs, num_training, min_lr, max_lr, mode, clip=1.0):
    from subgnn_amd import graph_step, lr_find, optim
    rates = lr_find.schedule(min_lr, max_lr, num_training, mode)
    opt = optim.accelerate(m.configure_optimizers(), clip, capturable=False)
    sm = lr_find.Smoother(4.0)
    lrs, losses, stop = [], [], False
    m.train()
    for _ in range(epochs):
        loader = m.train_dataloader()
        batches = ((m.make_batch('train', idx, trim=False) for idx in loader.index_batches()) if recorded else iter(loader))
        for batch in batches:
            k = len(losses)
            opt.lr = float(rates[k])
            s, stop = sm.add(graph_step.train_step(m, opt, batch, clip)[0].item())
            lrs.append(float(rates[k]))
            losses.append(s)
            if stop or len(losses) >= num_training:
                break
        if stop or len(losses) >= num_training:
            break
    sugg = None
    if len(losses[10:-1]) >= 2:
        i = int(np.argmin(np.gradient(np.array(losses[10:-1])))) + 10
        sugg = lrs[i]
    return lrs, losses, stop, sugg


@pytest.mark.parametrize('recorded', [True, False])
@pytest.mark.parametrize('mode,max_lr', [('exponential', 3.0), ('linear', 0.5)])
def test_finder_equals_a_plain_loop(tiny, tmp_path, recorded, mode, max_lr):
    from subgnn_amd import train_config
    rc = _rc(tiny, tmp_path, hip_graph_step=recorded)
    m1, m2 = _model(rc), _model(rc)
    tr = train_config.Trainer(4, 1.0, log=QUIET, hip_graph_step=recorded)
    f = tr.lr_find(m1, min_lr=1e-4, max_lr=max_lr, num_training=18, mode=mode)
    lrs, losses, stop, sugg = _plain_loop(m2, recorded, 4, 18, 1e-4, max_lr, mode)
    assert f.results['lr'] == lrs
    assert np.array_equal(np.array(f.results['loss']), np.array(losses), equal_nan=True)
    assert f.stopped_early == stop and f.steps == len(losses) and (stop or f.steps == 18)
    assert f.suggestion() == sugg


# -- 4. the model is as it was --------------------------------------------------------------------------------------------------
def test_lr_find_restores_the_model(tiny, tmp_path):
    import random
    from subgnn_amd import checkpoint, train_config
    rc = _rc(tiny, tmp_path, batch_norm=True)
    m = _model(rc)
    tr = train_config.Trainer(3, 1.0, log=QUIET)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    gens = checkpoint.generator_states(m.device)
    assert m.__dict__.get('_head_rng') is None
    f = tr.lr_find(m, num_training=12, max_lr=0.5)
    assert f.steps == 12
    after = m.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert m.__dict__.get('_head_rng') is None                               # "not yet created" stays so
    g2 = checkpoint.generator_states(m.device)
    assert torch.equal(gens['torch_cpu'], g2['torch_cpu']) and torch.equal(gens['torch_cuda'], g2['torch_cuda'])
    assert all(np.array_equal(a, b) for a, b in zip(gens['numpy'][1:3], g2['numpy'][1:3])) and gens['python'] == g2['python']
    assert random.getstate() == gens['python']
    # an existing dropout state is restored in place; the finder's recording, optimizer and gradients are released
    head = m._dropout_rng()
    head[1] = 5
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    tr.lr_find(m, num_training=12, max_lr=0.5)
    torch.cuda.synchronize()
    assert m.__dict__['_head_rng'] is head and head.tolist()[1] == 5
    assert torch.cuda.memory_allocated() == mem
    assert all(p.grad is None for p in m.parameters())


# -- 5-7. fit with the finder ---------------------------------------------------------------------------------------------------
def test_fit_with_finder_equals_fit_at_the_suggestion(tiny, tmp_path):
    from subgnn_amd import train_config
    rc = _rc(tiny, tmp_path)
    m1 = _model(rc, prepare=False)
    t1 = train_config.Trainer(4, 1.0, log=QUIET, auto_lr_find=True).fit(m1)
    sugg = t1.lr_finder.suggestion()
    assert t1.lr_finder.steps >= 13 and sugg is not None
    assert m1.hparams['learning_rate'] == sugg != 0.01
    m2 = _model(rc, prepare=False)
    m2.hparams['learning_rate'] = sugg
    t2 = train_config.Trainer(4, 1.0, log=QUIET).fit(m2)
    assert t1.history == t2.history
    _same_state(m1, m2)


def test_too_few_steps_keep_the_configured_rate(tiny, tmp_path):
    from subgnn_amd import train_config
    rc = _rc(tiny, tmp_path, max_epochs=2)                                   # 2 epochs x 5 batches < 12
    m1 = _model(rc, prepare=False)
    t1 = train_config.Trainer(2, 1.0, log=QUIET, auto_lr_find=True).fit(m1)
    assert t1.lr_finder.steps == 10 and t1.lr_finder.suggestion() is None
    assert m1.hparams['learning_rate'] == 0.01
    m2 = _model(rc, prepare=False)                                          # (seeded as m1 was, after its fit)
    t2 = train_config.Trainer(2, 1.0, log=QUIET).fit(m2)
    assert t1.history == t2.history
    _same_state(m1, m2)


def test_resume_does_not_run_the_finder_again(tiny, tmp_path):
    from subgnn_amd import train_config
    rc = _rc(tiny, tmp_path, max_epochs=3, auto_lr_find=True)
    _, full, tf = train_config.train_model(rc, results_dir=tmp_path / 'full', log=QUIET, checkpoint_k=1, auto_lr_find=True)
    found = tf.lr_finder.suggestion()
    assert found is not None and full.hparams['learning_rate'] == found
    _, _, ts = train_config.train_model(rc, results_dir=tmp_path / 'cut', log=QUIET, checkpoint_k=1, auto_lr_find=True,
                                        epoch_callback=lambda e, v: e == 0)
    assert ts.lr_finder is not None and ts.stopped_epoch == 1
    _, res, tr = train_config.train_model(rc, restore_path=tmp_path / 'cut', resume=True, log=QUIET, auto_lr_find=True)
    assert tr.lr_finder is None and res.hparams['learning_rate'] == found
    assert tr.history == tf.history
    _same_state(res, full)
    ck = torch.load(tmp_path / 'cut' / 'last.ckpt', weights_only=False)
    assert ck['optimizer_states'][0]['param_groups'][0]['lr'] == found


# -- 8. the CLI flag ------------------------------------------------------------------------------------------------------------
def test_cli_flag_writes_lr_find_json(tiny, tmp_path):
    rc = _rc(tiny, tmp_path, auto_lr_find=True, max_epochs=3)
    cfg = tmp_path / 'config.json'
    cfg.write_text(json.dumps(rc))
    env = dict(os.environ, PYTHONPATH=REPO)
    for flag, out in (([], 'off'), (['-auto_lr_find'], 'on')):
        r = subprocess.run([sys.executable, '-m', 'subgnn_amd.train_config', '-config_path', str(cfg), '-project_root',
                            str(tmp_path), '-results_dir', str(tmp_path / out)] + flag,
                           cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert json.loads((tmp_path / out / 'hyperparams.json').read_text())['learning_rate'] == 0.01
    assert not (tmp_path / 'off' / 'lr_find.json').exists()
    s = json.loads((tmp_path / 'on' / 'lr_find.json').read_text())
    assert s['configured_lr'] == 0.01 and s['steps'] == 15 and len(s['lr']) == len(s['loss']) == 15
    assert {'mode', 'min_lr', 'max_lr', 'num_training', 'suggestion', 'stopped_early'} <= set(s)
    assert s['suggestion'] is not None and 'learning rate set to' in r.stdout

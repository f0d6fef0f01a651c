"""-m gpu: the training recipe in ``Trainer.fit`` on the tiny fixture -- the weight average (hparams ema_decay) is validated,
ranked, checkpointed and served without feeding back into training; a device learning-rate table (lr_schedule) equals host rates
set before each step; early stopping; and all of it resumes bit for bit."""
import os

import pytest
import torch

from helpers import write_dataset_from_golden

pytestmark = pytest.mark.gpu
QUIET = (lambda *a: None)
MON = 'val_micro_f1'


def _rc(tiny, root, **over):
    from subgnn_amd import config
    if not (root / 'ds').exists():
        write_dataset_from_golden(tiny, root, 'ds')
    config.PROJECT_ROOT = root
    fix = dict(tiny.hp)
    fix.update({'max_epochs': 4, 'seed': 3, 'lin_dropout': 0.3, 'batch_size': 2, 'learning_rate': 0.01, 'grad_clip': 1.0,
                'compute_similarities': True})
    fix.update(over)
    return {'data': {'task': 'ds'}, 'optuna': {'monitor_metric': MON, 'opt_direction': 'maximize'}, 'hyperparams_fix': fix}


def _train(rc, out=None, **kw):
    from subgnn_amd import train_config
    return train_config.train_model(rc, results_dir=out, log=QUIET, **kw)


def _epoch_files(d):
    return sorted(n for n in os.listdir(d) if n.startswith('epoch') and n.endswith('.ckpt'))


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def _validate(model):
    """The trainer's own validation path on ``model`` as it stands -> the monitored value."""
    from subgnn_amd import train_config
    tr = train_config.Trainer(1, 1.0, MON, 'max', QUIET)
    model.eval()
    with torch.no_grad():
        res = model.validation_epoch_end(tr._validation_outputs(model))
    return float(res['log'][MON])


def _same_optimizer_state(a, b):
    assert a['state'].keys() == b['state'].keys()
    for i in a['state']:
        assert a['state'][i].keys() == b['state'][i].keys()
        for k, v in a['state'][i].items():
            w = b['state'][i][k]
            assert torch.equal(v, w) if torch.is_tensor(v) else v == w, (i, k)


@pytest.fixture
def pair(tiny, tmp_path):
    """The same fit without and with the weight average, every epoch kept."""
    plain = _train(_rc(tiny, tmp_path), tmp_path / 'plain', checkpoint_k=4)
    avg = _train(_rc(tiny, tmp_path, ema_decay=0.9), tmp_path / 'avg', checkpoint_k=4)
    return plain, avg


# -- 1. the average does not feed back ------------------------------------------------------------------------------------------
def test_average_does_not_feed_back_into_training(pair, tmp_path):
    (_, m0, t0), (best1, m1, t1) = pair
    _same_state(m0, m1)                                                       # the raw weights: the same run
    assert [h['train_loss'] for h in t0.history] == [h['train_loss'] for h in t1.history]
    assert [h['epoch'] for h in t1.history] == [0, 1, 2, 3]
    # ... validated with other weights: the losses of the averaged model differ in every epoch, and it is what the trainer ranks
    assert all(a['val_loss'] != b['val_loss'] for a, b in zip(t0.history, t1.history))
    assert best1 == max(h[MON] for h in t1.history)
    opt = t1._ema_run[1]
    assert not opt.swapped and opt.param_groups[0]['ema_decay'] == 0.9
    moved = [n for n, p in m1.named_parameters() if id(p) in opt.state and not torch.equal(opt.state[id(p)]['ema'], p.detach())]
    assert len(moved) >= 4, moved
    # the test pass after the fit runs on the averaged weights and leaves the raw ones in place
    from subgnn_amd import train_config
    before = {k: v.clone() for k, v in m1.state_dict().items()}
    r1 = t1.test(m1)
    r0 = t0.test(m0)
    assert all(torch.equal(v, before[k]) for k, v in m1.state_dict().items()) and not opt.swapped
    assert float(r1['avg_test_loss']) != float(r0['avg_test_loss'])
    with pytest.raises(ValueError, match='ClipAdam'):                           # an optimizer that stays torch's keeps no average
        from subgnn_amd import optim
        optim.accelerate(torch.optim.SGD(list(m1.parameters()), lr=0.1), ema_decay=0.9)
    assert train_config.Trainer(1, log=QUIET).__dict__.get('_ema_run') is None


# -- 2. the kept files ----------------------------------------------------------------------------------------------------------
def test_kept_files_serve_the_averaged_model(pair, tiny, tmp_path):
    from subgnn_amd import checkpoint, train_config
    from subgnn_amd.predict import Predictor
    (_, _, t0), (_, _, t1) = pair
    rc = _rc(tiny, tmp_path, ema_decay=0.9)
    files = _epoch_files(tmp_path / 'avg')
    assert len(files) == 4 == len(_epoch_files(tmp_path / 'plain'))
    model, _ = train_config.build_model(rc)
    model.prepare_data()
    for f in files:
        ck = checkpoint.load(tmp_path / 'avg' / f)
        info, e = ck[checkpoint.INFO_KEY], ck['epoch']
        assert info['ema_decay'] == 0.9 and info['value'] == t1.history[e][MON]
        names = [n for n, _ in model.named_parameters()]
        assert sorted(info['ema_params']) == sorted(names)
        assert all('ema' in ent for ent in ck['optimizer_states'][0]['state'].values())
        checkpoint.load_checkpoint(model, ck, weights='ema')
        assert model.__dict__['_loaded_weights'] == 'ema'
        served = {n: p.detach().clone() for n, p in model.named_parameters()}
        assert _validate(model) == info['value'], f
        checkpoint.load_checkpoint(model, ck, weights='raw')
        for k, v in model.state_dict().items():
            assert torch.equal(v.cpu(), ck['state_dict'][k]), k
        assert _validate(model) == t0.history[e][MON], f
        checkpoint.load_checkpoint(model, tmp_path / 'avg' / f)                   # 'auto': the averaged weights
        avg = checkpoint.ema_tensors(ck)
        differs = 0
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), served[n]) and torch.equal(p.detach().cpu(), avg[n]), n
            differs += int(not torch.equal(avg[n], ck['state_dict'][n]))
        assert differs >= 4
    # a file of the run without an average: 'auto' and 'raw' are the raw weights, 'ema' is refused
    plain = checkpoint.load(tmp_path / 'plain' / _epoch_files(tmp_path / 'plain')[0])
    assert plain[checkpoint.INFO_KEY]['ema_decay'] == 0.0 and checkpoint.ema_tensors(plain) is None
    checkpoint.load_checkpoint(model, plain)
    assert model.__dict__['_loaded_weights'] == 'raw'
    with pytest.raises(ValueError, match='averaged'):
        checkpoint.load_checkpoint(model, plain, weights='ema')
    with pytest.raises(ValueError, match='weights'):
        checkpoint.load_checkpoint(model, plain, weights='best')
    # the tools' loader
    p = Predictor.from_run(rc, tmp_path / 'avg')
    best = checkpoint.load(tmp_path / 'avg' / p.restored_from)
    assert best['epoch'] == t1.top_k.best()['epoch']
    avg = checkpoint.ema_tensors(best)
    for n, q in p.model.named_parameters():
        assert torch.equal(q.detach().cpu(), avg[n]), n


# -- 3. the device table equals host rates ----------------------------------------------------------------------------------------
def test_scheduled_fit_equals_a_plain_loop_at_host_rates(tiny, tmp_path):
    from subgnn_amd import graph_step, optim, schedule, train_config
    rc = _rc(tiny, tmp_path, lr_schedule='cosine', lr_warmup_steps=2)
    m1, _ = train_config.build_model(rc)
    t1 = train_config.Trainer(4, 1.0, MON, 'max', QUIET).fit(m1)
    m2, _ = train_config.build_model(rc)                                       # (seeded as m1 was)
    m2.prepare_data()
    steps = len(m2.train_dataloader())
    table = schedule.lr_table(0.01, 4 * steps, 'cosine', 2)
    assert torch.equal(table, schedule.table_from_hparams(m2.hparams, 0.01, steps, 4)) and float(table[0]) < float(table[1])
    opt = optim.accelerate(m2.configure_optimizers(), 1.0, capturable=False)
    t2 = train_config.Trainer(4, 1.0, MON, 'max', QUIET)
    k, losses = 0, []
    for epoch in range(4):
        m2.train()
        for idx in m2.train_dataloader().index_batches():
            opt.lr = float(table[k])
            losses.append(graph_step.train_step(m2, opt, m2.make_batch('train', idx.to(m2.device), trim=False), 1.0)[0])
            k += 1
        m2.eval()
        with torch.no_grad():
            m2.validation_epoch_end(t2._validation_outputs(m2))
    assert k == 4 * steps == t1.global_step
    _same_state(m1, m2)
    plain, _ = train_config.build_model(_rc(tiny, tmp_path))
    train_config.Trainer(4, 1.0, MON, 'max', QUIET).fit(plain)
    assert not torch.equal(plain.lin.weight, m1.lin.weight)                    # (the schedule did change the run)


# -- 4. early stopping ------------------------------------------------------------------------------------------------------------
def test_early_stop_and_its_resume(tiny, tmp_path):
    from subgnn_amd import checkpoint
    rc = _rc(tiny, tmp_path, max_epochs=6, early_stop_patience=2, early_stop_min_delta=1e9)
    _, _, tr = _train(rc, tmp_path / 'es', checkpoint_k=1)
    assert len(tr.history) == 3 and tr.stopped_epoch == 3                      # nothing can improve on epoch 0
    last = checkpoint.load(tmp_path / 'es' / checkpoint.LAST)
    assert last[checkpoint.RESUME_KEY]['next_epoch'] == 3 and last['epoch'] == 2
    assert last[checkpoint.RESUME_KEY]['early_stop'] == {'best': tr.history[0][MON], 'bad': 2}
    # resumed, it stays stopped: the counter survived
    _, _, tr2 = _train(rc, restore_path=tmp_path / 'es', resume=True)
    assert tr2.history == tr.history and tr2.stopped_epoch == 3
    assert checkpoint.load(tmp_path / 'es' / checkpoint.LAST)[checkpoint.RESUME_KEY]['next_epoch'] == 3
    # a checkpoint without the entry (written before there was one) resumes with a fresh counter
    del last[checkpoint.RESUME_KEY]['early_stop']
    checkpoint.save(last, tmp_path / 'es' / checkpoint.LAST)
    _, _, tr3 = _train(rc, restore_path=tmp_path / 'es', resume=True)
    assert len(tr3.history) == 6 and tr3.stopped_epoch == 6                    # epoch 3 is its first best, two more run
    # off by default: all epochs run
    _, _, tr4 = _train(_rc(tiny, tmp_path, max_epochs=3), tmp_path / 'all')
    assert len(tr4.history) == 3 and tr4.stopped_epoch is None


# -- 5. resume ------------------------------------------------------------------------------------------------------------------
def test_recipe_resumes_bit_for_bit(tiny, tmp_path):
    from subgnn_amd import checkpoint
    rc = _rc(tiny, tmp_path, ema_decay=0.9, ema_warmup=True, lr_schedule='cosine', lr_warmup_steps=3, lr_min_ratio=0.1,
             early_stop_patience=5, early_stop_min_delta=0.0)
    _, full, tf = _train(rc, tmp_path / 'full', checkpoint_k=1)
    _, _, tc = _train(rc, tmp_path / 'cut', checkpoint_k=1, epoch_callback=lambda e, v: e == 1)
    assert tc.stopped_epoch == 2 and len(tc.history) == 2
    _, res, tr = _train(rc, restore_path=tmp_path / 'cut', resume=True)
    assert tr.history == tf.history and len(tr.history) == 4
    _same_state(res, full)
    a = checkpoint.load(tmp_path / 'full' / checkpoint.LAST)
    b = checkpoint.load(tmp_path / 'cut' / checkpoint.LAST)
    _same_optimizer_state(a['optimizer_states'][0], b['optimizer_states'][0])
    assert all('ema' in e for e in a['optimizer_states'][0]['state'].values())
    assert a['optimizer_states'][0]['state'][0]['step'] == tf.global_step
    assert a[checkpoint.RESUME_KEY]['early_stop'] == b[checkpoint.RESUME_KEY]['early_stop']
    for k in a['state_dict']:
        assert torch.equal(a['state_dict'][k], b['state_dict'][k]), k
    assert _epoch_files(tmp_path / 'full') == _epoch_files(tmp_path / 'cut')

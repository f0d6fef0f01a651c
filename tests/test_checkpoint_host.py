"""Host-only logic of the checkpoints (subgnn_amd/checkpoint.py): the top-k rule and its ties, the file names, the loader's
key handling, the choice of the best file in a directory, and the drivers' new command-line flags."""
import math

import pytest
import torch

from subgnn_amd import checkpoint as C


def _run(values, k, mode='max'):
    t = C.TopK(k, mode)
    for e, v in enumerate(values):
        enters, out = t.offer(e, v)
        if out is not None:
            t.entries.remove(out)
        if enters:
            t.entries.append({'epoch': e, 'value': v, 'file': None, 'slot': None})
    return t


def _restated(values, k, mode):
    """The k best by value, the earliest first among equal values, NaN never kept."""
    keep = [e for e, v in enumerate(values) if not math.isnan(v)]
    return sorted(sorted(keep, key=lambda e: (-values[e] if mode == 'max' else values[e], e))[:k])


@pytest.mark.parametrize('mode', ['max', 'min'])
@pytest.mark.parametrize('k', [1, 2, 3, 5])
def test_top_k_is_the_k_best_earliest_first_among_ties(k, mode):
    seqs = [[0.5, 0.5, 0.5, 0.5], [0.1, 0.3, 0.3, 0.2, 0.3, 0.9, 0.1], [0.9, 0.1, 0.9, 0.4, 0.4, 0.9],
            [float('nan'), 0.2, float('nan'), 0.2, 0.7], [0.3, 0.2, 0.1, 0.1, 0.2, 0.3]]
    g = torch.Generator().manual_seed(1)
    seqs += [[float(x) for x in torch.randint(0, 4, (12,), generator=g) / 4] for _ in range(20)]
    for s in seqs:
        t = _run(s, k, mode)
        assert sorted(e['epoch'] for e in t.entries) == _restated(s, k, mode), (s, k, mode)
        if t.entries:
            b = t.best()['epoch']
            vals = [v if not math.isnan(v) else (-math.inf if mode == 'max' else math.inf) for v in s]
            want = vals.index(max(vals) if mode == 'max' else min(vals))
            assert b == want, (s, mode)


def test_equal_value_never_displaces_and_nan_never_enters():
    t = _run([0.4, 0.4, 0.4], 1)
    assert [e['epoch'] for e in t.entries] == [0]
    t = _run([float('nan'), float('nan')], 2)
    assert t.entries == [] and t.best() is None
    t = _run([0.2, float('nan'), 0.1], 1, 'min')
    assert [e['epoch'] for e in t.entries] == [2]
    assert C.TopK(0).offer(0, 1.0) == (False, None)
    with pytest.raises(ValueError):
        C.TopK(1, 'maximize')


def test_file_name_is_lightnings():
    logs = {'val_micro_f1': torch.tensor(0.456), 'val_acc': torch.tensor(0.5), 'val_auroc': float('nan')}
    assert C.checkpoint_name(3, 'val_micro_f1', logs) == 'epoch=3-val_micro_f1=0.46-val_acc=0.50-val_auroc=nan.ckpt'
    assert C.checkpoint_name(0, 'val_acc', logs) == 'epoch=0-val_acc=0.50-val_auroc=nan.ckpt'
    n = C.checkpoint_name(12, 'val_loss', {'val_loss': 1.0, 'val_acc': 0.25, 'val_auroc': 0.75})
    assert n == 'epoch=12-val_loss=1.00-val_acc=0.25-val_auroc=0.75.ckpt'
    assert n.startswith('epoch') and n.endswith('.ckpt') and not C.LAST.startswith('epoch')


def test_load_checkpoint_drops_unknown_keys_and_refuses_missing_ones():
    m = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    src = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    sd = dict(src.state_dict())
    sd['extra.weight'] = torch.ones(1)
    ptr = m[0].weight.data_ptr()
    C.load_checkpoint(m, {'state_dict': sd, 'epoch': 0})                   # (no optimizer_states: a bare PL file)
    assert m[0].weight.data_ptr() == ptr                                  # copied into, not rebound
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), src.state_dict().values()))
    del sd['0.bias']
    with pytest.raises(RuntimeError, match='0.bias'):
        C.load_checkpoint(m, {'state_dict': sd})
    with pytest.raises(KeyError):
        C.load_checkpoint(m, {'epoch': 1})


def test_best_checkpoint_prefers_stored_values_then_names(tmp_path):
    lin = torch.nn.Linear(2, 2)
    for e, v in ((0, 0.5), (1, 0.75), (2, 0.75), (3, 0.25)):
        C.save({'epoch': e, 'state_dict': lin.state_dict(), C.INFO_KEY: {'monitor': 'val_micro_f1', 'value': v}},
               tmp_path / C.checkpoint_name(e, 'val_micro_f1', {'val_micro_f1': 0.0}))
    C.save({'epoch': 9, 'state_dict': lin.state_dict()}, tmp_path / C.LAST)
    assert C.best_checkpoint(tmp_path).startswith('epoch=1-')
    assert C.best_checkpoint(tmp_path, mode='min').startswith('epoch=3-')
    pl = tmp_path / 'pl'
    pl.mkdir()
    for e, v in ((0, 0.31), (5, 0.62), (7, 0.40)):                          # Lightning's files: the value is in the name only
        torch.save({'epoch': e, 'state_dict': lin.state_dict()}, pl / ('epoch=%d-val_micro_f1=%.2f-val_acc=0.10.ckpt' % (e, v)))
    assert C.best_checkpoint(pl) == 'epoch=5-val_micro_f1=0.62-val_acc=0.10.ckpt'
    assert C.best_checkpoint(pl, 'val_acc') == 'epoch=0-val_micro_f1=0.31-val_acc=0.10.ckpt'
    empty = tmp_path / 'none'
    empty.mkdir()
    assert C.best_checkpoint(empty) is None


def test_trainer_needs_a_directory_to_checkpoint():
    from subgnn_amd.train_config import Trainer
    with pytest.raises(ValueError):
        Trainer(1, checkpoint_k=1)
    t = Trainer(1)
    assert t.checkpoint_k == 0 and t.best_checkpoint_path() is None


def test_train_config_flags():
    from subgnn_amd.train_config import parse_args
    a = parse_args(['-config_path', 'c.json'])
    assert (a.checkpoint_k, a.restoreModelPath, a.restoreModelName, a.noTrain, a.runTest, a.resume, a.max_epochs) == \
        (0, None, None, False, False, False, None)
    a = parse_args(['-config_path', 'c.json', '-restoreModelPath', 'run', '-restoreModelName', 'epoch=1.ckpt', '-noTrain'])
    assert a.restoreModelPath == 'run' and a.restoreModelName == 'epoch=1.ckpt' and a.noTrain
    a = parse_args(['-config_path', 'c.json', '-restoreModelPath', 'run', '-resume', '-max_epochs', '9', '-checkpoint_k', '2'])
    assert a.resume and a.max_epochs == 9 and a.checkpoint_k == 2
    a = parse_args(['-config_path', 'c.json', '-checkpoint_k', '1', '-runTest', '-results_dir', 'r'])
    assert a.runTest and a.checkpoint_k == 1
    for bad in (['-resume'], ['-noTrain'], ['-restoreModelPath', 'r', '-noTrain'],
                ['-restoreModelPath', 'r', '-resume', '-restoreModelName', 'x.ckpt']):
        with pytest.raises(SystemExit):
            parse_args(['-config_path', 'c.json'] + bad)


def test_seed_sweep_flags(monkeypatch):
    from subgnn_amd import test as sweep
    with pytest.raises(ValueError):
        sweep.run_seeds({'data': {'task': 'x'}}, checkpoint_k=1)
    seen = {}
    monkeypatch.setattr(sweep, 'read_json', lambda p: {'data': {'task': 'x'}})
    monkeypatch.setattr(sweep, 'run_seeds', lambda *a, **k: seen.update(k, args=a))
    sweep.main(['-config_path', 'c.json', '-checkpoint_k', '1', '-no_train', '-n_seeds', '2'])
    assert seen['checkpoint_k'] == 1 and seen['no_train'] and seen['args'][1] == 2
    sweep.main(['-config_path', 'c.json'])
    assert seen['checkpoint_k'] == 0 and not seen['no_train']

"""CPU: the host side of the training recipe (subgnn_amd/schedule.py) -- learning-rate tables against torch's schedulers, early
stopping, and the refusals of the hyper-parameters.

Tolerance of a table entry: 1 float32 ulp of float32(torch's rate).  Both sides round a float64 to float32 once, and the two
float64 values agree to ~1e-15 relative (the same closed form, or torch's recursive form of it): one rounding can split a tie at
most one ulp apart."""
import math

import numpy as np
import pytest
import torch

from subgnn_amd import schedule as S

BASE = 0.0123
TOTALS = [1, 2, 7, 40]
KINDS = [(None, {}), ('constant', {}), ('cosine', {}), ('cosine', {'min_ratio': 0.1}), ('linear', {}),
         ('linear', {'min_ratio': 0.25}), ('step', {'step_size': 3, 'gamma': 0.5}), ('step', {'step_size': 1, 'gamma': 0.9})]


def _torch_rates(total, make_scheduler):
    """The rate of each of ``total`` steps of a CPU torch.optim.Adam whose scheduler is stepped once per optimizer step."""
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.Adam([p], lr=BASE)
    sched = make_scheduler(opt)
    rates = []
    for _ in range(total):
        rates.append(opt.param_groups[0]['lr'])
        p.grad = torch.ones(3)
        opt.step()
        sched.step()
    return rates


def _assert_within_one_ulp(table, rates, what):
    assert table.dtype == torch.float32 and table.shape == (len(rates),)
    got = table.numpy()
    want = np.asarray(rates, dtype=np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(want))
    bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulp.astype(np.float64)
    assert not bad.any(), (what, got[bad], want[bad])


@pytest.mark.parametrize('total', TOTALS)
@pytest.mark.parametrize('warmup', [0, 1, 3, 50])
@pytest.mark.parametrize('kind,kw', KINDS)
def test_table_equals_lambda_lr_of_the_same_closed_form(kind, kw, warmup, total):
    table = S.lr_table(BASE, total, kind, warmup, **kw)
    rates = _torch_rates(total, lambda opt: torch.optim.lr_scheduler.LambdaLR(
        opt, lambda t: S.factor(t, total, kind, warmup, kw.get('min_ratio', 0.0), kw.get('step_size'), kw.get('gamma'))))
    _assert_within_one_ulp(table, rates, (kind, kw, warmup, total))
    # the shape itself: warm-up from base / W, the decays' end points
    t64 = table.double()
    if warmup and kind in (None, 'constant'):
        for s in range(1, total + 1):
            assert abs(float(t64[s - 1]) - BASE * min(1.0, s / warmup)) <= 1e-6 * BASE
    if warmup == 0 and kind in ('cosine', 'linear'):
        assert abs(float(t64[0]) - BASE) <= 1e-7 * BASE
        if total > 1:
            assert abs(float(t64[-1]) - kw.get('min_ratio', 0.0) * BASE) <= 1e-7 * BASE
            assert all(float(t64[i + 1]) <= float(t64[i]) for i in range(total - 1))


@pytest.mark.parametrize('total', TOTALS)
@pytest.mark.parametrize('warmup', [0, 3])
def test_cosine_and_step_equal_torchs_own_schedulers(warmup, total):
    """CosineAnnealingLR(T_max = total - 1) and StepLR, chained after LinearLR(start_factor = 1 / W, total_iters = W - 1) for
    the warm-up: chained schedulers multiply their factors, as the table does.  (Cosine with eta_min = 0: torch's recursive
    form under a chain only coincides with the closed form there.)"""
    L = torch.optim.lr_scheduler

    def chain(opt, decay):
        if warmup <= 1:
            return decay
        return L.ChainedScheduler([L.LinearLR(opt, start_factor=1.0 / warmup, end_factor=1.0, total_iters=warmup - 1), decay])
    if total > 1:
        rates = _torch_rates(total, lambda opt: chain(opt, L.CosineAnnealingLR(opt, T_max=total - 1, eta_min=0.0)))
        _assert_within_one_ulp(S.lr_table(BASE, total, 'cosine', warmup), rates, ('cosine', warmup, total))
        if warmup == 0:
            rates = _torch_rates(total, lambda opt: L.CosineAnnealingLR(opt, T_max=total - 1, eta_min=0.1 * BASE))
            _assert_within_one_ulp(S.lr_table(BASE, total, 'cosine', 0, min_ratio=0.1), rates, ('cosine eta_min', total))
    for step_size, gamma in ((3, 0.5), (1, 0.9)):
        rates = _torch_rates(total, lambda opt: chain(opt, L.StepLR(opt, step_size=step_size, gamma=gamma)))
        _assert_within_one_ulp(S.lr_table(BASE, total, 'step', warmup, step_size=step_size, gamma=gamma), rates,
                               ('step', step_size, gamma, warmup, total))


def test_table_from_hparams_counts_epochs_in_steps():
    hp = {'lr_schedule': 'step', 'lr_step_epochs': 2, 'lr_gamma': 0.5, 'lr_warmup_steps': 2}
    t = S.table_from_hparams(hp, 0.01, steps_per_epoch=3, max_epochs=5)
    assert t.shape == (15,)
    want = [0.01 * min(1.0, (s + 1) / 2) * 0.5 ** (s // 6) for s in range(15)]
    assert np.allclose(t.numpy(), np.float32(want), rtol=1e-7, atol=0)
    assert S.table_from_hparams({}, 0.01, 3, 5) is None and not S.scheduled({})
    assert S.table_from_hparams({'lr_warmup_steps': 4}, 0.01, 3, 5).shape == (15,)
    assert torch.equal(S.table_from_hparams({'lr_schedule': 'cosine'}, 0.01, 3, 5), S.lr_table(0.01, 15, 'cosine'))


# -- early stopping --------------------------------------------------------------------------------------------------------------
def _run(stop, values):
    return [stop.update(v) for v in values]


def test_early_stop_sequences():
    assert _run(S.EarlyStop(2, 0.0, 'max'), [0.5, 0.6, 0.6, 0.7, 0.7, 0.65]) == [False, False, False, False, False, True]
    assert _run(S.EarlyStop(2, 0.0, 'min'), [1.0, 0.9, 0.95, 0.8, 0.8, 0.85]) == [False, False, False, False, False, True]
    assert _run(S.EarlyStop(1, 0.0, 'max'), [0.1, 0.2, 0.2]) == [False, False, True]
    s = S.EarlyStop(3, 0.0, 'max')                                   # an improvement clears the counter
    assert _run(s, [0.5, 0.4, 0.4, 0.6, 0.5, 0.5]) == [False] * 6 and s.bad == 2 and s.best == 0.6


def test_early_stop_min_delta_on_both_sides_of_a_step():
    s = S.EarlyStop(1, 0.1, 'max')
    assert s.update(0.5) is False
    assert s.update(0.6) is True                                     # + 0.1 exactly (well: not MORE than min_delta): no improvement
    s = S.EarlyStop(1, 0.1, 'max')
    s.update(0.5)
    assert s.update(0.61) is False and s.best == 0.61
    s = S.EarlyStop(1, 0.1, 'min')
    s.update(0.5)
    assert s.update(0.41) is True and s.best == 0.5
    s = S.EarlyStop(1, 0.1, 'min')
    s.update(0.5)
    assert s.update(0.39) is False and s.best == 0.39
    big = S.EarlyStop(2, 1e9, 'max')                                 # nothing can improve on the first epoch
    assert _run(big, [0.1, 0.9, 0.95]) == [False, False, True]


def test_early_stop_nan_counts_as_no_improvement():
    s = S.EarlyStop(2, 0.0, 'max')
    assert _run(s, [float('nan'), 0.3, float('nan'), float('nan')]) == [False, False, False, True]
    assert s.best == 0.3
    s = S.EarlyStop(2, 0.0, 'min')
    assert _run(s, [float('nan'), float('nan')]) == [False, True] and s.best is None


def test_early_stop_state_round_trip_in_the_middle_of_a_run():
    values = [0.5, 0.6, 0.55, 0.58, 0.61, 0.6, 0.6, 0.6]
    whole = S.EarlyStop(3, 0.005, 'max')
    want = _run(whole, values)
    first = S.EarlyStop(3, 0.005, 'max')
    got = _run(first, values[:4])
    st = first.state()
    assert st == {'best': 0.6, 'bad': 2}
    second = S.EarlyStop(3, 0.005, 'max').load(st)
    got += _run(second, values[4:])
    assert got == want and want[-1] is True and second.state() == whole.state()
    assert S.EarlyStop(3, 0.0, 'max').load({'best': None, 'bad': 0}).state() == {'best': None, 'bad': 0}


# -- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hp', [
    {'ema_decay': 1.0}, {'ema_decay': -0.1}, {'ema_decay': 'high'}, {'ema_decay': True},
    {'ema_warmup': 1, 'ema_decay': 0.9}, {'ema_warmup': True},
    {'lr_schedule': 'plateau'}, {'lr_schedule': 'constant'},
    {'lr_warmup_steps': -1}, {'lr_warmup_steps': 2.5},
    {'lr_schedule': 'cosine', 'lr_min_ratio': 1.5}, {'lr_schedule': 'cosine', 'lr_min_ratio': -0.1}, {'lr_min_ratio': 0.1},
    {'lr_schedule': 'step'}, {'lr_schedule': 'step', 'lr_step_epochs': 2}, {'lr_schedule': 'step', 'lr_step_epochs': 0, 'lr_gamma': 0.5},
    {'lr_schedule': 'step', 'lr_step_epochs': 2, 'lr_gamma': 0.0}, {'lr_schedule': 'step', 'lr_step_epochs': 2, 'lr_gamma': float('inf')},
    {'lr_schedule': 'cosine', 'lr_gamma': 0.5}, {'lr_step_epochs': 2},
    {'early_stop_patience': 0}, {'early_stop_patience': 1.5}, {'early_stop_patience': 2, 'early_stop_min_delta': -1.0},
    {'early_stop_patience': 2, 'early_stop_min_delta': float('nan')}, {'early_stop_min_delta': 0.1},
])
def test_hyperparameter_refusals(hp):
    with pytest.raises(ValueError, match='hparams'):
        S.check_hparams(hp)


def test_accepted_hyperparameters_and_table_argument_refusals():
    for hp in ({}, {'ema_decay': 0.999, 'ema_warmup': True}, {'lr_schedule': 'constant', 'lr_warmup_steps': 5},
               {'lr_schedule': None, 'lr_warmup_steps': 5}, {'lr_schedule': 'cosine', 'lr_min_ratio': 0.01},
               {'lr_schedule': 'linear', 'lr_min_ratio': 1.0}, {'lr_schedule': 'step', 'lr_step_epochs': 3, 'lr_gamma': 0.3},
               {'early_stop_patience': 5, 'early_stop_min_delta': 0.001}, {'ema_decay': 0, 'ema_warmup': False,
                                                                           'early_stop_patience': None}):
        S.check_hparams(hp)
    for args in ((0.0, 5), (float('nan'), 5), (0.01, 0), (0.01, 2.5), (0.01, 5, 'exp'), (0.01, 5, 'cosine', -1),
                 (0.01, 5, 'cosine', 0, 2.0), (0.01, 5, 'step', 0, 0.0, None, 0.5), (0.01, 5, 'step', 0, 0.0, 2, None)):
        with pytest.raises(ValueError, match='lr_table'):
            S.lr_table(*args)
    for args in ((0, 0.0, 'max'), (2, -1.0, 'max'), (2, 0.0, 'best')):
        with pytest.raises(ValueError, match='EarlyStop'):
            S.EarlyStop(*args)
    assert math.isclose(S.factor(0, 10, 'cosine', 4), 0.25)
    S.refuse_multi_rank({'ema_decay': 0.9, 'lr_schedule': 'cosine'})       # no process group: nothing to refuse


def test_multi_rank_refusal(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_available', lambda: True)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a, **k: 2)
    S.refuse_multi_rank({})
    S.refuse_multi_rank({'early_stop_patience': 3})
    for hp in ({'ema_decay': 0.9}, {'lr_schedule': 'cosine'}, {'lr_warmup_steps': 3}):
        with pytest.raises(RuntimeError, match='multi-rank'):
            S.refuse_multi_rank(hp)

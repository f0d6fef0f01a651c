"""The learning-rate range test's host logic (subgnn_amd/lr_find.py, a restatement of Lightning 0.7.x trainer/lr_finder.py):
the two schedules, the smoothing / early stop / suggestion rules on synthetic loss curves with hand-derived outcomes, which
hyper-parameter the suggestion replaces, the drivers' -auto_lr_find flag and the library's device-table Adam entry point."""
import ctypes
import os

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _run(losses, threshold=4.0, n=None):
    """The finder's loop over a given loss curve -> LRFinder (rates: an exponential schedule over the curve's length)."""
    from subgnn_amd import lr_find
    n = n or len(losses)
    rates = lr_find.schedule(1e-6, 1.0, n)
    f = lr_find.LRFinder('exponential', 1e-6, 1.0, n)
    sm = lr_find.Smoother(threshold)
    for k, L in enumerate(losses):
        s, stop = sm.add(L)
        f.results['lr'].append(float(rates[k]))
        f.results['loss'].append(s)
        if stop:
            f.stopped_early = True
            break
    return f


def _closed_form(losses):
    """smoothed_k = sum_j 0.02 * 0.98^(k-j) L_j / (1 - 0.98^(k+1)): the recurrence unrolled."""
    out = []
    for k in range(len(losses)):
        out.append(sum(0.02 * 0.98 ** (k - j) * losses[j] for j in range(k + 1)) / (1 - 0.98 ** (k + 1)))
    return out


@pytest.mark.parametrize('mode', ['exponential', 'linear'])
@pytest.mark.parametrize('lo,hi,n', [(1e-8, 1.0, 100), (1e-5, 0.3, 7), (0.01, 0.02, 1)])
def test_schedules_are_lightnings_formulas_in_float32(mode, lo, hi, n):
    from subgnn_amd import lr_find
    got = lr_find.schedule(lo, hi, n, mode)
    if mode == 'exponential':
        want = [lo * (hi / lo) ** (k / n) for k in range(n)]
    else:
        want = [lo + (k / n) * (hi - lo) for k in range(n)]
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.array_equal(got, np.array(want, dtype=np.float64).astype(np.float32))
    assert got[0] == np.float32(lo)
    with pytest.raises(ValueError):
        lr_find.schedule(lo, hi, n, 'cosine')


def test_smoothing_is_the_debiased_moving_average():
    losses = [2.0, 1.5, 1.7, 0.9, 1.1, 0.4]
    f = _run(losses)
    assert np.allclose(f.results['loss'], _closed_form(losses), rtol=1e-12, atol=0)
    assert f.results['loss'][0] == 2.0


def test_a_sharp_drop_is_suggested_where_it_falls_steepest():
    # flat at 1 for 15 steps, then 0: the smoothed curve is 1 up to step 14 and falls after it; its central differences are
    # (s15 - s13) / 2 = -0.036, (s16 - s14) / 2 = -0.068, (s17 - s15) / 2 = -0.060, (s18 - s16) / 2 = -0.054 -> step 15
    losses = [1.0] * 15 + [0.0] * 5
    f = _run(losses)
    assert not f.stopped_early and f.steps == 20
    assert f.suggestion() == f.results['lr'][15] and f._optimal_idx == 15


def test_an_explosion_stops_the_run_and_keeps_the_stopping_entry():
    # step 12 jumps to 1000: avg = 0.98 (1 - 0.98^12) + 20 = 20.21, smoothed = 20.21 / (1 - 0.98^13) = 87.6 > 4 * best (1)
    losses = [1.0] * 12 + [1000.0] * 8
    f = _run(losses)
    assert f.stopped_early and f.steps == 13
    assert f.results['loss'][12] > 4.0 * min(f.results['loss'][:12])
    # loss[10:-1] = entries 10 and 11, both 1: a zero gradient, whose first argmin is entry 10
    assert f._optimal_idx is None and f.suggestion() == f.results['lr'][10] and f._optimal_idx == 10
    # a higher threshold lets the same curve run on
    g = _run(losses, threshold=2000.0)                  # (the smoothed loss stays below 1000)
    assert not g.stopped_early and g.steps == 20
    # no threshold: never stops
    assert _run(losses, threshold=None).steps == 20


def test_a_falling_curve_runs_to_the_end():
    losses = [1.0 - 0.01 * k for k in range(30)]
    f = _run(losses)
    assert not f.stopped_early and f.steps == 30
    s = f.suggestion()
    grad = np.gradient(np.array(f.results['loss'][10:-1]))
    assert f._optimal_idx == int(np.argmin(grad)) + 10 and s == f.results['lr'][f._optimal_idx]


@pytest.mark.parametrize('n,expect_none', [(0, True), (1, True), (11, True), (12, True), (13, False)])
def test_too_few_points_give_no_suggestion(n, expect_none):
    f = _run([1.0 - 0.01 * k for k in range(n)], n=max(n, 1))
    assert f.steps == n
    s = f.suggestion()
    assert (s is None) == expect_none
    if not expect_none:                       # loss[10:12]: two points, one central difference each side
        assert f._optimal_idx in (10, 11)
    assert f.suggestion(skip_begin=0, skip_end=0) is None           # (Lightning's slice [0:-0] is empty)


def test_a_nan_inside_is_not_filtered_out():
    # NaN at step 14: every smoothed value from 14 on is NaN, nothing compares above the threshold, the run goes on; the
    # gradient over loss[10:19] is first NaN at step 13 ((s14 - s12) / 2) and argmin returns the first NaN
    losses = [1.0 - 0.01 * k for k in range(20)]
    losses[14] = float('nan')
    f = _run(losses)
    assert not f.stopped_early and f.steps == 20
    assert all(np.isnan(f.results['loss'][14:])) and not any(np.isnan(f.results['loss'][:14]))
    assert f.suggestion() == f.results['lr'][13] and f._optimal_idx == 13


def test_the_key_the_suggestion_replaces():
    from subgnn_amd.lr_find import lr_key
    assert lr_key({'lr': 1, 'learning_rate': 2}) == 'lr'
    assert lr_key({'learning_rate': 2, 'batch_size': 3}) == 'learning_rate'
    assert lr_key({'learning_rate': 2, 'my_rate': 1}, 'my_rate') == 'my_rate'
    with pytest.raises(ValueError):
        lr_key({'learning_rate': 2}, 'my_rate')
    with pytest.raises(ValueError):
        lr_key({'batch_size': 3})


def test_summary_holds_the_run():
    f = _run([1.0] * 12 + [1000.0] * 8)
    s = f.summary(0.001)
    assert s['configured_lr'] == 0.001 and s['steps'] == 13 and s['stopped_early'] is True
    assert s['suggestion'] == f.results['lr'][10] and len(s['lr']) == len(s['loss']) == 13
    assert {'mode', 'min_lr', 'max_lr', 'num_training'} <= set(s)


def test_drivers_parse_auto_lr_find_default_off():
    from subgnn_amd import search, test, train_config
    assert train_config.parse_args(['-config_path', 'c.json']).auto_lr_find is False
    assert train_config.parse_args(['-config_path', 'c.json', '-auto_lr_find']).auto_lr_find is True
    assert search.parse_args(['-config_path', 'c.json']).auto_lr_find is False
    assert search.parse_args(['-config_path', 'c.json', '-auto_lr_find']).auto_lr_find is True
    assert test.parse_args(['-config_path', 'c.json']).auto_lr_find is False
    assert test.parse_args(['-config_path', 'c.json', '-auto_lr_find']).auto_lr_find is True
    assert train_config.Trainer(1).auto_lr_find is False and train_config.Trainer(1).lr_finder is None


def test_library_exports_the_device_table_adam():
    from subgnn_amd import _lib
    lib = _lib.load()
    assert 'sgnn_optim_adam_lr_table' in _lib.SIGNATURES
    assert 'sgnn_optim_adam_lr_table' in open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    f = lib.sgnn_optim_adam_lr_table
    bad = lib.sgnn_optim_adam_lr_table(None, None, None, None, None, None, 0, None, 1, 0.9, 0.999, 1e-8, None, None, None,
                                       None, None, None, 0, 0.0, None, None)
    assert bad != 0                                                       # no table: an argument error, reported
    assert f(None, None, None, None, None, None, 0, ctypes.c_void_p(256), 0, 0.9, 0.999, 1e-8, None, None, None, None, None,
             None, 0, 0.0, None, None) != 0                               # an empty table
    assert f(None, None, None, None, None, None, 0, ctypes.c_void_p(256), 4, 0.9, 0.999, 1e-8, None, None, None, None, None,
             None, 0, 0.0, None, None) == 0                               # nothing to update: nothing launched

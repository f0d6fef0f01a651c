"""The training recipe around the step, host side: learning-rate tables for ClipAdam's device schedule, early stopping, and the
checks of the hyper-parameters that switch them (and the weight average) on.

A host scheduler that writes ``param_groups[0]['lr']`` is frozen into a recorded step (graph_step.CapturedTrainStep: ``lr`` is a
scalar kernel argument).  The rate a recorded step can follow is a table on the device, indexed by the device step count
(``ClipAdam(lr_schedule=table)``, sgnn_optim_adam_lr_table): ``lr_table`` builds it once per fit, for every step of the run.

Hyper-parameters (all off by default; ordinary keys of a config, of ``hyperparams_optuna`` and of hyperparams.json):
  ema_decay (0), ema_warmup (false)                      the weight average of optim.ClipAdam
  lr_schedule (null | 'constant' | 'cosine' | 'linear' | 'step'), lr_warmup_steps (0), lr_min_ratio (0),
  lr_step_epochs, lr_gamma ('step' only)                 the table below
  early_stop_patience (null), early_stop_min_delta (0)   EarlyStop
"""
import math

import numpy as np
import torch

KINDS = (None, 'constant', 'cosine', 'linear', 'step')


def decay_factor(t, total_steps, kind=None, min_ratio=0.0, step_size=None, gamma=None):
    """The decay of step t + 1 (t = 0 .. total_steps - 1: the number of steps taken before it, a torch scheduler's
    ``last_epoch``) as a factor of the base rate, in Python floats (float64):
      None / 'constant'  1
      'cosine'           m + (1 - m) (1 + cos(pi t / (T - 1))) / 2       CosineAnnealingLR(T_max = T - 1, eta_min = m base)
      'linear'           1 - (1 - m) t / (T - 1)
      'step'             gamma ** (t // step_size)                         StepLR(step_size, gamma), step_size in STEPS
    with T = total_steps, m = min_ratio: 'cosine' and 'linear' reach m at the last step (T = 1: the one step runs at 1)."""
    if kind is None or kind == 'constant':
        return 1.0
    if kind == 'step':
        return float(gamma) ** (t // int(step_size))
    span = total_steps - 1
    if span <= 0:
        return 1.0
    m = float(min_ratio)
    if kind == 'cosine':
        return m + (1.0 - m) * (1.0 + math.cos(math.pi * t / span)) / 2.0
    if kind == 'linear':
        return 1.0 - (1.0 - m) * t / span
    raise ValueError('unknown lr_schedule %r (one of %s)' % (kind, ', '.join(repr(k) for k in KINDS)))


def warmup_factor(t, warmup_steps):
    """Linear warm-up: step s = t + 1 runs at s / warmup_steps of the rate it would have, from base / warmup_steps at the first
    step to the whole rate at step ``warmup_steps`` (LinearLR(start_factor = 1 / W, total_iters = W - 1)); 1 after it."""
    return (t + 1) / warmup_steps if t + 1 < warmup_steps else 1.0


def factor(t, total_steps, kind=None, warmup_steps=0, min_ratio=0.0, step_size=None, gamma=None):
    """warm-up x decay: the warm-up multiplies whichever decay runs (as chained torch schedulers multiply), so it composes
    with every kind and the decay's end point stays where it was."""
    return warmup_factor(t, warmup_steps) * decay_factor(t, total_steps, kind, min_ratio, step_size, gamma)


def lr_table(base_lr, total_steps, kind=None, warmup_steps=0, min_ratio=0.0, step_size=None, gamma=None):
    """-> float32 CPU tensor of ``total_steps`` rates: entry s - 1 is the rate of step s (what ClipAdam's ``lr_schedule`` reads
    with the step count s).  ``base_lr * factor(s - 1)`` evaluated in float64 and rounded once to float32.  ``step_size`` (kind
    'step') counts optimizer STEPS; the trainer passes lr_step_epochs x the steps of an epoch."""
    check_table_args(base_lr, total_steps, kind, warmup_steps, min_ratio, step_size, gamma)
    base = float(base_lr)
    rates = np.array([base * factor(t, int(total_steps), kind, int(warmup_steps), min_ratio, step_size, gamma)
                      for t in range(int(total_steps))], dtype=np.float64)
    return torch.from_numpy(rates.astype(np.float32))


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _whole(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_table_args(base_lr, total_steps, kind, warmup_steps, min_ratio, step_size, gamma):
    if not _number(base_lr) or not math.isfinite(base_lr) or base_lr <= 0:
        raise ValueError('lr_table: base_lr = %r must be a finite, positive number' % (base_lr,))
    if not _whole(total_steps) or total_steps < 1:
        raise ValueError('lr_table: total_steps = %r must be a whole number >= 1' % (total_steps,))
    if kind not in KINDS:
        raise ValueError('lr_table: unknown kind %r (one of %s)' % (kind, ', '.join(repr(k) for k in KINDS)))
    if not _whole(warmup_steps) or warmup_steps < 0:
        raise ValueError('lr_table: warmup_steps = %r must be a whole number >= 0' % (warmup_steps,))
    if not _number(min_ratio) or not (0.0 <= min_ratio <= 1.0):
        raise ValueError('lr_table: min_ratio = %r must lie in [0, 1]' % (min_ratio,))
    if kind == 'step':
        if not _whole(step_size) or step_size < 1:
            raise ValueError("lr_table: kind 'step' needs step_size, a whole number of steps >= 1 (got %r)" % (step_size,))
        if not _number(gamma) or not math.isfinite(gamma) or gamma <= 0:
            raise ValueError("lr_table: kind 'step' needs gamma, a finite, positive number (got %r)" % (gamma,))


def _get(hp, key, default):
    """hp[key]; an absent key and a null both mean the default."""
    v = hp.get(key)
    return default if v is None else v


def check_hparams(hp):
    """ValueError for the first of the recipe's hyper-parameters that is out of range or has no effect as configured."""
    d = _get(hp, 'ema_decay', 0)
    if not _number(d) or not (0.0 <= d < 1.0):
        raise ValueError("hparams['ema_decay'] = %r must lie in [0, 1) (0: no weight average)" % (d,))
    w = _get(hp, 'ema_warmup', False)
    if not isinstance(w, bool):
        raise ValueError("hparams['ema_warmup'] = %r must be true or false" % (w,))
    if w and d == 0:
        raise ValueError("hparams['ema_warmup'] has no meaning without hparams['ema_decay'] > 0")
    kind = hp.get('lr_schedule')
    if kind not in KINDS:
        raise ValueError("hparams['lr_schedule'] = %r: one of %s" % (kind, ', '.join(repr(k) for k in KINDS)))
    ws = _get(hp, 'lr_warmup_steps', 0)
    if not _whole(ws) or ws < 0:
        raise ValueError("hparams['lr_warmup_steps'] = %r must be a whole number >= 0" % (ws,))
    if kind == 'constant' and ws == 0:
        raise ValueError("hparams['lr_schedule'] = 'constant' only has a meaning with hparams['lr_warmup_steps'] > 0")
    m = _get(hp, 'lr_min_ratio', 0)
    if not _number(m) or not (0.0 <= m <= 1.0):
        raise ValueError("hparams['lr_min_ratio'] = %r must lie in [0, 1]" % (m,))
    if m != 0 and kind not in ('cosine', 'linear'):
        raise ValueError("hparams['lr_min_ratio'] belongs to lr_schedule 'cosine' or 'linear'")
    se, g = hp.get('lr_step_epochs'), hp.get('lr_gamma')
    if kind == 'step':
        if not _whole(se) or se < 1:
            raise ValueError("hparams['lr_schedule'] = 'step' needs hparams['lr_step_epochs'], a whole number of epochs >= 1 "
                             "(got %r)" % (se,))
        if not _number(g) or not math.isfinite(g) or g <= 0:
            raise ValueError("hparams['lr_schedule'] = 'step' needs hparams['lr_gamma'], a finite, positive number (got %r)" % (g,))
    elif se is not None or g is not None:
        raise ValueError("hparams['lr_step_epochs'] / ['lr_gamma'] belong to lr_schedule 'step'")
    p = hp.get('early_stop_patience')
    if p is not None and (not _whole(p) or p < 1):
        raise ValueError("hparams['early_stop_patience'] = %r must be null or a whole number of epochs >= 1" % (p,))
    md = _get(hp, 'early_stop_min_delta', 0)
    if not _number(md) or not math.isfinite(md) or md < 0:
        raise ValueError("hparams['early_stop_min_delta'] = %r must be finite and non-negative" % (md,))
    if md != 0 and p is None:
        raise ValueError("hparams['early_stop_min_delta'] has no meaning without hparams['early_stop_patience']")


def scheduled(hp):
    """Does the run read its learning rate from a table?"""
    return hp.get('lr_schedule') is not None or _get(hp, 'lr_warmup_steps', 0) > 0


def table_from_hparams(hp, base_lr, steps_per_epoch, max_epochs):
    """The table of a fit: max_epochs x steps_per_epoch steps (a short last batch is a step like the others) -- or None.  A
    resumed fit rebuilds the same table from the same hyper-parameters; the step counts come back with the optimizer."""
    check_hparams(hp)
    if not scheduled(hp):
        return None
    total = max(1, int(max_epochs) * int(steps_per_epoch))
    kind = hp.get('lr_schedule')
    step_size = int(hp['lr_step_epochs']) * max(1, int(steps_per_epoch)) if kind == 'step' else None
    return lr_table(float(base_lr), total, kind, int(_get(hp, 'lr_warmup_steps', 0)), float(_get(hp, 'lr_min_ratio', 0)), step_size,
                    hp.get('lr_gamma'))


def refuse_multi_rank(hp):
    """A model with a weight average or a learning-rate table under an initialised process group of more than one rank: the
    table's owned slice is stepped by dist.ShardedTableAdam, which has neither."""
    import torch.distributed as dist
    if not (_get(hp, 'ema_decay', 0) or scheduled(hp)):
        return
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError('ema_decay / lr_schedule / lr_warmup_steps are not supported in multi-rank runs: the sharded embedding '
                           'table is stepped by dist.ShardedTableAdam, which keeps no weight average and reads no learning-rate '
                           'table (world size %d)' % dist.get_world_size())


class EarlyStop:
    """Stop when the monitored value has not improved for ``patience`` consecutive epochs.  An epoch improves when its value
    beats the best one so far by MORE than ``min_delta`` (mode 'max': value > best + min_delta; 'min': value < best -
    min_delta); the first value that is a number is the first best.  NaN never improves."""

    def __init__(self, patience, min_delta=0.0, mode='max'):
        if not _whole(patience) or patience < 1:
            raise ValueError('EarlyStop: patience = %r must be a whole number >= 1' % (patience,))
        if not _number(min_delta) or not math.isfinite(min_delta) or min_delta < 0:
            raise ValueError('EarlyStop: min_delta = %r must be finite and non-negative' % (min_delta,))
        if mode not in ('max', 'min'):
            raise ValueError("EarlyStop: mode must be 'max' or 'min'")
        self.patience, self.min_delta, self.mode = int(patience), float(min_delta), mode
        self.best, self.bad = None, 0

    def update(self, value):
        """One epoch's value -> True when training should stop after it."""
        value = float(value)
        if math.isnan(value):
            better = False
        elif self.best is None:
            better = True
        elif self.mode == 'max':
            better = value > self.best + self.min_delta
        else:
            better = value < self.best - self.min_delta
        if better:
            self.best, self.bad = value, 0
        else:
            self.bad += 1
        return self.bad >= self.patience

    def state(self):
        return {'best': self.best, 'bad': int(self.bad)}

    def load(self, state):
        self.best = None if state.get('best') is None else float(state['best'])
        self.bad = int(state.get('bad', 0))
        return self

"""Hyper-parameter search over a config's ``hyperparams_optuna`` space: the study the reference's
``train_config.py`` runs through Optuna (train_config.py:233-279), rebuilt on the standard library, numpy
and torch.

  python -m subgnn_amd.search -config_path CONFIG [-project_root R] [-study_path P] [-n_workers K] [-checkpoint_k k]
  python -m subgnn_amd.train_config -config_path CONFIG -search ...       (the same)

* Space: ``hyperparams_optuna`` entries ``{"type": "suggest_*", "args": [...], "kwargs": {...}}`` merged over
  ``hyperparams_fix`` (train_config.get_hyperparams), types suggest_categorical / _int / _float and the legacy
  suggest_uniform / _loguniform (log scale) / _discrete_uniform.  Bounds are inclusive.
* Samplers (``optuna.sampler``): ``random`` (trial n's parameters are a function of (sampler seed, n, name) only),
  ``grid`` (``optuna.grid_search_space``: every combination once, in an order fixed by the seed), ``tpe`` (univariate
  TPE with Optuna 1.4's defaults; not Optuna's random stream).  The seed is ``optuna.sampler_seed``, else 0.
* Pruner (``optuna.pruning``): MedianPruner() defaults -- 5 start-up trials, no warm-up steps, every step.
* Storage: ``study.sqlite`` in the study directory (its own schema, not Optuna's).  Running a study again continues
  it with ``opt_n_trials`` more trials; trials a killed invocation left RUNNING become FAIL.
* Trials run in ``-n_workers`` fresh child processes on the current device (default ``optuna.opt_n_cores``), each in
  ``trial_<n>/`` (hyperparams.json, final_metric_scores.json, the k best epochs and last.ckpt).  A trial that raises, or a
  worker that dies, ends the study: nothing more is handed out and the command exits non-zero.
* The similarity files of a trial live in ``similarities/search_<key>/``: ``cache_key`` hashes every hyper-parameter a
  cached file can depend on, so trials that share a key share files and no trial reads another's anchors.

DESIGN.md section 8e has the semantics and where they follow Optuna 1.4.
"""
import argparse
import hashlib
import itertools
import json
import math
import os
import signal
import sqlite3
import subprocess
import sys
import time
import traceback
import zlib
from collections import OrderedDict
from pathlib import Path

import numpy as np

STATES = ('RUNNING', 'COMPLETE', 'PRUNED', 'FAIL')
MAX_WORKERS = 8

# Hyper-parameters no file of the similarity cache depends on (SubGNN.get_border_sets / get_similarities read
# neigh_sample_border_size, use_*, sample_walk_len, structure_patch_type, max_sim_epochs, n_anchor_patches_structure,
# n_layers, n_triangular_walks, random_walk_len, rw_beta, structure_anchor_patch_radius, structure_similarity_fn,
# dtw_tie_order and seed -- the draw tape's key).  Everything else below is read by the optimiser, the architecture or
# the per-run anchor draws of _prepare (init_anchors_*), never by a cached file.  Every parameter not listed here is
# part of the key.
CACHE_KEY_EXCLUDED = frozenset([
    'learning_rate', 'grad_clip', 'batch_size', 'max_epochs', 'lin_dropout', 'lstm_dropout', 'trainable_cc',
    'auto_lr_find', 'compute_similarities', 'lstm_aggregator', 'lstm_n_layers', 'ff_attn', 'batch_norm',
    'freeze_node_embeds', 'use_mpn_projection', 'n_processes', 'print_train_times', 'resample_anchor_patches',
    'n_anchor_patches_pos_in', 'n_anchor_patches_pos_out', 'n_anchor_patches_N_in', 'n_anchor_patches_N_out',
    'hip_graph_step', 'deterministic', 'warm_up', 'gc_freeze',
])
CACHE_KEY_EXCLUDED_PREFIXES = ('linear_hidden_dim_',)


def cache_key(hp):
    """12 hex digits of the sha1 of the sorted JSON of every hyper-parameter a similarity file can depend on."""
    kept = {k: v for k, v in hp.items()
            if k not in CACHE_KEY_EXCLUDED and not k.startswith(CACHE_KEY_EXCLUDED_PREFIXES)}
    return hashlib.sha1(json.dumps(kept, sort_keys=True, default=str).encode()).hexdigest()[:12]


# -- search space -----------------------------------------------------------------------------------------------------------
class Param:
    """One searched parameter: kind 'categorical' (choices) or 'int' / 'float' (low, high, step, log)."""

    def __init__(self, name, kind, choices=None, low=None, high=None, step=None, log=False):
        self.name, self.kind, self.choices = name, kind, choices
        self.low, self.high, self.step, self.log = low, high, step, bool(log)
        if kind == 'categorical':
            if not choices:
                raise ValueError('%s: suggest_categorical needs at least one choice' % name)
            return
        if low > high:
            raise ValueError('%s: low %r > high %r' % (name, low, high))
        if self.log and low <= 0:
            raise ValueError('%s: a log scale needs low > 0' % name)
        if self.log and step not in (None, 1):
            raise ValueError('%s: step and log cannot be combined' % name)
        if step is not None and step <= 0:
            raise ValueError('%s: step must be > 0' % name)

    def __repr__(self):
        return 'Param(%r, %r)' % (self.name, self.__dict__)

    def cast(self, v):
        return int(v) if self.kind == 'int' else float(v) if self.kind == 'float' else v

    def snap(self, v):
        """A value of the (transformed-back) continuous range -> the nearest legal value."""
        if self.kind == 'int':
            st = self.step or 1
            k = round((v - self.low) / st)
            k = min(max(k, 0), (self.high - self.low) // st)
            return int(self.low + k * st)
        if self.step is not None:
            k = round((v - self.low) / self.step)
            k = min(max(k, 0), int(math.floor((self.high - self.low) / self.step + 1e-9)))
            return float(min(self.low + k * self.step, self.high))
        return float(min(max(v, self.low), self.high))


def _categorical(name, choices):
    return Param(name, 'categorical', choices=list(choices))


def _int(name, low, high, step=1, log=False):
    return Param(name, 'int', low=int(low), high=int(high), step=int(step), log=log)


def _float(name, low, high, step=None, log=False):
    return Param(name, 'float', low=float(low), high=float(high), step=None if step is None else float(step), log=log)


SUGGEST = {
    'suggest_categorical': _categorical,
    'suggest_int': _int,
    'suggest_float': _float,
    'suggest_uniform': lambda name, low, high: _float(name, low, high),
    'suggest_loguniform': lambda name, low, high: _float(name, low, high, log=True),
    'suggest_discrete_uniform': lambda name, low, high, q: _float(name, low, high, step=q),
}


def parse_space(run_config):
    """``hyperparams_optuna`` -> [Param] in the config's order."""
    space = []
    for name, spec in run_config.get('hyperparams_optuna', {}).items():
        fn = SUGGEST.get(spec.get('type'))
        if fn is None:
            raise ValueError('hyper-parameter %r: unknown type %r (one of %s)' % (name, spec.get('type'), ', '.join(SUGGEST)))
        try:
            space.append(fn(name, *spec.get('args', []), **spec.get('kwargs', {})))
        except TypeError as ex:
            raise ValueError('hyper-parameter %r: bad arguments for %s (%s)' % (name, spec['type'], ex))
    return space


def merged_hyperparams(run_config, params):
    """hyperparams_fix with the searched values over it (train_config.get_hyperparams' order)."""
    hp = OrderedDict(run_config['hyperparams_fix'])
    for name in run_config.get('hyperparams_optuna', {}):
        hp[name] = params[name]
    return hp


def _rng(seed, number, name=''):
    """The generator of (sampler seed, trial number, parameter name): no stream is shared between trials."""
    return np.random.default_rng([int(seed) & 0xFFFFFFFF, int(number), zlib.crc32(name.encode())])


def sample_random(p, rng):
    if p.kind == 'categorical':
        return p.choices[int(rng.integers(len(p.choices)))]
    if p.kind == 'int':
        if p.log:
            x = math.exp(rng.uniform(math.log(p.low - 0.5), math.log(p.high + 0.5)))
            return p.snap(x)
        return int(p.low + int(rng.integers(0, (p.high - p.low) // p.step + 1)) * p.step)
    if p.log:
        return float(min(max(math.exp(rng.uniform(math.log(p.low), math.log(p.high))), p.low), p.high))
    if p.step is not None:
        n = int(math.floor((p.high - p.low) / p.step + 1e-9))
        return p.snap(p.low + int(rng.integers(0, n + 1)) * p.step)
    return float(rng.uniform(p.low, p.high)) if p.high > p.low else float(p.low)


# -- samplers ---------------------------------------------------------------------------------------------------------------
class RandomSampler:
    name = 'random'

    def __init__(self, space, seed=0):
        self.space, self.seed = space, seed

    def sample(self, number, trials, direction):
        """-> (params, grid_id).  ``trials``: the study's trial rows (unused here)."""
        return OrderedDict((p.name, sample_random(p, _rng(self.seed, number, p.name))) for p in self.space), None


class GridSampler:
    name = 'grid'

    def __init__(self, space, grid, seed=0):
        if grid is None:
            raise ValueError('sampler "grid" needs optuna.grid_search_space')
        names = [p.name for p in space]
        missing = [n for n in names if n not in grid]
        if missing:
            raise ValueError('grid_search_space has no values for the searched parameter(s) %s' % ', '.join(missing))
        extra = [n for n in grid if n not in names]
        if extra:
            raise ValueError('grid_search_space names parameter(s) outside hyperparams_optuna: %s' % ', '.join(extra))
        self.space, self.seed, self.names = space, seed, names
        self.grid = list(itertools.product(*[list(grid[n]) for n in names]))
        self.order = [int(i) for i in np.random.default_rng(int(seed) & 0xFFFFFFFF).permutation(len(self.grid))]

    def sample(self, number, trials, direction):
        """The first grid point in the seed's order that no trial holds (a FAIL trial's point is handed out again);
        None when the grid is exhausted."""
        taken = {t['grid_id'] for t in trials if t['state'] != 'FAIL' and t['grid_id'] is not None}
        for gid in self.order:
            if gid not in taken:
                return OrderedDict(zip(self.names, self.grid[gid])), gid
        return None


def default_gamma(n):
    return min(int(math.ceil(0.1 * n)), 25)


def default_weights(n):
    if n == 0:
        return np.asarray([])
    if n < 25:
        return np.ones(n)
    return np.concatenate([np.linspace(1.0 / n, 1.0, num=n - 25), np.ones(25)])


_EPS = 1e-12


def _ndtr(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(x / math.sqrt(2.0)))


def _ndtri(p):
    import torch
    return torch.special.ndtri(torch.as_tensor(np.asarray(p, dtype=np.float64))).numpy()


def parzen_estimator(mus, low, high, weights_func=default_weights, prior_weight=1.0):
    """Optuna 1.4's _ParzenEstimator with consider_prior, consider_magic_clip and not consider_endpoints:
    -> (weights, mus, sigmas) of the mixture, sorted by mu, the prior (mid-range, sigma = range) inserted."""
    mus = np.asarray(mus, dtype=np.float64)
    prior_mu, prior_sigma = 0.5 * (low + high), 1.0 * (high - low)
    order = np.argsort(mus, kind='stable')
    ordered = mus[order]
    pos = int(np.searchsorted(ordered, prior_mu))
    lsh = np.concatenate([[low], ordered[:pos], [prior_mu], ordered[pos:], [high]])
    sorted_mus = lsh[1:-1]
    sigma = np.maximum(lsh[1:-1] - lsh[:-2], lsh[2:] - lsh[1:-1])
    if lsh.size > 3:                                      # (not consider_endpoints)
        sigma[0] = lsh[2] - lsh[1]
        sigma[-1] = lsh[-2] - lsh[-3]
    w = weights_func(mus.size)
    sw = np.concatenate([w[order[:pos]], [prior_weight], w[order[pos:]]])
    sw = sw / sw.sum()
    maxsigma = 1.0 * (high - low)
    minsigma = 1.0 * (high - low) / min(100.0, 1.0 + sorted_mus.size)
    sigma = np.clip(sigma, minsigma, maxsigma)
    sigma[pos] = prior_sigma
    return sw, sorted_mus.copy(), sigma


def _gmm_sample(rng, est, low, high, q, size):
    w, mu, sg = est
    active = rng.choice(len(w), size=size, p=w)
    a, b = _ndtr((low - mu[active]) / sg[active]), _ndtr((high - mu[active]) / sg[active])
    u = a + rng.uniform(size=size) * (b - a)
    x = mu[active] + sg[active] * _ndtri(np.clip(u, 1e-16, 1 - 1e-16))
    x = np.clip(x, low, high)
    if q is not None:
        x = np.round(x / q) * q
    return x


def _gmm_log_pdf(x, est, low, high, q):
    w, mu, sg = est
    p_accept = float(np.sum(w * (_ndtr((high - mu) / sg) - _ndtr((low - mu) / sg))))
    if q is None:
        d = (x[:, None] - mu[None, :]) / np.maximum(sg, _EPS)
        coef = w / (math.sqrt(2 * math.pi) * sg) / p_accept
        m = -0.5 * d * d
        top = m.max(axis=1, keepdims=True)
        return (top[:, 0] + np.log(np.sum(coef * np.exp(m - top), axis=1) + _EPS))
    up = np.minimum(x + 0.5 * q, high)[:, None]
    lo = np.maximum(x - 0.5 * q, low)[:, None]
    prob = np.sum(w * (_ndtr((up - mu) / sg) - _ndtr((lo - mu) / sg)), axis=1) / p_accept
    return np.log(prob + _EPS)


class TPESampler:
    """Univariate TPE, Optuna 1.4's defaults (n_startup_trials 10, gamma min(ceil(0.1 n), 25), 24 EI candidates from l(x),
    prior weight 1, magic clipping).  Observations: COMPLETE trials by value, PRUNED ones by (last step, its value) --
    later steps rank better, as in Optuna.  The random numbers are this module's, not Optuna's."""
    name = 'tpe'
    n_startup_trials, n_ei_candidates = 10, 24

    def __init__(self, space, seed=0):
        self.space, self.seed = space, seed

    @staticmethod
    def observations(trials, direction):
        sign = -1.0 if direction == 'maximize' else 1.0
        obs = []
        for t in sorted(trials, key=lambda t: t['number']):
            if t['state'] == 'COMPLETE' and t['value'] is not None:
                obs.append((t, (-math.inf, sign * t['value'])))
            elif t['state'] == 'PRUNED':
                iv = t['intermediate']
                if iv:
                    s = max(iv, key=int)
                    obs.append((t, (-int(s), sign * iv[s])))
                else:
                    obs.append((t, (math.inf, 0.0)))
        return obs

    def sample(self, number, trials, direction):
        obs = self.observations(trials, direction)
        if len(obs) < self.n_startup_trials:
            return RandomSampler(self.space, self.seed).sample(number, trials, direction)
        n_below = default_gamma(len(obs))
        rank = sorted(range(len(obs)), key=lambda i: obs[i][1])
        below_idx = set(rank[:n_below])
        out = OrderedDict()
        for p in self.space:
            rng = _rng(self.seed, number, p.name)
            below = [o[0]['params'][p.name] for i, o in enumerate(obs) if i in below_idx and p.name in o[0]['params']]
            above = [o[0]['params'][p.name] for i, o in enumerate(obs) if i not in below_idx and p.name in o[0]['params']]
            out[p.name] = self._sample_param(p, below, above, rng)
        return out, None

    def _sample_param(self, p, below, above, rng):
        if p.kind == 'categorical':
            k = len(p.choices)
            idx = lambda vs: np.asarray([p.choices.index(v) for v in vs if v in p.choices], dtype=np.int64)
            ib, ia = idx(below), idx(above)
            pb = np.bincount(ib, weights=default_weights(ib.size), minlength=k) + 1.0
            pa = np.bincount(ia, weights=default_weights(ia.size), minlength=k) + 1.0
            pb, pa = pb / pb.sum(), pa / pa.sum()
            cand = rng.choice(k, size=self.n_ei_candidates, p=pb)
            score = np.log(pb[cand]) - np.log(pa[cand])
            return p.choices[int(cand[int(np.argmax(score))])]
        # the transformed space: log scale -> log(x); a step -> a grid of q with the range widened by q/2 at both ends
        q = None
        if p.kind == 'int' and p.log:
            low, high = math.log(p.low - 0.5), math.log(p.high + 0.5)
            tf = np.log
        elif p.log:
            low, high = math.log(p.low), math.log(p.high)
            tf = np.log
        else:
            q = p.step if p.kind == 'float' else (p.step or 1)
            low, high = (p.low - 0.5 * q, p.high + 0.5 * q) if q is not None else (p.low, p.high)
            tf = lambda v: v
        if high <= low:
            return p.cast(p.low)
        xb, xa = tf(np.asarray(below, dtype=np.float64)), tf(np.asarray(above, dtype=np.float64))
        shift = p.low if q is not None else 0.0            # (the step grid is anchored at low)
        est_b = parzen_estimator(xb - shift, low - shift, high - shift)
        est_a = parzen_estimator(xa - shift, low - shift, high - shift)
        cand = _gmm_sample(rng, est_b, low - shift, high - shift, q, self.n_ei_candidates)
        score = _gmm_log_pdf(cand, est_b, low - shift, high - shift, q) - _gmm_log_pdf(cand, est_a, low - shift, high - shift, q)
        best = float(cand[int(np.argmax(score))]) + shift
        return p.snap(math.exp(best) if p.log else best)


def make_sampler(run_config, space):
    opt = run_config.get('optuna', {})
    kind, seed = opt.get('sampler', 'random'), int(opt.get('sampler_seed', 0))
    if kind == 'random':
        return RandomSampler(space, seed)
    if kind == 'grid':
        return GridSampler(space, opt.get('grid_search_space'), seed)
    if kind == 'tpe':
        return TPESampler(space, seed)
    raise ValueError('unknown optuna.sampler %r (random, grid or tpe)' % (kind,))


# -- pruner -----------------------------------------------------------------------------------------------------------------
def median_should_prune(direction, reported, step, completed, n_startup_trials=5, n_warmup_steps=0, interval_steps=1):
    """MedianPruner(): ``reported`` {step: value} of this trial up to ``step``; ``completed``: the {step: value} of every
    COMPLETE trial.  Pruned when at least ``n_startup_trials`` trials are complete and this trial's best value so far is
    worse than the nan-median of the completed trials' values at ``step`` (a step none of them reached prunes nothing)."""
    if len(completed) < n_startup_trials or step < n_warmup_steps:
        return False
    if (step - n_warmup_steps) % interval_steps != 0:
        return False
    vals = np.asarray([v for s, v in reported.items() if int(s) <= step], dtype=np.float64)
    if vals.size == 0:
        return False
    if np.all(np.isnan(vals)):
        return True
    best = np.nanmax(vals) if direction == 'maximize' else np.nanmin(vals)
    at = np.asarray([c[s] for c in completed for s in c if int(s) == step], dtype=np.float64)
    if at.size == 0 or np.all(np.isnan(at)):
        return False
    med = float(np.nanmedian(at))
    return bool(best < med) if direction == 'maximize' else bool(best > med)


# -- storage ----------------------------------------------------------------------------------------------------------------
STUDY_FILE = 'study.sqlite'
_SCHEMA = '''
CREATE TABLE IF NOT EXISTS study (id INTEGER PRIMARY KEY CHECK (id = 1), direction TEXT, monitor TEXT, sampler TEXT,
                                  created REAL);
CREATE TABLE IF NOT EXISTS invocations (id INTEGER PRIMARY KEY, n_trials INTEGER, stopped INTEGER DEFAULT 0, started REAL);
CREATE TABLE IF NOT EXISTS trials (number INTEGER PRIMARY KEY, state TEXT NOT NULL, params TEXT NOT NULL, grid_id INTEGER,
                                   value REAL, intermediate TEXT NOT NULL DEFAULT '{}', dir TEXT, wall_s REAL,
                                   device_bytes INTEGER, device_peak_bytes INTEGER, invocation INTEGER, worker INTEGER,
                                   error TEXT);
'''


class Storage:
    """study.sqlite: one connection per process; every hand-out is one IMMEDIATE transaction."""

    def __init__(self, path):
        self.path = Path(path)
        self.conn = sqlite3.connect(str(self.path), timeout=300, isolation_level=None)
        self.conn.execute('PRAGMA busy_timeout = 300000')
        self.conn.executescript(_SCHEMA)

    def close(self):
        self.conn.close()

    def _tx(self):
        self.conn.execute('BEGIN IMMEDIATE')

    def check_study(self, direction, monitor, sampler):
        """Record the study's settings, or raise ValueError when the stored ones differ."""
        self._tx()
        try:
            row = self.conn.execute('SELECT direction, monitor, sampler FROM study WHERE id = 1').fetchone()
            if row is None:
                self.conn.execute('INSERT INTO study VALUES (1, ?, ?, ?, ?)', (direction, monitor, sampler, time.time()))
            elif tuple(row) != (direction, monitor, sampler):
                raise ValueError('the stored study %s has direction / monitor / sampler %s, the config %s' % (
                    self.path, tuple(row), (direction, monitor, sampler)))
            self.conn.execute('COMMIT')
        except BaseException:
            self.conn.execute('ROLLBACK')
            raise

    def begin_invocation(self, n_trials):
        """Trials left RUNNING by an earlier (killed) invocation become FAIL -> this invocation's id."""
        self._tx()
        self.conn.execute("UPDATE trials SET state = 'FAIL', error = 'left RUNNING by an earlier invocation' "
                          "WHERE state = 'RUNNING'")
        cur = self.conn.execute('INSERT INTO invocations (n_trials, started) VALUES (?, ?)', (int(n_trials), time.time()))
        self.conn.execute('COMMIT')
        return cur.lastrowid

    def stop(self, invocation):
        self.conn.execute('UPDATE invocations SET stopped = 1 WHERE id = ?', (invocation,))

    def fail_running(self, invocation, error):
        self.conn.execute("UPDATE trials SET state = 'FAIL', error = ? WHERE state = 'RUNNING' AND invocation = ?",
                          (error, invocation))

    def trials(self):
        rows = self.conn.execute('SELECT number, state, params, grid_id, value, intermediate, dir, wall_s, device_bytes, '
                                 'device_peak_bytes, invocation, worker, error FROM trials ORDER BY number').fetchall()
        keys = ('number', 'state', 'params', 'grid_id', 'value', 'intermediate', 'dir', 'wall_s', 'device_bytes',
                'device_peak_bytes', 'invocation', 'worker', 'error')
        out = []
        for r in rows:
            t = dict(zip(keys, r))
            t['params'] = json.loads(t['params'], object_pairs_hook=OrderedDict)
            t['intermediate'] = json.loads(t['intermediate'])
            out.append(t)
        return out

    def claim(self, invocation, sampler, direction, study_dir, worker=0):
        """-> (number, params) of a new RUNNING trial, or None: the invocation is stopped, its opt_n_trials are handed
        out, or the grid is exhausted."""
        self._tx()
        try:
            inv = self.conn.execute('SELECT n_trials, stopped FROM invocations WHERE id = ?', (invocation,)).fetchone()
            done = self.conn.execute('SELECT COUNT(*) FROM trials WHERE invocation = ?', (invocation,)).fetchone()[0]
            got = None
            if inv is not None and not inv[1] and done < inv[0]:
                trials = self.trials()
                number = trials[-1]['number'] + 1 if trials else 0
                s = sampler.sample(number, trials, direction)
                if s is not None:
                    params, gid = s
                    d = str(Path(study_dir) / ('trial_%d' % number))
                    self.conn.execute('INSERT INTO trials (number, state, params, grid_id, dir, invocation, worker) '
                                      "VALUES (?, 'RUNNING', ?, ?, ?, ?, ?)",
                                      (number, json.dumps(params), gid, d, invocation, worker))
                    got = number, params
            self.conn.execute('COMMIT')
            return got
        except BaseException:
            self.conn.execute('ROLLBACK')
            raise

    def report(self, number, step, value):
        self._tx()
        iv = json.loads(self.conn.execute('SELECT intermediate FROM trials WHERE number = ?', (number,)).fetchone()[0])
        iv[str(int(step))] = float(value)
        self.conn.execute('UPDATE trials SET intermediate = ? WHERE number = ?', (json.dumps(iv), number))
        self.conn.execute('COMMIT')
        return iv

    def completed_intermediates(self):
        return [json.loads(r[0]) for r in
                self.conn.execute("SELECT intermediate FROM trials WHERE state = 'COMPLETE'").fetchall()]

    def finish(self, number, state, value=None, wall_s=None, device_bytes=None, device_peak_bytes=None, error=None):
        assert state in STATES
        self.conn.execute('UPDATE trials SET state = ?, value = ?, wall_s = ?, device_bytes = ?, device_peak_bytes = ?, '
                          'error = ? WHERE number = ?',
                          (state, value, wall_s, device_bytes, device_peak_bytes, error, number))


# -- the study --------------------------------------------------------------------------------------------------------------
def study_settings(run_config):
    opt = run_config.get('optuna', {})
    direction = opt.get('opt_direction', 'maximize')
    if direction not in ('maximize', 'minimize'):
        raise ValueError('optuna.opt_direction must be maximize or minimize, not %r' % (direction,))
    return direction, opt.get('monitor_metric', 'val_micro_f1'), opt.get('sampler', 'random')


def default_study_dir(run_config, project_root):
    """tb.dir/tb.name under the project root, or as given with tb.local (the reference's train_config.py:234-248)."""
    tb = run_config.get('tb', {})
    base = Path(tb.get('dir', 'tensorboard'))
    if not tb.get('local', False):
        base = Path(project_root) / base
    return base / tb.get('name', 'study')


def best_trial(trials, direction):
    """The best COMPLETE trial (ties: the lowest number), or None."""
    done = [t for t in trials if t['state'] == 'COMPLETE' and t['value'] is not None and not math.isnan(t['value'])]
    if not done:
        return None
    sign = -1.0 if direction == 'maximize' else 1.0
    return min(done, key=lambda t: (sign * t['value'], t['number']))


def write_results(storage, study_dir, run_config):
    direction, monitor, sampler = study_settings(run_config)
    trials = storage.trials()
    b = best_trial(trials, direction)
    res = {'direction': direction, 'monitor': monitor, 'sampler': sampler,
           'trials': [{'number': t['number'], 'state': t['state'], 'value': t['value'], 'params': t['params'],
                       'dir': t['dir']} for t in trials],
           'best_trial': None if b is None else {'number': b['number'], 'value': b['value'], 'params': b['params'],
                                                 'dir': b['dir']}}
    with open(Path(study_dir) / 'study_results.json', 'w') as f:
        json.dump(res, f, indent=2)
    return res


class StudyFailed(RuntimeError):
    pass


def run_study(run_config, study_dir, n_workers=None, checkpoint_k=3, project_root=None, trial_fn=None, log=print,
              poll_s=0.2, auto_lr_find=False):
    """Run ``opt_n_trials`` more trials of the study in ``study_dir`` with ``n_workers`` worker processes.
    ``trial_fn``: 'module:function' run in the workers instead of the training trial (host tests).
    ``auto_lr_find``: the trials honour their ``auto_lr_find`` hyper-parameter (train_config.train_model's).
    -> the study_results dict; raises StudyFailed when a trial failed or a worker died."""
    from . import config
    opt = run_config.get('optuna', {})
    n_workers = int(opt.get('opt_n_cores', 1) if n_workers is None else n_workers)
    if not 1 <= n_workers <= MAX_WORKERS:
        raise ValueError('n_workers must be in 1..%d (each worker opens the GPU), not %d' % (MAX_WORKERS, n_workers))
    direction, monitor, sampler_name = study_settings(run_config)
    space = parse_space(run_config)
    make_sampler(run_config, space)                       # (raises on a bad sampler / grid before anything starts)
    study_dir = Path(study_dir).resolve()
    study_dir.mkdir(parents=True, exist_ok=True)
    storage = Storage(study_dir / STUDY_FILE)
    storage.check_study(direction, monitor, sampler_name)
    inv = storage.begin_invocation(int(opt.get('opt_n_trials', 1)))
    args = {'run_config': run_config, 'study_dir': str(study_dir), 'invocation': inv, 'n_workers': n_workers,
            'checkpoint_k': int(checkpoint_k), 'trial_fn': trial_fn, 'auto_lr_find': bool(auto_lr_find),
            'project_root': str(Path(project_root if project_root is not None else config.PROJECT_ROOT).resolve()),
            'sys_path': [p for p in sys.path if p]}
    prelude = ('import json, sys; a = json.loads(sys.argv[1]); sys.path[:0] = a["sys_path"]; '
               'from subgnn_amd.search import worker_main; sys.exit(worker_main(a))')
    procs, logs = [], []
    failure = None
    try:
        for w in range(n_workers):
            lp = study_dir / ('worker_%d.log' % w)
            fh = open(lp, 'a')
            logs.append((lp, fh))
            procs.append(subprocess.Popen([sys.executable, '-c', prelude, json.dumps(dict(args, worker=w))],
                                          stdout=fh, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL))
        log('study %s: %d worker(s), %d trial(s) this invocation' % (study_dir, n_workers, int(opt.get('opt_n_trials', 1))))
        live = set(range(n_workers))
        while live and failure is None:
            time.sleep(poll_s)
            for w in sorted(live):
                rc = procs[w].poll()
                if rc is None:
                    continue
                live.discard(w)
                if rc != 0:
                    how = 'killed by signal %d' % -rc if rc < 0 else 'exited with status %d' % rc
                    failure = 'worker %d %s; its log: %s' % (w, how, logs[w][0])
                    break
    except BaseException:
        failure = failure or 'interrupted'
        raise
    finally:
        if failure is not None:
            storage.stop(inv)                             # (nothing more is handed out)
            for p in procs:
                if p.poll() is None:
                    p.send_signal(signal.SIGTERM)
            for p in procs:
                try:
                    p.wait(timeout=60)
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            storage.fail_running(inv, failure)
        for _, fh in logs:
            fh.close()
        res = write_results(storage, study_dir, run_config)
        storage.close()
    if failure is not None:
        raise StudyFailed(failure)
    return res


# -- the worker -------------------------------------------------------------------------------------------------------------
class TrialContext:
    """What a trial function gets: its number, parameters, merged hyper-parameters and directory, and ``report``."""

    def __init__(self, storage, number, params, run_config, study_dir, checkpoint_k, pruning, direction, log,
                 auto_lr_find=False):
        self.storage, self.number, self.params, self.auto_lr_find = storage, number, params, bool(auto_lr_find)
        self.run_config, self.checkpoint_k, self.pruning, self.direction, self.log = \
            run_config, checkpoint_k, pruning, direction, log
        self.hp = merged_hyperparams(run_config, params)
        self.dir = Path(study_dir) / ('trial_%d' % number)
        self.pruned_at = None

    def report(self, step, value):
        """Trainer.fit's epoch callback: records the value; True (stop after this epoch) when the median pruner says so."""
        iv = self.storage.report(self.number, step, value)
        if self.pruning and median_should_prune(self.direction, iv, int(step), self.storage.completed_intermediates()):
            self.pruned_at = int(step)
            return True
        return False


def train_trial(ctx):
    """The trial: train_config.train_model with the sampled values, the pruning callback and the trial's similarity
    directory -> the best monitored value."""
    from .train_config import FixedTrial, train_model
    best, model, trainer = train_model(ctx.run_config, trial=FixedTrial(ctx.params), results_dir=ctx.dir, log=ctx.log,
                                       checkpoint_k=ctx.checkpoint_k, epoch_callback=ctx.report,
                                       similarities_subdir='search_' + cache_key(ctx.hp), auto_lr_find=ctx.auto_lr_find)
    del model, trainer
    return best


def _load_fn(spec):
    if spec is None:
        return train_trial
    import importlib
    mod, fn = spec.split(':')
    return getattr(importlib.import_module(mod), fn)


def worker_main(a):
    """One worker process: claim a trial, run it, record it, repeat; exits 0 when nothing is left, 1 after a failed trial."""
    import gc
    import torch
    from . import config
    config.PROJECT_ROOT = Path(a['project_root'])
    budget = int(os.environ.get('OMP_NUM_THREADS') or torch.get_num_threads())
    torch.set_num_threads(max(1, budget // int(a['n_workers'])))
    run_config, study_dir = a['run_config'], Path(a['study_dir'])
    direction, _, _ = study_settings(run_config)
    sampler = make_sampler(run_config, parse_space(run_config))
    pruning = bool(run_config.get('optuna', {}).get('pruning', False))
    fn = _load_fn(a.get('trial_fn'))
    storage = Storage(study_dir / STUDY_FILE)
    log = lambda *m: print(*m, flush=True)
    while True:
        got = storage.claim(a['invocation'], sampler, direction, study_dir, a['worker'])
        if got is None:
            return 0
        number, params = got
        log('trial %d: %s' % (number, json.dumps(params)))
        ctx = TrialContext(storage, number, params, run_config, study_dir, a['checkpoint_k'], pruning, direction, log,
                           auto_lr_find=a.get('auto_lr_find', False))
        cuda = torch.cuda.is_available() and torch.cuda.is_initialized()
        if cuda:
            torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        try:
            value = fn(ctx)
        except BaseException:
            traceback.print_exc()
            sys.stdout.flush()
            storage.finish(number, 'FAIL', wall_s=time.perf_counter() - t0, error=traceback.format_exc(limit=3))
            storage.stop(a['invocation'])
            return 1
        wall = time.perf_counter() - t0
        # nothing of the trial is referenced any more: Trainer.fit froze the collector's view (gc.freeze), so collect here
        gc.unfreeze()
        gc.collect()
        cuda = torch.cuda.is_available() and torch.cuda.is_initialized()
        held = peak = None
        if cuda:
            torch.cuda.synchronize()
            held, peak = int(torch.cuda.memory_allocated()), int(torch.cuda.max_memory_allocated())
        state = 'PRUNED' if ctx.pruned_at is not None else 'COMPLETE'
        storage.finish(number, state, value=None if value is None else float(value), wall_s=wall, device_bytes=held,
                       device_peak_bytes=peak)
        log('trial %d: %s %s (%.1f s)' % (number, state, value, wall))
        del ctx, value


# -- CLI --------------------------------------------------------------------------------------------------------------------
def add_search_args(ap):
    ap.add_argument('-study_path', type=str, default=None, help='study directory (default: tb.dir/tb.name)')
    ap.add_argument('-n_workers', type=int, default=None, help='concurrent trial processes (default: optuna.opt_n_cores)')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Hyper-parameter search over a reference-format config.json')
    ap.add_argument('-config_path', type=str, required=True)
    ap.add_argument('-project_root', type=str, default=None, help='overrides subgnn_amd.config.PROJECT_ROOT')
    ap.add_argument('-checkpoint_k', type=int, default=3, help='epochs kept per trial by the monitored metric')
    ap.add_argument('-auto_lr_find', action='store_true', help="the trials honour their auto_lr_find hyper-parameter")
    add_search_args(ap)
    ap.add_argument('-trial_fn', type=str, default=None, help=argparse.SUPPRESS)    # module:function instead of training (tests)
    return ap.parse_args(argv)


def main_from_args(args):
    from . import config
    from .train_config import read_json
    if args.project_root:
        config.PROJECT_ROOT = Path(args.project_root)
    run_config = read_json(args.config_path)
    study_dir = Path(args.study_path) if args.study_path else default_study_dir(run_config, config.PROJECT_ROOT)
    k = 3 if args.checkpoint_k is None else args.checkpoint_k
    try:
        res = run_study(run_config, study_dir, n_workers=args.n_workers, checkpoint_k=k,
                        trial_fn=getattr(args, 'trial_fn', None), auto_lr_find=getattr(args, 'auto_lr_find', False))
    except StudyFailed as ex:
        print('study failed: %s' % ex, file=sys.stderr)
        return 1
    b = res['best_trial']
    if b is not None:
        print('best trial %d: %s %.4f  %s' % (b['number'], res['monitor'], b['value'], b['dir']))
    return 0


def main(argv=None):
    return main_from_args(parse_args(argv))


if __name__ == '__main__':
    sys.exit(main())

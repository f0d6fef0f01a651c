"""Learning-rate range test: ``Trainer.lr_find`` and ``Trainer(auto_lr_find=...)``, the reference's ``auto_lr_find``
hyper-parameter (train_config.py:128-130, train.py:297-298: PyTorch Lightning's learning-rate finder, config_files/README.md).

This RESTATES Lightning 0.7.x ``trainer/lr_finder.py`` (``_LRFinder``, ``_LRCallback``, ``_ExponentialLR``, ``_LinearLR``) from
its published source as recalled -- Lightning is not a dependency of this project, so nothing here is checked against it, in
the way ``oracle/fastdtw_restate.py`` restates fastdtw.  The tests pin this restatement:

  schedule   step k of num_training: exponential  lr_k = min_lr * (max_lr / min_lr) ** (k / num_training)
                                     linear       lr_k = min_lr + (k / num_training) * (max_lr - min_lr)
             (double, stored as float32: the rates the steps actually use)
  steps      a fresh optimizer (configure_optimizers through optim.accelerate, with the trainer's gradient clip), the trainer's
             own training step (recorded full batches, eager otherwise), batches of successive train_dataloader epochs, at most
             num_training steps and max_epochs epochs
  smoothing  avg = 0.98 avg + 0.02 L_k (from 0), smoothed = avg / (1 - 0.98 ** (k + 1)); after step k stop when k + 1 > 1 and
             smoothed > early_stop_threshold * best; best = smoothed when smaller or k == 0; the stopping entry is kept
  suggestion lr at argmin(np.gradient(loss[skip_begin:-skip_end])) + skip_begin; None with fewer than 2 points there

The rate of every step lives in a float32 table on the device that ClipAdam reads (``lr_schedule``,
sgnn_optim_adam_lr_table), so ONE recording replays the whole range test; each step's loss is read back (one small copy per
replay) so that no step runs past the stop.  Afterwards the model is as it was: parameters and buffers (checkpoint.Snapshot),
the head's dropout state, the anchor draw and the torch / numpy / python generators -- a fit after the finder is bit for bit a
fit at the suggested rate set by hand (Lightning leaves the finder's draws consumed; DESIGN.md section 8f lists the
differences)."""
import numpy as np
import torch

from . import checkpoint, ops
from .graph_step import CapturedTrainStep, StepNotRecordable, make_eager
from .optim import accelerate

BETA = 0.98
_ABSENT = object()


def schedule(min_lr, max_lr, num_training, mode='exponential'):
    """The rate of steps 0 .. num_training-1 -> float32 numpy array (``_ExponentialLR`` / ``_LinearLR`` with base_lr = min_lr)."""
    if mode not in ('exponential', 'linear'):
        raise ValueError("mode must be 'exponential' or 'linear', got %r" % (mode,))
    n = int(num_training)
    if n < 1:
        raise ValueError('num_training must be at least 1')
    lo, hi = float(min_lr), float(max_lr)
    if mode == 'exponential':
        vals = [lo * (hi / lo) ** (k / n) for k in range(n)]
    else:
        vals = [lo + (k / n) * (hi - lo) for k in range(n)]
    return np.asarray(vals, dtype=np.float64).astype(np.float32)


class Smoother:
    """``_LRCallback.on_batch_end``: ``add(loss)`` -> (smoothed loss, stop after this step)."""

    def __init__(self, early_stop_threshold=4.0, beta=BETA):
        self.threshold, self.beta = early_stop_threshold, beta
        self.avg, self.best, self.k = 0.0, 0.0, 0

    def add(self, loss):
        self.avg = self.beta * self.avg + (1 - self.beta) * float(loss)
        smoothed = self.avg / (1 - self.beta ** (self.k + 1))
        stop = self.threshold is not None and self.k + 1 > 1 and smoothed > self.threshold * self.best
        if smoothed < self.best or self.k == 0:
            self.best = smoothed
        self.k += 1
        return smoothed, stop


class LRFinder:
    """What ``lr_find`` returns: ``results = {'lr': [...], 'loss': [...]}`` (rate and smoothed loss per step run),
    ``suggestion()``, and the run's ``mode``, ``min_lr``, ``max_lr``, ``num_training``, ``steps``, ``stopped_early``."""

    def __init__(self, mode, min_lr, max_lr, num_training):
        self.mode, self.min_lr, self.max_lr, self.num_training = mode, float(min_lr), float(max_lr), int(num_training)
        self.results = {'lr': [], 'loss': []}
        self.stopped_early = False
        self._optimal_idx = None

    @property
    def steps(self):
        return len(self.results['loss'])

    def suggestion(self, skip_begin=10, skip_end=1):
        """The rate at the steepest descent of the smoothed loss: ``np.gradient`` over ``loss[skip_begin:-skip_end]``, its
        argmin (non-finite losses are not filtered out: the first NaN wins, as in 0.7.x); None on any failure, fewer than 2
        points among them included."""
        try:
            loss = np.asarray(self.results['loss'][skip_begin:-skip_end], dtype=np.float64)
            if loss.size < 2:
                raise ValueError('%d points after skipping %d and %d' % (loss.size, skip_begin, skip_end))
            self._optimal_idx = int(np.argmin(np.gradient(loss))) + skip_begin
            return self.results['lr'][self._optimal_idx]
        except Exception:
            self._optimal_idx = None
            return None

    def summary(self, configured_lr=None):
        """The dict a run directory's ``lr_find.json`` holds."""
        return {'mode': self.mode, 'min_lr': self.min_lr, 'max_lr': self.max_lr, 'num_training': self.num_training,
                'configured_lr': configured_lr, 'suggestion': self.suggestion(), 'steps': self.steps,
                'stopped_early': self.stopped_early, 'lr': list(self.results['lr']), 'loss': list(self.results['loss'])}


def lr_key(hparams, auto_lr_find=True):
    """Which hyper-parameter the suggestion replaces (Lightning 0.7.x ``_run_lr_finder_internally``): the named one for a
    ``str``, else ``lr`` when present, else ``learning_rate``; ValueError when it is missing."""
    if isinstance(auto_lr_find, str):
        if auto_lr_find not in hparams:
            raise ValueError('auto_lr_find is %r, but the model has no such hyper-parameter' % (auto_lr_find,))
        return auto_lr_find
    for k in ('lr', 'learning_rate'):
        if k in hparams:
            return k
    raise ValueError("auto_lr_find needs a hyper-parameter 'lr' or 'learning_rate' to set")


def run(trainer, model, min_lr=1e-8, max_lr=1.0, num_training=100, mode='exponential', early_stop_threshold=4.0):
    """``Trainer.lr_find``: the range test on ``model`` (prepared here if it is not) -> LRFinder.  The model, its generators
    and the device memory in use are as they were before; the trainer is unchanged."""
    rates = schedule(min_lr, max_lr, num_training, mode)
    finder = LRFinder(mode, min_lr, max_lr, num_training)
    if not checkpoint._prepared(model):
        model.prepare_data()
    dev = model.node_embeddings.weight.device
    # -- what the steps change, kept -----------------------------------------------------------------------------------------
    gens = checkpoint.generator_states(dev)
    kept = {k: model.__dict__.get(k, _ABSENT) for k in ('_head_rng', '_head_result', '_head_labels', '_resample_epoch')}
    live = list(model.state_dict().values())
    head = kept['_head_rng']
    if head is not _ABSENT and head is not None:
        live.append(head)
    snap = checkpoint.Snapshot()
    snap.capture(live, {})
    was_training = model.training
    opt = captured = None
    try:
        table = torch.from_numpy(rates).to(dev)
        recorded = trainer.hip_graph_step
        opt = accelerate(model.configure_optimizers(), trainer.clip, capturable=recorded, lr_schedule=table)
        smooth = Smoother(early_stop_threshold)
        model.train()
        for _ in range(trainer.max_epochs):
            if finder.steps >= finder.num_training or finder.stopped_early:
                break
            loader = model.train_dataloader()
            if recorded:
                if captured is None:
                    captured = CapturedTrainStep(model, opt, loader.bs, trainer.clip, warmup=3)
                batches = ((bi, idx, None) for bi, idx in enumerate(loader.index_batches()))
            else:
                batches = ((bi, None, b) for bi, b in enumerate(loader))
            for bi, idx, batch in batches:
                loss = None
                if recorded and idx.numel() == loader.bs:
                    try:
                        loss = captured.replay(idx)[0]
                    except StepNotRecordable as ex:      # (as in fit: the steps that follow are the eager ones)
                        trainer.log('lr_find: the training step could not be recorded (%s); stepping eagerly' % (ex,))
                        recorded, captured = False, None
                        make_eager(opt)
                        torch.cuda.synchronize()
                if loss is None:
                    loss = trainer._eager_step(model, opt, batch if batch is not None else model.make_batch('train', idx), bi)
                k = finder.steps
                smoothed, stop = smooth.add(loss.item())          # (the one read-back of the step)
                finder.results['lr'].append(float(rates[k]))
                finder.results['loss'].append(smoothed)
                if stop:
                    finder.stopped_early = True
                if stop or finder.steps >= finder.num_training:
                    break
    finally:
        # -- everything back: the finder's recording, optimizer and gradients go; the kept state returns --------------------
        captured = None
        if opt is not None and hasattr(opt, 'release'):
            opt.release()
        opt = None
        for p in model.parameters():
            ops.drop_zeroed(p)
            p.grad = None
        snap.restore(live)
        snap = None
        for k, v in kept.items():
            if v is _ABSENT:
                model.__dict__.pop(k, None)
            else:
                model.__dict__[k] = v
        checkpoint.set_generator_states(gens, dev)
        model.invalidate_half_table()
        model.train(was_training)
    return finder

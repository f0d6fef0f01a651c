"""Build-owned counterpart of the reference driver SubGNN/train_config.py.

The reference driver cannot travel (it imports optuna, commentjson and pytorch-lightning 0.7.1 at
module level, train_config.py:8,21-29); this file replays the same call sequence against the same
``config.json`` schema (SubGNN/config_files/README.md:5-116) with nothing but the standard library
and torch, so the drop-in module can be exercised end to end on the GPU box:

  read json (// comments allowed)                                  train_config.py:44-52
  -> dataset paths from data.task + hyperparams_fix.embedding_type  :213-232
  -> fixed + "suggested" hyper-parameters merged into one dict      :60-86
  -> seed torch / numpy                                             :96-101
  -> SubGNN(hparams, 7 paths)                                       :104-106
  -> hyperparams.json                                               :174-183
  -> fit: prepare_data, configure_optimizers, per batch training_step -> model.backward ->
     clip grad-norm to grad_clip -> optimizer.step/zero_grad; per epoch validation_step* ->
     validation_epoch_end; keep the best monitored metric           (PL 0.7.x hook order)
  -> final_metric_scores.json from model.metric_scores[-1]          :189-193
  -> return the monitored metric                                    :196-200

A single run answers every ``suggest_*`` call with a ``FixedTrial``: the first categorical choice / the lower bound (or
a value supplied by the caller).  ``-search`` runs the study instead (``subgnn_amd.search``: samplers, median pruning,
concurrent trial processes).
"""
import argparse
import json
import random
import re
from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch

from . import checkpoint, config, schedule
from . import lr_find as range_test
from .SubGNN import SubGNN, dataset_paths
from .graph_step import CapturedEvalStep, CapturedTrainStep, StepNotRecordable, make_capturable, make_eager, train_step
from .optim import accelerate


def read_json(fname):
    """commentjson.load(..., object_hook=OrderedDict): strips // and /* */ comments."""
    txt = Path(fname).read_text()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'(^|[\s,{\[])//[^\n]*', r'\1', txt)
    txt = re.sub(r',(\s*[}\]])', r'\1', txt)
    return json.loads(txt, object_pairs_hook=OrderedDict)


class FixedTrial:
    """Deterministic stand-in for optuna.Trial: first categorical choice, lower bound of ranges."""

    def __init__(self, values=None):
        self.values, self.params = dict(values or {}), {}

    def _pick(self, name, default):
        v = self.values.get(name, default)
        self.params[name] = v
        return v

    def suggest_categorical(self, name, choices):
        return self._pick(name, choices[0])

    def suggest_float(self, name, low, high, *a, **kw):         # (*a: suggest_discrete_uniform's q, a positional step)
        return self._pick(name, float(low))

    def suggest_int(self, name, low, high, *a, **kw):
        return self._pick(name, int(low))

    suggest_uniform = suggest_loguniform = suggest_discrete_uniform = suggest_float

    def report(self, *a, **k):
        pass

    def should_prune(self):
        return False


def get_hyperparams(run_config, trial):
    hp = dict(run_config['hyperparams_fix'])
    for name, spec in run_config.get('hyperparams_optuna', {}).items():
        hp[name] = getattr(trial, spec['type'])(name, *spec.get('args', []), **spec.get('kwargs', {}))
    return hp


def build_model(run_config, trial=None, hp=None, similarities_subdir=None):
    """``hp``: the hyper-parameters themselves (a restored run's hyperparams.json, train.py:233-237) instead of the config's.
    ``similarities_subdir``: the similarity cache lives in that subdirectory of the dataset's (a search trial's)."""
    if hp is None:
        hp = get_hyperparams(run_config, trial or FixedTrial())
    if 'seed' in hp:
        torch.manual_seed(hp['seed'])
        np.random.seed(hp['seed'])
        random.seed(hp['seed'])
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(hp['seed'])
    paths = dataset_paths(run_config['data']['task'], hp.get('embedding_type', 'gin'))
    if similarities_subdir is not None:
        paths['similarities_path'] = str(Path(paths['similarities_path']) / similarities_subdir)
    return SubGNN(hp, **paths), hp


class Trainer:
    """The slice of pl.Trainer the reference uses (train_config.py:121-156): max_epochs,
    gradient clipping, validation every epoch, best-by-monitor bookkeeping."""

    def __init__(self, max_epochs, gradient_clip_val=0.0, monitor='val_micro_f1', mode='max', log=print,
                 hip_graph_step=True, checkpoint_dir=None, checkpoint_k=0, auto_lr_find=False):
        self.max_epochs, self.clip, self.monitor, self.mode, self.log = max_epochs, gradient_clip_val, monitor, mode, log
        # auto_lr_find (pl.Trainer's): True or the name of a hyper-parameter -- a fresh fit runs ``lr_find`` first and trains at
        # its suggestion (subgnn_amd/lr_find.py); the finder's result stays on ``lr_finder``
        self.auto_lr_find, self.lr_finder, self.lr_finder_configured = auto_lr_find, None, None
        self.best, self.history = None, []
        # checkpoint_k >= 1: the k best epochs by ``monitor`` (checkpoint.TopK, PL 0.7.1's rule) are kept as device copies and
        # written to ``checkpoint_dir`` with last.ckpt (the resume state) when fit returns; 0 writes nothing
        self.checkpoint_dir = Path(checkpoint_dir) if checkpoint_dir is not None else None
        self.checkpoint_k = int(checkpoint_k)
        if self.checkpoint_k > 0 and self.checkpoint_dir is None:
            raise ValueError('checkpoint_k > 0 needs a checkpoint_dir')
        self.top_k = checkpoint.TopK(self.checkpoint_k, mode)
        self.global_step = 0
        # Full batches replay a recorded step (graph_step.CapturedTrainStep) unless hparams['hip_graph_step'] is False: at the
        # reference's batch sizes the eager step is bound by the host's ~250 launches (3.5-11.5 ms against 1.3-4.6 ms replayed,
        # profiles/r03_bench_standin_*.json).  A short last batch runs eagerly; a model whose step cannot be recorded (an
        # operation that needs the host inside training_step) is reported and trained eagerly.  With
        # hparams['resample_anchor_patches'] the prepared tensors change at every epoch end, so the step is recorded again
        # once per epoch (a device synchronisation + one capture: ~the cost of 3-4 eager steps per epoch).
        self.hip_graph_step = bool(hip_graph_step) and torch.cuda.is_available()
        # measurement aid (standins.bench_config's ``epoch`` object): a list makes ``fit`` append one dict of wall-clock phase
        # times per epoch (each phase then ends with a device synchronisation -- not for a production run)
        self.phase_times = None

    def _phase(self, rec, name, t0):
        if rec is None:
            return t0
        import time
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rec[name] = rec.get(name, 0.0) + (t1 - t0)
        return t1

    def lr_find(self, model, min_lr=1e-8, max_lr=1.0, num_training=100, mode='exponential', early_stop_threshold=4.0):
        """pl.Trainer.lr_find: a learning-rate range test with this trainer's step and clip -> lr_find.LRFinder (``results``,
        ``suggestion()``).  The model is left as it was (subgnn_amd/lr_find.py)."""
        return range_test.run(self, model, min_lr, max_lr, num_training, mode, early_stop_threshold)

    def _find_lr(self, model):
        """Trainer(auto_lr_find): the suggestion becomes the hyper-parameter ``configure_optimizers`` reads; without one the
        configured rate stays."""
        key = range_test.lr_key(model.hparams, self.auto_lr_find)
        self.lr_finder_configured = model.hparams[key]
        self.lr_finder = self.lr_find(model)
        lr = self.lr_finder.suggestion()
        if lr is None:
            self.log('lr_find: no suggestion after %d steps; keeping %s = %s' % (self.lr_finder.steps, key, model.hparams[key]))
        else:
            model.hparams[key] = lr
            self.log('learning rate set to %s' % (lr,))

    def _eager_step(self, model, opt, batch, bi):
        return train_step(model, opt, batch, self.clip)[0]

    def _validation_outputs(self, model):
        """[validation_step(batch) for batch in val_dataloader] (train_config.py:156-186 via PL's validation loop).  With
        ``hip_graph_step`` the forward of every batch is a replay of ONE recording (graph_step.CapturedEvalStep; a short last
        batch padded with index 0, its padded rows dropped), the logits and labels of the whole epoch come to the host in one
        transfer and the per-batch loss / accuracy / F1 are evaluated there by the same functions -- an eager validation step is
        ~100 launches + three read-backs (2-6 ms at a batch of 64: as much as the epoch's training steps on the small configs)."""
        loader = model.val_dataloader()
        if not self.hip_graph_step or len(loader) == 0:
            return [model.validation_step(b, i) for i, b in enumerate(loader)]
        cap = self.__dict__.get('_captured_eval')
        if cap is None or cap.model is not model or cap.stale() or cap.B != min(loader.bs, loader.n):
            cap = self.__dict__['_captured_eval'] = CapturedEvalStep(model, min(loader.bs, loader.n), 'val', warmup=1)
        kept, sizes = [], []
        try:
            for idx in loader.index_batches():
                n = idx.numel()
                if n < cap.B:
                    idx = torch.cat([idx, idx.new_zeros(cap.B - n)])
                logits, labels = cap.replay(idx)
                kept.append((logits[:n].clone(), labels[:n].clone()))
                sizes.append(n)
        except StepNotRecordable as ex:
            self.log('hip_graph_step: the validation forward could not be recorded (%s); validating eagerly' % (ex,))
            self.__dict__['_captured_eval'] = None
            return [model.validation_step(b, i) for i, b in enumerate(loader)]
        all_logits = torch.cat([a for a, _ in kept], 0).cpu()              # one transfer (and the one wait of the epoch's validation)
        all_labels = torch.cat([b for _, b in kept], 0).cpu()
        from . import ops
        ops.poll_index_errors(block=True)
        outs, lo = [], 0
        for n in sizes:
            outs.append(model.val_test_outputs('val', all_logits[lo:lo + n], all_labels[lo:lo + n].squeeze(-1)))
            lo += n
        return outs

    def fit(self, model, prepared=False, resume_from=None, epoch_callback=None):
        """``prepared``: the caller has already run prepare_data (or hotpath.prepare_sparse for graphs whose dense structures
        cannot exist).  ``resume_from``: a last.ckpt written by a fit with checkpoint_k >= 1 -- training continues at its next
        epoch, bit for bit the run it was written by (the weights, the optimizer, the anchor draw, the random generators, the
        head's dropout state and this trainer's bookkeeping are restored; the step is recorded again here).
        ``epoch_callback(epoch, monitored value)``: called after each epoch's validation (and checkpoint bookkeeping); a true
        return stops training after that epoch (a pruned search trial) -- last.ckpt then names the next epoch to run."""
        if resume_from is not None and checkpoint.resume_blocker(model):
            raise ValueError(checkpoint.resume_blocker(model))
        # the recipe around the step (schedule.py): hparams ema_decay / ema_warmup, lr_schedule / lr_warmup_steps / ..., and
        # early_stop_patience / early_stop_min_delta -- all off by default
        hp = model.hparams
        schedule.check_hparams(hp)
        schedule.refuse_multi_rank(hp)
        if not prepared:
            model.prepare_data()
        resume = None
        if resume_from is not None:
            resume = checkpoint.load(resume_from)
            self._resumed_from = resume_from
            checkpoint.check_resumable(model, resume)
            st = resume[checkpoint.RESUME_KEY]
            if st['hip_graph_step'] and not self.hip_graph_step:
                raise ValueError('cannot resume bit for bit: the checkpoint was trained with recorded steps (unpadded eager '
                                 'batches sum in another order); resume with hip_graph_step=True')
            self.hip_graph_step = bool(st['hip_graph_step'])     # (a run that fell back to eager steps continues eagerly)
            if model.hparams.get('resample_anchor_patches') and model.__dict__.get('_resample_epoch', 0) != st['resample_epoch']:
                model.__dict__['_resample_epoch'] = st['resample_epoch']
                model._prepare_anchors_only()
            checkpoint.load_checkpoint(model, resume, weights='raw')
        elif self.auto_lr_find:
            self._find_lr(model)
        if model.hparams.get('gc_freeze', True):
            # everything prepare_data left behind (the loaded dataset: subgraph lists, the graph's containers) lives as long as the
            # run: moved out of the cyclic collector's sight, so that a full collection does not walk a few million long-lived
            # objects in the middle of an epoch
            import gc
            gc.collect()
            gc.freeze()
        # plain Adam over CUDA parameters (what configure_optimizers returns) becomes optim.ClipAdam: same update and clipping
        # rule, the embedding table in one HIP pass, the clip coefficient a device scalar (optim.accelerate)
        # hparams['lr_schedule'] / ['lr_warmup_steps']: the rate of every step of the run as a device table the (recorded) step
        # indexes by its own count -- a host scheduler would be frozen into the recording.  Base rate: configure_optimizers'
        # (auto_lr_find's suggestion on a fresh fit; on a resumed one the rate the interrupted fit trained at)
        # hparams['ema_decay']: the update kernel also keeps an average of the weights, which is what the epoch is validated,
        # ranked, checkpointed and tested with (exchanged in place around the validation, _swap_ema)
        configured = model.configure_optimizers()
        table = None
        if schedule.scheduled(hp):
            base = (resume['optimizer_states'][0]['param_groups'][0]['lr'] if resume is not None
                    else getattr(configured, 'param_groups', [{}])[0].get('lr', hp.get('learning_rate')))
            table = schedule.table_from_hparams(hp, float(base), len(model.train_dataloader()), self.max_epochs)
            table = table.to(model.node_embeddings.weight.device)
        opt = accelerate(configured, self.clip, capturable=self.hip_graph_step, lr_schedule=table,
                         ema_decay=float(hp.get('ema_decay', 0) or 0), ema_warmup=bool(hp.get('ema_warmup') or False))
        averaged = getattr(opt, 'ema', None) is not None
        self._ema_run = (model, opt) if averaged else None
        model.__dict__.pop('_loaded_weights', None)              # (the model holds this run's live weights from here on)
        patience = hp.get('early_stop_patience')
        stopper = schedule.EarlyStop(int(patience), hp.get('early_stop_min_delta') or 0, self.mode) if patience is not None else None
        start = 0
        if resume is not None:
            checkpoint.check_resumable(model, resume, opt)
            start = self._restore(model, opt, resume)
            if stopper is not None and resume[checkpoint.RESUME_KEY].get('early_stop') is not None:
                stopper.load(resume[checkpoint.RESUME_KEY]['early_stop'])     # (a checkpoint without the entry: a fresh counter)
            if self.auto_lr_find:                                # (the rate the interrupted fit found is the optimizer's)
                model.hparams[range_test.lr_key(model.hparams, self.auto_lr_find)] = float(opt.param_groups[0]['lr'])
        captured = None
        if self.hip_graph_step:
            make_capturable(opt)
        import time
        next_epoch = max(start, self.max_epochs)
        self.stopped_epoch = None
        self._stopper = stopper
        last = self.max_epochs
        if stopper is not None and stopper.bad >= stopper.patience:          # a run that had stopped early stays stopped
            self.stopped_epoch = next_epoch = last = start
        for epoch in range(start, last):
            rec = None
            if self.phase_times is not None:
                rec = {'replayed_steps': 0, 'eager_steps': 0, 'recordings': 0}
                self.phase_times.append(rec)
                torch.cuda.synchronize()
            t_ph = time.perf_counter()
            model.train()
            losses = []
            loader = model.train_dataloader()
            if self.hip_graph_step:
                # full batches replay the recorded step (graph_step.py); a ragged last batch, or
                # anchors resampled at the end of the previous epoch, fall back / record again
                if captured is None or captured.stale():
                    captured = CapturedTrainStep(model, opt, loader.bs, self.clip, warmup=3 if captured is None else 0)
                    if rec is not None:
                        rec['recordings'] += 1
                for bi, idx in enumerate(loader.index_batches()):
                    if idx.numel() == loader.bs and self.hip_graph_step:
                        try:
                            losses.append(captured.replay(idx)[0].clone())
                            if rec is not None:
                                rec['replayed_steps' if captured.graph is not None and captured._warm_left == 0 else 'eager_steps'] += 1
                            continue
                        except StepNotRecordable as ex:
                            # only a failure of the RECORDING falls back (an error of the eager warm-up steps or of a replay is
                            # the step's own and propagates); the optimizer returns to its eager form: the steps that follow
                            # are the ones hip_graph_step=False would have run
                            self.log('hip_graph_step: the training step could not be recorded (%s); training eagerly' % (ex,))
                            self.hip_graph_step = False
                            make_eager(opt)
                            torch.cuda.synchronize()
                    losses.append(self._eager_step(model, opt, model.make_batch('train', idx), bi))
                    if rec is not None:
                        rec['eager_steps'] += 1
            else:
                for bi, batch in enumerate(loader):
                    losses.append(self._eager_step(model, opt, batch, bi))
                    if rec is not None:
                        rec['eager_steps'] += 1
            t_ph = self._phase(rec, 'train_steps_s', t_ph)
            model.eval()
            if averaged:
                self._swap_ema(model, opt)
            with torch.no_grad():
                outs = self._validation_outputs(model)
                t_ph = self._phase(rec, 'validation_steps_s', t_ph)
                if rec is not None:
                    rec['validation_batches'] = len(outs)
                drawn = model.__dict__.get('_resample_epoch', 0)      # (the anchor draw this epoch was validated with)
                res = model.validation_epoch_end(outs)
                t_ph = self._phase(rec, 'validation_epoch_end_s', t_ph)
            if averaged:                                         # (before the epoch is kept: state_dict stays the raw weights)
                self._swap_ema(model, opt)
            val = float(res['log'][self.monitor])
            if self.best is None or (val > self.best if self.mode == 'max' else val < self.best):
                self.best = val
            self.global_step += len(losses)
            if self.checkpoint_k > 0:
                kept = self._keep(model, opt, epoch, val, res['log'], drawn)
                if rec is not None:
                    rec['checkpoint_kept'] = kept
                    t_ph = self._phase(rec, 'checkpoint_s', t_ph)
            tl = float(torch.stack(losses).mean()) if losses else float('nan')
            self.history.append({'epoch': epoch, 'train_loss': tl, 'val_loss': float(res['avg_val_loss']), self.monitor: val})
            self.log('epoch %d  train_loss %.4f  val_loss %.4f  %s %.4f' % (epoch, tl, float(res['avg_val_loss']), self.monitor, val))
            stop = stopper is not None and stopper.update(val)
            if epoch_callback is not None and epoch_callback(epoch, val):
                self.stopped_epoch = next_epoch = epoch + 1
                self.log('stopped after epoch %d by the epoch callback' % epoch)
                break
            if stop:
                self.stopped_epoch = next_epoch = epoch + 1
                self.log('stopped after epoch %d: %s has not improved by more than %g for %d epochs' % (
                    epoch, self.monitor, stopper.min_delta, stopper.patience))
                break
        if self.checkpoint_k > 0:
            self._write(model, opt, next_epoch)
        return self

    def _swap_ema(self, model, opt):
        """Parameters <-> their averages, in place (ClipAdam.swap_ema): the recorded eval forward reads the parameters' own
        storage; what the model derived from the weights (the half-precision table) is refreshed by its next reader."""
        if hasattr(model, 'invalidate_half_table'):
            model.invalidate_half_table()
        opt.swap_ema()
        if hasattr(model, 'invalidate_half_table'):
            model.invalidate_half_table()

    # -- checkpoints (checkpoint.py) ------------------------------------------------------------------------------------------
    def _state_tensors(self, model, opt):
        """The live tensors a kept epoch copies -- the model's state_dict, then the optimizer's state -- with the structures
        that name them.  Looked up once per fit (and again after a fall-back to eager steps replaces the step counters)."""
        key = (id(model), id(opt), self.hip_graph_step)
        if self.__dict__.get('_ck_key') != key:
            sd = model.state_dict()
            refs = checkpoint.optimizer_state_refs(opt)
            self._ck_refs = (list(sd), refs, list(sd.values()) + checkpoint._leaves(refs, []))
            self._ck_key = key
        keys, refs, src = self._ck_refs
        if not self.hip_graph_step:                              # (host step counts: read now, they are not in ``src``)
            refs = checkpoint.optimizer_state_refs(opt)
        return keys, refs, src

    def _keep(self, model, opt, epoch, value, logs, drawn):
        enters, out = self.top_k.offer(epoch, value)
        if not enters:
            return False
        if out is not None:
            self.top_k.entries.remove(out)
            if out['slot'] is None:                              # written by an earlier fit of this run (a resumed one)
                self.__dict__.setdefault('_ck_stale', []).append(out['file'])
        slots = self.__dict__.setdefault('_ck_slots', [])
        held = {e['slot'] for e in self.top_k.entries}
        free = next((i for i in range(len(slots)) if i not in held), None)
        if free is None:
            slots.append(checkpoint.Snapshot())
            free = len(slots) - 1
        keys, refs, src = self._state_tensors(model, opt)
        slots[free].capture(src, {'epoch': epoch, 'global_step': self.global_step, 'keys': keys, 'refs': refs,
                                  'resample_epoch': drawn})
        self.top_k.entries.append({'epoch': epoch, 'value': value, 'file': checkpoint.checkpoint_name(epoch, self.monitor, logs),
                                   'slot': free})
        return True

    def _info(self, value, resample_epoch, model=None, opt=None):
        """``ema_decay`` > 0: ``value`` is the AVERAGED model's, and ``ema_params`` names the parameters in the order of the
        optimizer's state (whose 'ema' entries hold the averages): what checkpoint.load_checkpoint serves."""
        info = {'monitor': self.monitor, 'mode': self.mode, 'value': value, 'resample_epoch': resample_epoch, 'ema_decay': 0.0}
        if opt is not None and getattr(opt, 'ema', None) is not None:
            names = {id(p): n for n, p in model.named_parameters()}
            info['ema_decay'] = float(opt.ema_decay)
            info['ema_params'] = [names[id(p)] for p in opt.param_groups[0]['params']]
        return info

    def _write(self, model, opt, next_epoch):
        """The kept epochs' files and last.ckpt (the run's state now), written when fit returns."""
        import time
        t0 = time.perf_counter()
        d = self.checkpoint_dir
        d.mkdir(parents=True, exist_ok=True)
        slots = self.__dict__.get('_ck_slots', [])
        for e in self.top_k.entries:
            if e['slot'] is None:
                continue
            snap = slots[e['slot']]
            keys, refs, meta = snap.meta['keys'], snap.meta['refs'], snap.meta
            n = len(keys)
            checkpoint.save({'epoch': meta['epoch'], 'global_step': meta['global_step'],
                             'state_dict': {k: t.cpu() for k, t in zip(keys, snap.bufs[:n])},
                             'optimizer_states': [checkpoint._optimizer_for_file(opt, refs, snap.bufs[n:])],
                             checkpoint.INFO_KEY: self._info(e['value'], meta['resample_epoch'], model, opt)}, d / e['file'])
            e['slot'] = None                                     # (on disk now)
        for f in self.__dict__.pop('_ck_stale', []):
            if (d / f).exists() and f not in {e['file'] for e in self.top_k.entries}:
                (d / f).unlink()
        self.__dict__.pop('_ck_slots', None)
        dev = model.node_embeddings.weight.device
        head = model.__dict__.get('_head_rng')
        resume = {'next_epoch': int(next_epoch), 'optimizer': checkpoint.optimizer_kind(opt), 'hip_graph_step': self.hip_graph_step,
                  'generators': checkpoint.generator_states(dev), 'head_rng': head.cpu() if head is not None else None,
                  'resample_epoch': int(model.__dict__.get('_resample_epoch', 0)),
                  'metric_scores': list(model.metric_scores), 'history': list(self.history), 'best': self.best,
                  'top_k': [dict(e) for e in self.top_k.entries], 'k': self.checkpoint_k, 'monitor': self.monitor,
                  'mode': self.mode}
        stopper = self.__dict__.get('_stopper')
        if stopper is not None:
            resume['early_stop'] = stopper.state()
        last = {'epoch': int(next_epoch) - 1, 'global_step': self.global_step,
                'state_dict': checkpoint.to_cpu(model.state_dict()), 'optimizer_states': [checkpoint.to_cpu(opt.state_dict())],
                checkpoint.RESUME_KEY: resume}
        if getattr(opt, 'ema', None) is not None:                # (the last epoch's averages can be served from it too)
            last[checkpoint.INFO_KEY] = self._info(self.history[-1][self.monitor] if self.history else None,
                                                   resume['resample_epoch'], model, opt)
        checkpoint.save(last, d / checkpoint.LAST)
        self.checkpoint_write_s = time.perf_counter() - t0

    def _restore(self, model, opt, ck):
        """The resume half of ``fit`` after the weights: optimizer, bookkeeping, generators.  -> the epoch to continue at."""
        st = ck[checkpoint.RESUME_KEY]
        if st['monitor'] != self.monitor or st['mode'] != self.mode:
            raise ValueError('cannot resume: the checkpoint monitors %s (%s), this trainer %s (%s)' % (
                st['monitor'], st['mode'], self.monitor, self.mode))
        if self.checkpoint_k == 0:                               # (a resumed run checkpoints as the run it continues did)
            self.checkpoint_k, self.top_k = int(st['k']), checkpoint.TopK(st['k'], self.mode)
            if self.checkpoint_dir is None:
                self.checkpoint_dir = Path(self.__dict__['_resumed_from']).parent
        opt.load_state_dict(ck['optimizer_states'][0])
        dev = model.node_embeddings.weight.device
        if st['head_rng'] is not None:
            model.__dict__['_head_rng'] = st['head_rng'].to(dev)
        model.metric_scores[:] = st['metric_scores']
        self.history, self.best, self.global_step = list(st['history']), st['best'], int(ck['global_step'])
        self.top_k.entries = []
        for e in sorted(st['top_k'], key=lambda e: e['epoch']):     # (already on disk: a smaller k keeps the best of them)
            enters, out = self.top_k.offer(e['epoch'], e['value'])
            if out is not None:
                self.top_k.entries.remove(out)
                self.__dict__.setdefault('_ck_stale', []).append(out['file'])
            if enters:
                self.top_k.entries.append(dict(e, slot=None))
            elif self.checkpoint_k > 0:
                self.__dict__.setdefault('_ck_stale', []).append(e['file'])
        checkpoint.set_generator_states(st['generators'], dev)
        return int(st['next_epoch'])

    def best_checkpoint_path(self):
        """The file of the best kept epoch (ties: the earliest), or None."""
        b = self.top_k.best()
        return self.checkpoint_dir / b['file'] if b is not None else None

    def test(self, model):
        """After a fit with ``ema_decay`` > 0 the model this trainer trained is tested with its averaged weights (exchanged in
        place and back) -- unless a checkpoint was loaded into it since: load_checkpoint has then put the weights to serve there."""
        run = self.__dict__.get('_ema_run')
        swap = run is not None and run[0] is model and model.__dict__.get('_loaded_weights') is None
        if swap:
            self._swap_ema(model, run[1])
        model.eval()
        try:
            with torch.no_grad():
                outs = [model.test_step(b, i) for i, b in enumerate(model.test_dataloader())]
                return model.test_epoch_end(outs)
        finally:
            if swap:
                self._swap_ema(model, run[1])


def write_hyperparams(results_dir, hp):
    """``results_dir/hyperparams.json``: the run's hyper-parameters as configured (train.py:174-183) -- what ``restore_path``
    reads back.  Values stay in their configured form ('balanced' for a loss weight stays the word: the weights are rebuilt from
    it and the training split)."""
    Path(results_dir).mkdir(parents=True, exist_ok=True)
    with open(Path(results_dir) / 'hyperparams.json', 'w') as f:
        json.dump({k: v for k, v in hp.items()}, f, indent=2, default=str)


def train_model(run_config, trial=None, results_dir=None, log=print, checkpoint_k=0, restore_path=None, restore_name=None,
                no_train=False, run_test=False, resume=False, max_epochs=None, epoch_callback=None, similarities_subdir=None,
                auto_lr_find=False):
    """train.py's train_model (train.py:375-420) for one run.
    ``checkpoint_k``: keep the k best epochs by the monitored metric in ``results_dir`` (ModelCheckpoint, train.py:327-334).
    ``restore_path``: hyper-parameters from ``restore_path/hyperparams.json`` (``max_epochs`` overrides them); with
    ``restore_name`` the weights of that checkpoint are loaded after prepare_data; ``resume`` continues from
    ``restore_path/last.ckpt`` bit for bit.  ``no_train``: test the restored model without training (train.py:392-411).
    ``run_test``: after training, test the best checkpoint (the last epoch when nothing was checkpointed) and write
    ``test_results.json``.  ``epoch_callback``: Trainer.fit's; ``similarities_subdir``: build_model's (both for a search trial).
    ``auto_lr_find``: honour the hyper-parameter ``auto_lr_find`` (Trainer(auto_lr_find=hp['auto_lr_find']), train.py:297-298);
    when the finder ran, ``lr_find.json`` records it.  hyperparams.json keeps the configured rate (written before fit, as the
    reference does); the checkpoints' optimizer state holds the found one.
    -> (best monitored value, model, trainer)."""
    hp = None
    if restore_path is not None:
        hp = json.loads((Path(restore_path) / 'hyperparams.json').read_text(), object_pairs_hook=OrderedDict)
        if results_dir is None and not no_train:
            results_dir = restore_path
    elif resume or restore_name is not None:
        raise ValueError('resume / restore_name need restore_path')
    if max_epochs:
        hp = hp if hp is not None else get_hyperparams(run_config, trial or FixedTrial())
        hp['max_epochs'] = int(max_epochs)
    model, hp = build_model(run_config, trial, hp, similarities_subdir=similarities_subdir)
    opt_cfg = run_config.get('optuna', {})
    monitor = opt_cfg.get('monitor_metric', 'val_micro_f1')
    mode = 'max' if opt_cfg.get('opt_direction', 'maximize') == 'maximize' else 'min'
    trainer = Trainer(hp['max_epochs'], hp.get('grad_clip', 0.0), monitor, mode, log,
                      hip_graph_step=bool(hp.get('hip_graph_step', True)), checkpoint_dir=results_dir,
                      checkpoint_k=0 if no_train else checkpoint_k,
                      auto_lr_find=hp.get('auto_lr_find', False) if auto_lr_find else False)
    if results_dir is not None and not no_train:
        write_hyperparams(results_dir, hp)
    prepared = False
    if restore_name is not None:
        model.prepare_data()
        prepared = True
        checkpoint.load_checkpoint(model, Path(restore_path) / restore_name)
    if not no_train:
        trainer.fit(model, prepared=prepared, resume_from=Path(restore_path) / checkpoint.LAST if resume else None,
                    epoch_callback=epoch_callback)
        if trainer.lr_finder is not None and results_dir is not None:
            with open(Path(results_dir) / 'lr_find.json', 'w') as f:
                json.dump(trainer.lr_finder.summary(trainer.lr_finder_configured), f, indent=2)
    if no_train or run_test:
        if not prepared and no_train:
            model.prepare_data()
        best_file = trainer.best_checkpoint_path() if not no_train else None
        if best_file is not None:
            checkpoint.load_checkpoint(model, best_file)
        trainer.test(model)
        out = results_dir if results_dir is not None else restore_path
        if out is not None:
            with open(Path(out) / 'test_results.json', 'w') as f:
                json.dump({k: float(v) for k, v in model.test_results.items()}, f, indent=2)
    if model.metric_scores:
        scores = {k: (float(v) if hasattr(v, '__float__') else v) for k, v in model.metric_scores[-1].items()}
        if results_dir is not None:
            with open(Path(results_dir) / 'final_metric_scores.json', 'w') as f:
                json.dump(scores, f, indent=2)
    return trainer.best, model, trainer


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Train SubGNN on MI355X from a reference-format config.json')
    ap.add_argument('-config_path', type=str, required=True)
    ap.add_argument('-project_root', type=str, default=None, help='overrides subgnn_amd.config.PROJECT_ROOT')
    ap.add_argument('-results_dir', type=str, default=None)
    ap.add_argument('-max_epochs', type=int, default=None, help='overrides the hyper-parameters (a restored run\'s too)')
    ap.add_argument('-checkpoint_k', type=int, default=None,
                    help='keep the k best epochs by the monitored metric (default 0: none; 3 per trial with -search)')
    ap.add_argument('-restoreModelPath', type=str, default=None, help='directory of a run: its hyperparams.json is used')
    ap.add_argument('-restoreModelName', type=str, default=None, help='checkpoint file in -restoreModelPath to load')
    ap.add_argument('-noTrain', action='store_true', help='test the restored model without training')
    ap.add_argument('-runTest', action='store_true', help='test after training (the best checkpoint) -> test_results.json')
    ap.add_argument('-resume', action='store_true', help='continue the run in -restoreModelPath from its last.ckpt')
    ap.add_argument('-search', action='store_true', help='run the hyper-parameter study (subgnn_amd.search) instead of one run')
    ap.add_argument('-auto_lr_find', action='store_true',
                    help="honour the hyper-parameter auto_lr_find: a learning-rate range test before training (lr_find.json)")
    from .search import add_search_args
    add_search_args(ap)
    args = ap.parse_args(argv)
    if args.search and (args.restoreModelPath or args.results_dir or args.max_epochs or args.runTest):
        ap.error('-search takes none of -restoreModelPath, -results_dir, -max_epochs, -runTest')
    if not args.search and (args.study_path or args.n_workers is not None):
        ap.error('-study_path and -n_workers need -search')
    if args.checkpoint_k is None:
        args.checkpoint_k = 3 if args.search else 0
    if (args.resume or args.restoreModelName or args.noTrain) and not args.restoreModelPath:
        ap.error('-resume, -restoreModelName and -noTrain need -restoreModelPath')
    if args.noTrain and not args.restoreModelName:
        ap.error('-noTrain needs -restoreModelName')
    if args.resume and (args.noTrain or args.restoreModelName):
        ap.error('-resume restores last.ckpt: it takes neither -restoreModelName nor -noTrain')
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.search:
        from . import search
        rc = search.main_from_args(args)
        if rc:
            raise SystemExit(rc)
        return None
    if args.project_root:
        config.PROJECT_ROOT = Path(args.project_root)
    run_config = read_json(args.config_path)
    best, model, trainer = train_model(run_config, results_dir=args.results_dir, checkpoint_k=args.checkpoint_k,
                                       restore_path=args.restoreModelPath, restore_name=args.restoreModelName,
                                       no_train=args.noTrain, run_test=args.runTest, resume=args.resume,
                                       max_epochs=args.max_epochs, auto_lr_find=args.auto_lr_find)
    if best is not None:
        print('best %s: %.4f' % (trainer.monitor, best))
    return best


if __name__ == '__main__':
    main()

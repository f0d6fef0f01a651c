"""Checkpoints: the best epochs by a monitored metric (Lightning 0.7.1's ModelCheckpoint(save_top_k=k), which the reference's
train.py:327-334 installs), a full resume state (``last.ckpt``), and the reference's loader (train.py:265-271).

Files.  ``epoch=<e>-<monitor>=<v:.2f>-val_acc=<..>-val_auroc=<..>.ckpt`` holds what a PL 0.7.1 checkpoint holds --
``epoch``, ``global_step``, ``state_dict`` (CPU tensors, the module's own key names), ``optimizer_states`` -- plus one
namespaced entry (``subgnn_amd``: the monitored value and the anchor draw the epoch was validated with).  It loads with a
plain ``torch.load`` (weights_only) and with the reference's ``checkpoint['state_dict']``.  ``last.ckpt`` has the same keys and
a ``subgnn_amd_resume`` entry with everything a bit-exact continuation needs (``Trainer.fit(resume_from=...)``); its name does
not start with ``epoch``, so the reference's file search (train.py:398-408, test.py:73-82) skips it.

Cost.  A kept epoch is copied on the device, one multi-tensor copy into buffers allocated once per slot; the keep decision
reads the host float ``validation_epoch_end`` already returned.  The files are written when ``fit`` returns.
"""
import math
import os
import random
import re
from pathlib import Path

import numpy as np
import torch

LAST = 'last.ckpt'
RESUME_KEY = 'subgnn_amd_resume'
INFO_KEY = 'subgnn_amd'


# -- which epochs are kept ----------------------------------------------------------------------------------------------------
class TopK:
    """The k best epochs by a monitored value, PL 0.7.1's rule: while fewer than k are kept every epoch enters; after that an
    epoch enters only on STRICT improvement over the k-th best (``>`` for mode 'max', ``<`` for 'min'), which it replaces.
    Among equal values the earliest epoch is kept: an equal newcomer does not enter, and of several equal k-th best entries
    the latest leaves.  A NaN value never enters (it would compare false against everything and never leave).
    Entries: dicts {'epoch', 'value', 'file', 'slot'}, in the order they entered."""

    def __init__(self, k, mode='max'):
        if mode not in ('max', 'min'):
            raise ValueError("mode must be 'max' or 'min'")
        self.k, self.mode, self.entries = int(k), mode, []

    def _better(self, a, b):
        return a > b if self.mode == 'max' else a < b

    def _rank(self, e):
        """Sort key: best first; among equal values the earliest epoch first."""
        return (-e['value'] if self.mode == 'max' else e['value'], e['epoch'])

    def worst(self):
        return max(self.entries, key=self._rank) if self.entries else None

    def best(self):
        return min(self.entries, key=self._rank) if self.entries else None

    def offer(self, epoch, value):
        """-> (enters, evicted entry or None)."""
        if self.k <= 0 or value is None or math.isnan(value):
            return False, None
        if len(self.entries) < self.k:
            return True, None
        w = self.worst()
        return (True, w) if self._better(value, w['value']) else (False, None)


def _fmt(v):
    v = float(v)
    return 'nan' if math.isnan(v) else '%.2f' % v


def checkpoint_name(epoch, monitor, logs):
    """PL 0.7.1's name for the filepath template "{epoch}-{<monitor>:.2f}-{val_acc:.2f}-{val_auroc:.2f}" (train.py:329): each
    field written as ``name=value``; a field named twice (monitor 'val_acc') once."""
    fields = []
    for k in (monitor, 'val_acc', 'val_auroc'):
        if k not in fields:
            fields.append(k)
    return '-'.join(['epoch=%d' % int(epoch)] + ['%s=%s' % (k, _fmt(logs.get(k, float('nan')))) for k in fields]) + '.ckpt'


# -- live state as trees of tensors ---------------------------------------------------------------------------------------------
def optimizer_state_refs(opt):
    """The optimizer's state_dict structure holding its LIVE tensors (no copies, no read-back): torch's Optimizer.state_dict
    already references them; ClipAdam.state_refs keeps device step counts as 0-d views."""
    return opt.state_refs() if hasattr(opt, 'state_refs') else opt.state_dict()


def _leaves(tree, out):
    if torch.is_tensor(tree):
        out.append(tree)
    elif isinstance(tree, dict):
        for v in tree.values():
            _leaves(v, out)
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            _leaves(v, out)
    return out


def _rebuild(tree, it, fn):
    """``tree`` with every tensor leaf replaced by fn(next(it))."""
    if torch.is_tensor(tree):
        return fn(next(it))
    if isinstance(tree, dict):
        return {k: _rebuild(v, it, fn) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_rebuild(v, it, fn) for v in tree)
    return tree


def to_cpu(tree):
    return _rebuild(tree, iter(_leaves(tree, [])), lambda t: t.detach().cpu())


def _optimizer_for_file(opt, refs, tensors):
    """A state_dict of ``opt``'s form from ``refs`` (optimizer_state_refs) with its tensors taken from ``tensors``, on the CPU;
    ClipAdam's device step counts become the ints its state_dict holds."""
    sd = _rebuild(refs, iter(tensors), lambda t: t.detach().cpu())
    if hasattr(opt, 'state_refs'):
        for ent in sd['state'].values():
            if torch.is_tensor(ent['step']):
                ent['step'] = int(ent['step'])
    return sd


class Snapshot:
    """Device copies of the model's state_dict tensors and the optimizer's state, for one kept epoch.  Buffers are allocated
    at the first capture and reused; a capture is one multi-tensor copy per dtype (no host synchronisation; a list of mixed
    dtypes would take torch's per-tensor route: one launch per tensor, ~1.5 ms of host time for the stand-ins' ~300)."""

    def __init__(self):
        self.bufs, self.groups, self.meta = None, None, None

    def capture(self, src, meta):
        if self.bufs is None or len(self.bufs) != len(src) or any(
                b.shape != s.shape or b.dtype != s.dtype or b.device != s.device for b, s in zip(self.bufs, src)):
            self.bufs = [torch.empty_like(s) for s in src]
            by = {}
            for i, s in enumerate(src):
                by.setdefault((s.dtype, s.device), []).append(i)
            self.groups = list(by.values())
        with torch.no_grad():
            for idx in self.groups:
                torch._foreach_copy_([self.bufs[i] for i in idx], [src[i] for i in idx])
        self.meta = dict(meta)

    def restore(self, dst):
        """The captured values back into ``dst`` (the tensors ``capture`` was given, or tensors of the same shapes): the same
        multi-tensor copies the other way, in place, so a recording that reads ``dst`` sees them."""
        with torch.no_grad():
            for idx in self.groups:
                torch._foreach_copy_([dst[i] for i in idx], [self.bufs[i] for i in idx])


# -- files --------------------------------------------------------------------------------------------------------------------
def save(obj, path):
    """torch.save through a temporary name, so that an interrupted write never leaves a truncated checkpoint behind."""
    path = Path(path)
    tmp = path.with_name(path.name + '.tmp')
    torch.save(obj, tmp)
    os.replace(tmp, path)


def load(path, weights_only=False):
    return torch.load(path, map_location='cpu', weights_only=weights_only)


def ema_tensors(ck):
    """{parameter name: averaged tensor} of a checkpoint written by a run with ``ema_decay`` > 0, or None.  The average travels
    as the ``'ema'`` entry of each parameter's optimizer state; the file's info names the parameters in the optimizer's order
    (``'ema_params'``), so reading it does not depend on rebuilding the optimizer."""
    info = ck.get(INFO_KEY) or {}
    names = info.get('ema_params')
    if not info.get('ema_decay') or not names:
        return None
    states = ck.get('optimizer_states') or []
    state = states[0].get('state') if states and isinstance(states[0], dict) else None
    if not state:
        return None
    out = {}
    for i, name in enumerate(names):
        ent = state.get(i)
        if ent is None or ent.get('ema') is None:
            return None
        out[name] = ent['ema']
    return out


def load_checkpoint(model, path_or_dict, weights='auto'):
    """Load a checkpoint's ``state_dict`` into ``model`` as the reference does (train.py:265-271): keys the model lacks are
    dropped, a key the checkpoint lacks raises (``load_state_dict``'s strict check), tensors go to the model's device.  The
    values are COPIED into the model's existing tensors, never rebound, so a training step already recorded in a hipGraph
    (graph_step.CapturedTrainStep) reads the loaded weights.  Works before or after ``prepare_data`` / ``hotpath.prepare_sparse``.
    A file of this project also names the anchor draw its epoch was validated with: a prepared model with
    ``resample_anchor_patches`` draws those anchors again, so that testing it does not depend on how many epochs ran since.
    ``weights``: a run with ``ema_decay`` > 0 validated, ranked and kept its epochs by the AVERAGED weights; its files hold
    the raw weights in ``state_dict`` (what a resume and the reference's loader read) and the averages beside the moments.
    'auto' (the default, what the tools call) copies the averages over the parameters when the file says the run validated
    with them and they are there; 'raw' never does (``fit(resume_from=)``); 'ema' raises when the file has none.  The model then
    carries ``_loaded_weights`` = 'ema' or 'raw' (``Trainer.test`` does not exchange the weights of a loaded model again).
    Returns the checkpoint dict."""
    if weights not in ('auto', 'raw', 'ema'):
        raise ValueError("load_checkpoint: weights must be 'auto', 'raw' or 'ema', not %r" % (weights,))
    ck = load(path_or_dict) if isinstance(path_or_dict, (str, os.PathLike)) else path_or_dict
    if 'state_dict' not in ck:
        raise KeyError("checkpoint has no 'state_dict'")
    own = model.state_dict()
    sd = {k: v for k, v in ck['state_dict'].items() if k in own}
    avg = ema_tensors(ck) if weights != 'raw' else None
    if weights == 'ema' and avg is None:
        raise ValueError("load_checkpoint(weights='ema'): the checkpoint holds no averaged weights (its run had ema_decay = 0, or "
                         "it was not written by this project)")
    if avg is not None:
        named = dict(model.named_parameters())
        for name, t in avg.items():
            if name not in named or tuple(named[name].shape) != tuple(t.shape):
                raise ValueError('load_checkpoint: the averaged %r of the checkpoint does not match the model' % (name,))
    with torch.no_grad():
        model.load_state_dict(sd)                       # (copy_ into the existing parameters and buffers; strict on missing keys)
        if avg is not None:
            for name, t in avg.items():
                named[name].copy_(t)
    model.__dict__['_loaded_weights'] = 'ema' if avg is not None else 'raw'
    if hasattr(model, 'invalidate_half_table'):
        model.invalidate_half_table()
    info = ck.get(INFO_KEY) or {}
    ep = info.get('resample_epoch')
    if ep is not None and _prepared(model) and model.hparams.get('resample_anchor_patches'):
        if model.__dict__.get('_resample_epoch', 0) != ep:
            model.__dict__['_resample_epoch'] = int(ep)
            model._prepare_anchors_only()
    return ck


def _prepared(model):
    return getattr(model, 'train_cc_ids', None) is not None


def best_checkpoint(directory, monitor='val_micro_f1', mode='max'):
    """The best ``epoch*.ckpt`` in ``directory``: by the value this project's files store, else by the ``<monitor>=<v>`` field
    of the name (a Lightning file); among equal values the earliest epoch.  Unlike the reference (test.py:73-77, train.py:
    398-408, which take whichever file ``os.listdir`` lists last) the choice does not depend on the directory's order.
    -> the file name, or None when there is none."""
    names = sorted(n for n in os.listdir(directory) if n.startswith('epoch') and n.endswith('.ckpt'))
    table = TopK(len(names), mode)
    for n in names:
        ck = load(Path(directory) / n)
        info = ck.get(INFO_KEY) or {}
        v = info.get('value') if info.get('monitor') == monitor else None
        if v is None:
            m = re.search(r'(?:^|-)%s=(-?[0-9.]+|nan)' % re.escape(monitor), n[:-len('.ckpt')])
            v = float(m.group(1)) if m else float('nan')
        if not math.isnan(v):
            table.entries.append({'epoch': int(ck.get('epoch', 0)), 'value': float(v), 'file': n, 'slot': None})
    b = table.best()
    return b['file'] if b is not None else (names[-1] if names else None)


# -- resume state -------------------------------------------------------------------------------------------------------------
def generator_states(device):
    return {'torch_cpu': torch.get_rng_state(),
            'torch_cuda': torch.cuda.get_rng_state(device) if device.type == 'cuda' else None,
            'numpy': np.random.get_state(), 'python': random.getstate()}


def set_generator_states(st, device):
    """The torch CUDA generator's state is its seed and Philox offset.  A replayed hipGraph advances that offset on the host by
    the recording's whole increment (the capture itself advances nothing), exactly as the eager steps it stands for would, so
    the offset at an epoch boundary is the same whether the epoch's steps ran eagerly, were recorded or were replayed: a
    resumed run that records its step afresh consumes the same offsets as the run it continues."""
    torch.set_rng_state(st['torch_cpu'])
    if st.get('torch_cuda') is not None and device.type == 'cuda':
        torch.cuda.set_rng_state(st['torch_cuda'], device)
    np.random.set_state(st['numpy'])
    random.setstate(st['python'])


def resume_blocker(model):
    """Why ``model`` cannot continue bit for bit in another process, or None.  The one case: inter-layer LSTM dropout on the
    library LSTM (hidden sizes ops.bilstm_layer is not built for).  That LSTM is MIOpen's, whose dropout masks come from a
    dropout descriptor the process creates once, seeded from the CUDA generator, and then advances on the device: no
    generator state saved at an epoch boundary restores it.  (The fused LSTM draws its dropout through
    nn.functional.dropout, from the CUDA generator, and resumes exactly.)"""
    from . import ops
    m = getattr(getattr(model, 'lstm', None), 'lstm', None)
    if m is not None and m.num_layers > 1 and m.dropout > 0 and not ops.lstm_supported(m.input_size, m.hidden_size):
        return ('cannot resume bit for bit: the %d-layer LSTM with lstm_dropout %g runs on the library LSTM at hidden size %d, '
                'whose dropout state lives in the process that trained it' % (m.num_layers, m.dropout, m.hidden_size))
    return None


def check_resumable(model, ck, opt=None):
    """ValueError naming the first difference between a resume checkpoint and ``model`` (and ``opt``)."""
    if RESUME_KEY not in ck:
        raise ValueError('not a resume checkpoint (no %r entry): only %s can be resumed from' % (RESUME_KEY, LAST))
    own, theirs = model.state_dict(), ck['state_dict']
    for k, v in own.items():
        if k not in theirs:
            raise ValueError('cannot resume: the checkpoint has no %r (another model configuration)' % (k,))
        if tuple(theirs[k].shape) != tuple(v.shape) or theirs[k].dtype != v.dtype:
            raise ValueError('cannot resume: %r is %s %s in the checkpoint and %s %s in the model' % (
                k, tuple(theirs[k].shape), theirs[k].dtype, tuple(v.shape), v.dtype))
    for k in theirs:
        if k not in own:
            raise ValueError('cannot resume: the model has no %r (another model configuration)' % (k,))
    if opt is not None:
        kind = ck[RESUME_KEY]['optimizer']
        if kind != optimizer_kind(opt):
            raise ValueError('cannot resume: the checkpoint holds a %s state and this run steps with %s' % (kind, optimizer_kind(opt)))


def optimizer_kind(opt):
    return '%s.%s' % (type(opt).__module__, type(opt).__qualname__)

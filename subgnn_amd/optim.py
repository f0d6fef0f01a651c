"""Gradient clipping + Adam as the reference's caller runs them per step (train_config.py: Trainer(gradient_clip_val)
-> clip_grad_norm_, then SubGNN.configure_optimizers' torch.optim.Adam, SubGNN/SubGNN.py:1156-1161), over every parameter in two
launches (ops.OptimTail: sgnn_optim_sumsq, sgnn_optim_adam) instead of torch's multi-tensor norm, multiply and fused Adam
around a chunked pass over the (N+1, D) embedding table.  Same update rule, same clipping rule (coefficient = min(1, max_norm /
(total_norm + 1e-6)) over ALL parameters, NaN when the norm is NaN, as torch's clamp leaves it); the coefficient stays a device
scalar, so the step has no host round trip."""
import torch

from . import ops


def fusable(params):
    """What ops.OptimTail steps: a non-empty list of float32, contiguous CUDA parameters on one device."""
    return bool(params) and len({p.device for p in params}) == 1 and all(
        p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params)


class ClipAdam:
    """``step()`` = clip_grad_norm_(params, max_norm) followed by Adam(params, lr).step(), non-finite gradients included (a NaN
    anywhere makes every parameter NaN, as there);  ``zero_grad()`` as usual.
    After ``step()`` the gradient of a large parameter is gone (``p.grad is None``): its buffer, zeroed by the update
    kernel, hangs on the parameter (``ops.release_zeroed``) and becomes the next backward's accumulator -- a caller that
    kept a reference to ``p.grad`` across ``step()`` holds that recycled buffer, not the old gradient.  ``release()``
    drops the kept buffers.
    ``lr_schedule``: a float32 CUDA tensor of learning rates read ON THE DEVICE in place of ``lr`` -- step s (the parameters'
    step count) takes ``lr_schedule[min(s, len) - 1]`` (sgnn_optim_adam_lr_table), so a recorded step replays a changing rate
    (lr_find's range test) and the rate never enters the recording key.  All parameters it steps must share one step count:
    an eager step that would update tensors of different counts raises.
    ``ema_decay`` > 0: an exponential moving average of the weights, ``state[id(p)]['ema']`` (initialised to the parameter),
    moved INSIDE the update kernel (sgnn_optim_adam_ema: the parameter is in registers there): e += (1 - d_s) (p_new - e) for
    every element the step updates, d_s = ema_decay, or with ``ema_warmup`` min(ema_decay, (1 + s) / (10 + s)) at the tensor's
    step count s.  The average advances with the tensor's OWN steps: a parameter without a gradient in a step keeps its average
    as it is, and a table row the update skips (never a gradient: p == e bit for bit) costs nothing.  ``swap_ema()``
    exchanges parameters and averages in place (validate / test / serve the averaged model, then swap back); ``step()`` raises
    while they are exchanged."""

    def __init__(self, params, lr, max_norm=None, betas=(0.9, 0.999), eps=1e-8, big_bytes=16 << 20, capturable=False,
                 skip_untouched_rows=True, lr_schedule=None, ema_decay=0.0, ema_warmup=False):
        params = [p for p in params if p.requires_grad]
        if not fusable(params):
            raise ValueError('ClipAdam needs a non-empty list of float32, contiguous CUDA parameters on one device')
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("ClipAdam's ema_decay = %r must lie in [0, 1) (0: no average)" % (ema_decay,))
        self.betas, self.eps, self.max_norm = (float(betas[0]), float(betas[1])), float(eps), max_norm
        # one parameter group, torch-shaped: a learning-rate scheduler (or a caller) that writes param_groups[0]['lr'] is
        # honoured by the next step (``lr`` below reads it); 'params' lists every parameter this optimizer updates
        self.param_groups = [{'params': list(params), 'lr': float(lr), 'betas': self.betas, 'eps': self.eps, 'weight_decay': 0,
                              'amsgrad': False, 'maximize': False, 'max_norm': max_norm, 'ema_decay': float(ema_decay),
                              'ema_warmup': bool(ema_warmup)}]
        # the large parameters (the embedding table): the kernel zeroes their gradients and hands the buffers back as the next
        # backward's accumulators, and skips their untouched rows
        self.big = [p for p in params if p.numel() * 4 >= big_bytes and p.data_ptr() % 16 == 0]
        ids = {id(p) for p in self.big}
        self.small = [p for p in params if id(p) not in ids]
        self.all = self.big + self.small                        # the table first: its workgroups start first
        self.state = {id(p): {'step': 0, 'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)} for p in self.all}
        self.ema = None                                         # the averages, in the order of ``all`` (ema_decay > 0)
        if float(ema_decay) > 0.0:
            for p in self.all:
                self.state[id(p)]['ema'] = p.detach().clone()
            self.ema = [self.state[id(p)]['ema'] for p in self.all]
        self.swapped = False                                    # parameters and averages stand exchanged (swap_ema)
        self.tail = ops.OptimTail(self.all, [self.state[id(p)]['exp_avg'] for p in self.all],
                                  [self.state[id(p)]['exp_avg_sq'] for p in self.all], [id(p) in ids for p in self.all],
                                  row_skip=range(len(self.big)) if skip_untouched_rows else ())
        # capturable: the step counts live on the device, so that a step recorded into a hipGraph (hotpath.CapturedTraining)
        # replays with the right bias corrections; same arithmetic either way
        self.capturable = bool(capturable)
        self.counters = torch.zeros(len(self.all), dtype=torch.int64, device=params[0].device) if self.capturable else None
        self.last_clip = None                                   # (2,) device tensor [coefficient, total norm] of the last step
        if lr_schedule is not None and not (torch.is_tensor(lr_schedule) and lr_schedule.is_cuda and lr_schedule.dim() == 1
                                            and lr_schedule.dtype == torch.float32 and lr_schedule.numel() >= 1
                                            and lr_schedule.is_contiguous() and lr_schedule.device == params[0].device):
            raise ValueError("ClipAdam's lr_schedule must be a non-empty, contiguous 1-D float32 tensor on the parameters' device")
        self.lr_schedule = lr_schedule
        self._sched_which = None                                # the parameters a scheduled step updates (device step counts)

    @property
    def lr(self):
        return float(self.param_groups[0]['lr'])

    @lr.setter
    def lr(self, value):
        self.param_groups[0]['lr'] = float(value)

    @property
    def ema_decay(self):
        return float(self.param_groups[0].get('ema_decay', 0.0))

    def swap_ema(self):
        """Exchange every parameter with its average, in place (ops.OptimTail.swap: one launch per group of tensors, no
        temporary): after an odd number of calls the parameters' own storage holds the averaged weights -- what a recorded
        forward reads -- and ``swapped`` is set.  The caller drops what it derived from the weights (a half-precision copy of
        the table) around it."""
        if self.ema is None:
            raise ValueError('swap_ema: this ClipAdam keeps no weight average (ema_decay = 0)')
        self.tail.swap(range(len(self.all)), self.ema)
        self.swapped = not self.swapped

    def step(self):
        if self.swapped:
            raise RuntimeError('ClipAdam.step while parameters and averages are exchanged: call swap_ema() again first')
        which, grads, takes = [], [], []
        for i, p in enumerate(self.all):
            g = p.grad
            if g is None:
                continue
            take = g.is_contiguous() and g.dtype == torch.float32
            which.append(i)
            grads.append(g if take else g.contiguous().float())
            takes.append(take)
        if not which:
            return
        steps = None
        if self.counters is None:
            steps = [self.state[id(self.all[i])]['step'] + 1 for i in which]
            if self.lr_schedule is not None and len(set(steps)) > 1:
                raise ValueError('a scheduled ClipAdam step would update tensors at different step counts %s: the learning-rate '
                                 'table has one position for all of them' % sorted(set(steps)))
            for i, n in zip(which, steps):
                self.state[id(self.all[i])]['step'] = n
        elif self.lr_schedule is not None:
            # (device counts are not read back: the counts stay equal while every step updates the same parameters)
            if self._sched_which is None:
                self._sched_which = tuple(which)
            elif tuple(which) != self._sched_which:
                raise ValueError('a scheduled ClipAdam step would update another set of parameters than its first step: their '
                                 'step counts would part and the learning-rate table has one position for all of them')
        self.last_clip = self.tail.step(which, grads, self.lr, self.betas, self.eps, self.max_norm, steps=steps,
                                        step_counters=self.counters, lr_table=self.lr_schedule, ema=self.ema,
                                        ema_decay=self.ema_decay, ema_warmup=bool(self.param_groups[0].get('ema_warmup', False)))
        for i, g, take in zip(which, grads, takes):
            p = self.all[i]
            if self.tail.zero[i] and take:                      # (the kernel zeroed the gradient it consumed)
                ops.release_zeroed(p, g)
                p.grad = None
            elif self.tail.zero[i]:
                p.grad = None

    def release(self):
        """Drop the zeroed gradient buffers kept on the large parameters (256 MB for the benchmark's table)."""
        for p in self.big:
            ops.drop_zeroed(p)

    def zero_grad(self, set_to_none=True):
        for p in self.all:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    # -- checkpointing (torch.optim.Optimizer's surface: what a Lightning-style caller saves and restores) ----------------------
    def state_refs(self):
        """``state_dict``'s structure holding the LIVE tensors: no copy and no read-back -- a device step count is a 0-d view
        of the counters (what checkpoint.Snapshot copies on the device when a trainer keeps an epoch)."""
        pos = {id(p): i for i, p in enumerate(self.param_groups[0]['params'])}
        state = {}
        for k, p in enumerate(self.all):
            st = self.state[id(p)]
            ent = {'step': self.counters[k] if self.counters is not None else int(st['step']),
                   'exp_avg': st['exp_avg'], 'exp_avg_sq': st['exp_avg_sq']}
            if 'ema' in st:
                ent['ema'] = st['ema']
            if k in self.tail.seen:
                ent['rows_seen'] = self.tail.seen[k]
            state[pos[id(p)]] = ent
        group = {k: v for k, v in self.param_groups[0].items() if k != 'params'}
        group['params'] = list(range(len(self.param_groups[0]['params'])))
        return {'state': state, 'param_groups': [group]}

    def state_dict(self):
        """Moments, step counts, the row-skip bytes and (ema_decay > 0) the average ``'ema'`` of every parameter, by position in ``param_groups[0]['params']`` (as
        torch keys optimizer state).  Device step counters are read back (one host round trip)."""
        sd = self.state_refs()
        counts = self.counters.tolist() if self.counters is not None else None
        pos = {id(p): i for i, p in enumerate(self.param_groups[0]['params'])}
        for k, p in enumerate(self.all):
            ent = sd['state'][pos[id(p)]]
            ent['step'] = int(counts[k]) if counts is not None else ent['step']
            for name in ('exp_avg', 'exp_avg_sq', 'rows_seen', 'ema'):
                if name in ent:
                    ent[name] = ent[name].detach().clone()
        return sd

    def load_state_dict(self, sd):
        """Inverse of ``state_dict``.  A checkpoint without the row-skip bytes (moments restored from elsewhere) marks every row
        whose first moment is non-zero as seen -- a row with m = v = 0 is exactly the row Adam leaves alone, so skipping only
        those stays bit-identical to the full update.  A checkpoint whose ``'small'`` holds a torch optimizer state (the small
        parameters stepped by torch's Adam) is refused: their moments would be lost."""
        if sd.get('small') is not None:
            raise ValueError("ClipAdam.load_state_dict: this checkpoint keeps the small parameters' Adam state in a separate "
                             "torch optimizer ('small'); ClipAdam keeps every parameter's moments itself and cannot restore it")
        if self.swapped:
            raise RuntimeError('ClipAdam.load_state_dict while parameters and averages are exchanged')
        params = self.param_groups[0]['params']
        keeps = (self.param_groups[0]['ema_decay'], self.param_groups[0]['ema_warmup'])
        for k, v in sd['param_groups'][0].items():
            if k != 'params':
                self.param_groups[0][k] = v
        # (whether there is an average is decided at construction: a state saved without one -- or with one this optimizer
        # does not keep -- leaves the optimizer's own setting; the loop below then starts the average at the parameters)
        if (float(self.param_groups[0].get('ema_decay', 0.0)) > 0) != (self.ema is not None):
            self.param_groups[0]['ema_decay'], self.param_groups[0]['ema_warmup'] = keeps
        self.max_norm = self.param_groups[0].get('max_norm', self.max_norm)
        order = {id(p): k for k, p in enumerate(self.all)}
        for i, ent in sd['state'].items():
            p = params[int(i)]
            st = self.state[id(p)]
            st['exp_avg'].copy_(ent['exp_avg'])
            st['exp_avg_sq'].copy_(ent['exp_avg_sq'])
            st['step'] = int(ent['step'])
            if 'ema' in st:                                      # (a state without the average starts it at the current parameters)
                st['ema'].copy_(ent['ema'] if ent.get('ema') is not None else p.detach())
            k = order[id(p)]
            if self.counters is not None:
                self.counters[k] = int(ent['step'])
            if k in self.tail.seen:
                seen = ent.get('rows_seen')
                if seen is None:
                    seen = ((st['exp_avg'] != 0) | (st['exp_avg_sq'] != 0)).reshape(p.shape[0], -1).any(1).to(torch.uint8)
                self.tail.seen[k].copy_(seen)

    def make_eager(self):
        """Back to host-side step counts (the trainer's fallback when a step cannot be recorded): same arithmetic."""
        self.capturable = False
        if self.counters is not None:
            for p, n in zip(self.all, self.counters.tolist()):
                self.state[id(p)]['step'] = int(n)
            self.counters = None
        return self


TRAINER_BIG_BYTES = 6 << 20        # the embedding table of the stand-ins (7.5-30 MB), not their per-split component embeddings (4.6 MB each)


def accelerate(optimizer, max_norm=None, capturable=False, big_bytes=TRAINER_BIG_BYTES, lr_schedule=None, ema_decay=0.0,
               ema_warmup=False):
    """What ``train_config.Trainer`` steps with: the optimizer ``configure_optimizers`` returned when it is anything but a plain
    ``torch.optim.Adam`` over float32, contiguous CUDA parameters on one device (``fusable``) -- else a ClipAdam with the same
    learning rate, betas and eps that also applies the trainer's ``gradient_clip_val`` (so the caller must NOT clip again): clip
    and Adam over every parameter in two launches, the clip coefficient a device scalar, the gradient of the embedding table
    (and of any other parameter of at least ``big_bytes``) zeroed in the update and its untouched rows skipped -- at a batch
    of 64 torch's chunked multi-tensor Adam over a 9 MB table and the ten small launches of ``clip_grad_norm_`` were ~140 us of
    a 1.5 ms step (PPI-BP stand-in).  Same update rule (tests/test_gpu_float.py::test_clip_adam_matches_torch).
    ``lr_schedule``: ClipAdam's device learning-rate table (lr_find, schedule.lr_table); ``ema_decay`` / ``ema_warmup``: its
    weight average.  An optimizer that would stay torch's has neither and raises."""
    if lr_schedule is not None or ema_decay:
        out = _accelerate(optimizer, max_norm, capturable, big_bytes, lr_schedule, ema_decay, ema_warmup)
        if not isinstance(out, ClipAdam) or out is optimizer:
            raise ValueError('a learning-rate schedule on the device and a weight average (ema_decay) need a plain '
                             'torch.optim.Adam over float32, contiguous CUDA parameters on one device (what accelerate turns '
                             'into ClipAdam); configure_optimizers returned %s' % type(optimizer).__name__)
        return out
    return _accelerate(optimizer, max_norm, capturable, big_bytes, None)


def _accelerate(optimizer, max_norm, capturable, big_bytes, lr_schedule, ema_decay=0.0, ema_warmup=False):
    if isinstance(optimizer, ClipAdam):
        return optimizer
    if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1 or len(optimizer.state) != 0:
        return optimizer
    g = optimizer.param_groups[0]
    if g.get('weight_decay', 0) or g.get('amsgrad', False) or g.get('maximize', False) or g.get('differentiable', False):
        return optimizer
    params = [p for p in g['params'] if p.requires_grad]
    if not fusable(params) or torch.is_tensor(g['lr']):
        return optimizer
    return ClipAdam(params, g['lr'], max_norm=(max_norm if max_norm and max_norm > 0 else None), betas=g['betas'], eps=g['eps'],
                    big_bytes=big_bytes, capturable=capturable, lr_schedule=lr_schedule, ema_decay=ema_decay, ema_warmup=ema_warmup)

"""Class weights of the training loss: hparams['class_weight'] / hparams['pos_weight'] -> torch's ``weight`` / ``pos_weight`` of
the two loss modules the model builds (nn.CrossEntropyLoss / nn.BCEWithLogitsLoss, reference SubGNN.py:133), the shaped losses
(hparams['label_smoothing'] / hparams['focal_gamma'] -> ShapedLoss), and the decision which route a loss module takes through a
training step (the kernels of csrc/head.hip and csrc/loss.hip, or the library).
Host code only: nothing here touches a device."""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

KINDS = ('class_weight', 'pos_weight')


def class_counts(labels, K):
    """Rows per class of a split's labels -> (int64 array of K counts, number of rows).  ``labels``: an int64 tensor (N,) of
    class indices (single-label; -100 rows are not counted) or a list of N lists of class indices (multi-label: a row counts for
    each of its classes once)."""
    counts = np.zeros(int(K), dtype=np.int64)
    if isinstance(labels, (list, tuple)):
        for row in labels:
            for c in set(int(v) for v in row):
                if 0 <= c < K:
                    counts[c] += 1
        return counts, len(labels)
    y = torch.as_tensor(labels).reshape(-1).to(torch.int64).cpu().numpy()
    y = y[(y >= 0) & (y < K)]
    counts += np.bincount(y, minlength=int(K))[:int(K)]
    return counts, int(y.shape[0])


def balanced(kind, counts, N):
    """'balanced' weights from the training split's class counts n_k over N rows.  class_weight: N / (K n_k), which is
    sklearn.utils.class_weight.compute_class_weight('balanced'); pos_weight: (N - n_k) / n_k, negatives per positive.  A class
    without a training row gets 1.0 (its weight is never applied to a training row)."""
    K = len(counts)
    out = []
    for n in counts:
        n = int(n)
        if n == 0:
            out.append(1.0)
        elif kind == 'class_weight':
            out.append(float(N) / (K * n))
        else:
            out.append(float(N - n) / n)
    return out


def resolve(spec, kind, K, multilabel, labels=None, names=None):
    """hparams[kind] -> None or a list of K finite non-negative floats in class-index order.
    ``spec``: None; a list of K numbers; a dict {label string: number} (``names[k]`` is class k's label string, missing labels get
    1); or 'balanced' (from ``labels``, the training split's; see ``balanced``).  Raises ValueError for a wrong length, a
    negative or non-finite value, an unknown label string, pos_weight on a single-label model and 'balanced' as a multi-label
    class_weight (a per-column factor has no balanced form there: pos_weight is the tool)."""
    if kind not in KINDS:
        raise ValueError('unknown loss weight %r' % (kind,))
    if spec is None:
        return None
    K = int(K)
    if kind == 'pos_weight' and not multilabel:
        raise ValueError("hparams['pos_weight'] belongs to a multi-label dataset (nn.BCEWithLogitsLoss); use class_weight")
    if isinstance(spec, str):
        if spec != 'balanced':
            raise ValueError("hparams[%r] = %r: the only string form is 'balanced'" % (kind, spec))
        if kind == 'class_weight' and multilabel:
            raise ValueError("hparams['class_weight'] = 'balanced' has no meaning for a multi-label dataset; use pos_weight: 'balanced'")
        if labels is None:
            raise ValueError("hparams[%r] = 'balanced' needs the training split's labels" % kind)
        counts, N = class_counts(labels, K)
        values = balanced(kind, counts, N)
    elif isinstance(spec, dict):
        names = [str(k) for k in range(K)] if names is None else [str(n) for n in names]
        unknown = [k for k in spec if str(k) not in names]
        if unknown:
            raise ValueError('hparams[%r]: no class is labelled %s (labels: %s)' % (kind, unknown, names))
        by_name = {str(k): v for k, v in spec.items()}
        values = [by_name.get(names[k], 1.0) if k < len(names) else 1.0 for k in range(K)]
    elif isinstance(spec, (list, tuple)) or (hasattr(spec, 'tolist') and not isinstance(spec, (int, float))):
        values = list(spec.tolist() if hasattr(spec, 'tolist') else spec)
        if len(values) != K:
            raise ValueError('hparams[%r] has %d values for %d classes' % (kind, len(values), K))
    else:
        raise ValueError("hparams[%r] must be None, a list of %d numbers, a dict from label to number, or 'balanced'" % (kind, K))
    out = []
    for k, v in enumerate(values):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError('hparams[%r][%d] = %r is not a number' % (kind, k, v))
        v = float(v)
        if not math.isfinite(v) or v < 0:
            raise ValueError('hparams[%r][%d] = %r: weights must be finite and non-negative' % (kind, k, v))
        out.append(v)
    return out


def check_shape(label_smoothing, focal_gamma, multilabel, where='loss'):
    """(label_smoothing, focal_gamma) as two floats.  ValueError for a label_smoothing outside [0, 1), a negative or non-finite
    focal_gamma, both non-zero (no definition of a smoothed focal loss is torch's), or label smoothing of a multi-label loss
    (torch has none for BCE)."""
    out = []
    for name, v in (('label_smoothing', label_smoothing), ('focal_gamma', focal_gamma)):
        if v is None:
            v = 0.0
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError('%s: %s = %r is not a number' % (where, name, v))
        out.append(float(v))
    eps, gamma = out
    if not (0.0 <= eps < 1.0):
        raise ValueError('%s: label_smoothing = %r must lie in [0, 1)' % (where, eps))
    if not (math.isfinite(gamma) and gamma >= 0.0):
        raise ValueError('%s: focal_gamma = %r must be finite and non-negative' % (where, gamma))
    if eps != 0.0 and gamma != 0.0:
        raise ValueError('%s: label_smoothing and focal_gamma exclude each other' % where)
    if eps != 0.0 and multilabel:
        raise ValueError('%s: label_smoothing belongs to a single-label dataset (torch has none for BCE); use focal_gamma or pos_weight'
                         % where)
    return eps, gamma


class ShapedLoss(nn.Module):
    """Label smoothing or focal loss with per-class weights, mean reduction: the torch expression of what the shaped kernels of
    csrc/head.hip and csrc/loss.hip compute -- the validation loss, the library route and the tests' reference.
      single-label, label_smoothing eps   F.cross_entropy(logits, target, weight=weight, label_smoothing=eps)
      single-label, focal_gamma g         sum_i w[y_i] (1 - p_t)^g (-log p_t) / sum_i w[y_i] over the rows with y_i != -100 (p_t the
                                          softmax probability of the label; the class weights play alpha's role)
      multi-label, focal_gamma g          mean over B K of weight_k L (1 - p_t)^g (-log p_t), p_t = sigmoid(x) for a target and
                                          sigmoid(-x) otherwise, L = pos_weight_k for a target, else 1 (pos_weight is alpha)
    With both 0 it is the weighted nn.CrossEntropyLoss / nn.BCEWithLogitsLoss.  ``weight`` / ``pos_weight``: None or K numbers, kept
    as NON-persistent float32 buffers (no state_dict keys, as make_loss keeps them).  (1 - p_t)^g is formed from a clamped 1 - p_t
    and is exactly 0 where 1 - p_t is: loss and gradient are 0 and finite there, also for g < 1."""

    def __init__(self, multilabel, label_smoothing=0.0, focal_gamma=0.0, weight=None, pos_weight=None):
        super().__init__()
        self.multilabel = bool(multilabel)
        self.label_smoothing, self.focal_gamma = check_shape(label_smoothing, focal_gamma, self.multilabel, 'ShapedLoss')
        if pos_weight is not None and not self.multilabel:
            raise ValueError('ShapedLoss: pos_weight belongs to a multi-label loss')
        for name, w in (('weight', weight), ('pos_weight', pos_weight)):
            self.register_buffer(name, None if w is None else torch.as_tensor(w, dtype=torch.float32).detach().clone(), persistent=False)

    def extra_repr(self):
        return 'multilabel=%s, label_smoothing=%g, focal_gamma=%g' % (self.multilabel, self.label_smoothing, self.focal_gamma)

    @staticmethod
    def _qpow(q, gamma):
        """q^gamma for q in [0, 1] with a finite gradient: 0 (value and gradient) at q = 0."""
        return torch.where(q > 0, q.clamp_min(torch.finfo(q.dtype).tiny).pow(gamma), torch.zeros_like(q))

    def forward(self, logits, target):
        w = None if self.weight is None else self.weight.to(logits.dtype)
        if self.multilabel:
            pw = None if self.pos_weight is None else self.pos_weight.to(logits.dtype)
            t = target != 0
            if self.focal_gamma == 0.0:
                return F.binary_cross_entropy_with_logits(logits, t.to(logits.dtype), weight=w, pos_weight=pw)
            z = torch.where(t, logits, -logits)
            el = -F.logsigmoid(z) * self._qpow(torch.sigmoid(-z), self.focal_gamma)
            if pw is not None:
                el = el * torch.where(t, pw.expand_as(el), torch.ones_like(el))
            if w is not None:
                el = el * w
            return el.mean()
        if self.focal_gamma == 0.0:
            return F.cross_entropy(logits, target, weight=w, label_smoothing=self.label_smoothing)
        counted = target != -100
        y = torch.where(counted, target, torch.zeros_like(target))
        lp = F.log_softmax(logits, 1).gather(1, y.unsqueeze(1)).squeeze(1)
        wy = torch.ones_like(lp) if w is None else w[y]
        wy = torch.where(counted, wy, torch.zeros_like(wy))
        return (wy * self._qpow(-torch.expm1(lp), self.focal_gamma) * -lp).sum() / wy.sum()


def make_loss(multilabel, class_weight=None, pos_weight=None, label_smoothing=0.0, focal_gamma=0.0):
    """The model's loss module (reference SubGNN.py:133) carrying the weights as NON-persistent buffers: they follow the module
    across devices but are no state_dict keys -- a checkpoint has the same keys with and without weights, which are rebuilt from
    the hyper-parameters and the training split.  With label_smoothing or focal_gamma non-zero: a ShapedLoss carrying the same
    rows; with both 0 exactly the nn module this returned before."""
    eps, gamma = check_shape(label_smoothing, focal_gamma, multilabel, 'hparams')
    if eps != 0.0 or gamma != 0.0:
        return ShapedLoss(multilabel, eps, gamma, weight=class_weight, pos_weight=pos_weight)
    cw = None if class_weight is None else torch.tensor(class_weight, dtype=torch.float32)
    pw = None if pos_weight is None else torch.tensor(pos_weight, dtype=torch.float32)
    loss = nn.BCEWithLogitsLoss() if multilabel else nn.CrossEntropyLoss()
    for name, w in (('weight', cw), ('pos_weight', pw)):
        if w is not None:
            loss._buffers.pop(name, None)
            loss.register_buffer(name, w, persistent=False)
    return loss


def refuse_multi_rank(loss):
    """A model with loss weights under an initialised process group of more than one rank: the ranks' weighted means are averaged,
    which is not the weighted mean over all rows (each rank divides by its own sum of weights)."""
    import torch.distributed as dist
    if getattr(loss, 'weight', None) is None and getattr(loss, 'pos_weight', None) is None:
        return
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError('class_weight / pos_weight are not supported in multi-rank runs: every rank would divide by its own sum of '
                           'weights, and the average of those per-rank means is not the global weighted mean (world size %d)'
                           % dist.get_world_size())


def _row_ok(w, K, device):
    return (torch.is_tensor(w) and w.dtype == torch.float32 and w.dim() == 1 and w.shape[0] == int(K)
            and (device is None or w.device == torch.device(device)))


def kernel_plan(loss, multilabel, K, device=None):
    """Can the loss kernels compute what ``loss`` computes?  -> (weight, pos_weight) (either None: the bare launches take (None,
    None)) or None: the library path.  The kernels restate the mean reduction of nn.CrossEntropyLoss (ignore_index -100, no label
    smoothing) and nn.BCEWithLogitsLoss with per-class rows of K float32 weights (on ``device`` when given); a subclass, another
    reduction / ignore_index / label_smoothing or a weight of another shape or dtype is the library's."""
    if multilabel:
        if type(loss) is not nn.BCEWithLogitsLoss or loss.reduction != 'mean':
            return None
        w, pw = loss.weight, loss.pos_weight
    else:
        if type(loss) is not nn.CrossEntropyLoss or loss.reduction != 'mean' or loss.ignore_index != -100 \
                or float(getattr(loss, 'label_smoothing', 0.0)) != 0.0:
            return None
        w, pw = loss.weight, None
    for row in (w, pw):
        if row is not None and not _row_ok(row, K, device):
            return None
    return w, pw


def plan(loss, multilabel, K, device=None):
    """What the loss kernels take of ``loss`` -> (weight, pos_weight, label_smoothing, focal_gamma) or None: the library path.  A
    module whose type is exactly ShapedLoss (of this kind of dataset, its rows K float32 values on ``device``): its parameters;
    anything else: kernel_plan's answer with (0.0, 0.0) appended -- a hand-assigned nn.CrossEntropyLoss(label_smoothing=) stays
    the library's."""
    if type(loss) is ShapedLoss:
        if loss.multilabel != bool(multilabel):
            return None
        for row in (loss.weight, loss.pos_weight):
            if row is not None and not _row_ok(row, K, device):
                return None
        return loss.weight, loss.pos_weight, loss.label_smoothing, loss.focal_gamma
    kp = kernel_plan(loss, multilabel, K, device)
    return None if kp is None else kp + (0.0, 0.0)


def route(loss, hparams, multilabel, K, head_ok, device=None):
    """Which route a training step's loss takes: 'fused_head' (inside the head's launches, ops.fused_head), 'standalone' (one pass
    over the logits: ops.cross_entropy_with_accuracy / ops.bce_with_logits_and_accuracy -- a head the fused kernel does not take,
    or fused_head: false) or 'library' (the torch module itself).  ``head_ok``: ops.head_supported of the head's widths.  What
    SubGNN.training_step decides for device tensors of the expected shapes."""
    if plan(loss, multilabel, K, device) is None or not hparams.get('fused_forward', True):
        return 'library'
    if multilabel and not hparams.get('fused_multilabel_loss', True):
        return 'library'
    return 'fused_head' if (head_ok and hparams.get('fused_head', True)) else 'standalone'

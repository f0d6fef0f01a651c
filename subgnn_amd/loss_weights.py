"""Class weights of the training loss: hparams['class_weight'] / hparams['pos_weight'] -> torch's ``weight`` / ``pos_weight`` of
the two loss modules the model builds (nn.CrossEntropyLoss / nn.BCEWithLogitsLoss, reference SubGNN.py:133), and the decision
which route a loss module takes through a training step (the kernels of csrc/head.hip and csrc/loss.hip, or the library).
Host code only: nothing here touches a device."""
import math

import numpy as np
import torch
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


def make_loss(multilabel, class_weight=None, pos_weight=None):
    """The model's loss module (reference SubGNN.py:133) carrying the weights as NON-persistent buffers: they follow the module
    across devices but are no state_dict keys -- a checkpoint has the same keys with and without weights, which are rebuilt from
    the hyper-parameters and the training split."""
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


def route(loss, hparams, multilabel, K, head_ok, device=None):
    """Which route a training step's loss takes: 'fused_head' (inside the head's launches, ops.fused_head), 'standalone' (one pass
    over the logits: ops.cross_entropy_with_accuracy / ops.bce_with_logits_and_accuracy -- a head the fused kernel does not take,
    or fused_head: false) or 'library' (the torch module itself).  ``head_ok``: ops.head_supported of the head's widths.  What
    SubGNN.training_step decides for device tensors of the expected shapes."""
    if kernel_plan(loss, multilabel, K, device) is None or not hparams.get('fused_forward', True):
        return 'library'
    if multilabel and not hparams.get('fused_multilabel_loss', True):
        return 'library'
    return 'fused_head' if (head_ok and hparams.get('fused_head', True)) else 'standalone'

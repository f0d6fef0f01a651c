"""Shared by tests/test_weighted_loss_host.py and tests/test_gpu_weighted_loss.py: the shapes, the inputs and the float64 torch
references of the class-weighted loss kernels (csrc/head.hip headw_*, csrc/loss.hip *_weighted_kernel).  A case is computed once
per process and handed out unchanged."""
import functools

import torch
import torch.nn.functional as F

# (B, H0, H1, H2, K) of the fused head: the smallest; the 32-row chunk edge; odd widths; every limit (H <= 128, K <= 32); a
# workgroup that takes two chunks (HEAD_MAX_BLOCKS * 32 = 32768 rows)
HEAD_SHAPES = [(1, 7, 3, 2, 1), (31, 20, 16, 8, 2), (32, 20, 16, 8, 2), (33, 20, 16, 8, 2), (1000, 70, 100, 37, 5),
               (4133, 130, 128, 128, 32), (32801, 16, 8, 8, 3)]
# (B, K) of the stand-alone pairs: one row; the 256-row workgroup edge; K above the head's 32; many workgroups
PAIR_SHAPES = [(1, 1), (255, 3), (256, 3), (257, 40), (70001, 33)]
ML_MODES = ('pos_weight', 'weight', 'both')
NEW_ENTRIES = ('sgnn_cross_entropy_fwd_weighted', 'sgnn_cross_entropy_bwd_weighted', 'sgnn_bce_logits_fwd_weighted',
               'sgnn_bce_logits_bwd_weighted', 'sgnn_head_fwd_weighted', 'sgnn_head_bwd_weighted', 'sgnn_head_fwd_ml_weighted',
               'sgnn_head_bwd_ml_weighted')
WEIGHTED_KERNELS = ('headw_fwd_kernel', 'headw_fwd_ml_kernel', 'headw_bwd_kernel<1>', 'headw_bwd_kernel<2>', 'headw_bwd_kernel<4>',
                    'headw_bwd_ml_kernel<1>', 'headw_bwd_ml_kernel<2>', 'headw_bwd_ml_kernel<4>', 'ce_fwd_weighted_kernel',
                    'ce_bwd_weighted_kernel', 'bce_fwd_weighted_kernel', 'bce_bwd_weighted_kernel')


def head_modules(H0, H1, H2, K, seed):
    """Initialisation of tests/test_gpu_multilabel_head.py::_head_modules (activations and logits of order 1)."""
    g = torch.Generator().manual_seed(seed)
    mods = [torch.nn.Linear(H0, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, K)]
    for m in mods:
        m.weight.data = torch.randn(m.weight.shape, generator=g) / m.in_features ** 0.5
        m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.3
    return mods


def class_weights(K, g, zero=True):
    """K weights in [0.1, 10] (log-uniform), class K - 1 at weight 0 when there is a second class to carry the loss."""
    w = torch.exp(torch.empty(K).uniform_(-2.302585, 2.302585, generator=g)).float()
    if zero and K >= 2:
        w[K - 1] = 0.0
    return w


def labels_for(B, K, g):
    """int64 (B,) labels over all K classes; every seventh row from row 3 on ignored (-100) when there are rows to spare."""
    y = torch.randint(0, K, (B,), generator=g)
    if B >= 10:
        y[3::7] = -100
        y[0] = 0                                           # a counted row of a class with weight > 0: the denominator is not 0
    return y


def ml_weights(K, g, mode):
    """(weight, pos_weight) of a multi-label case: the rows ``mode`` names, the other None; one zero in each given row."""
    w = class_weights(K, g, zero=K >= 2) if mode in ('weight', 'both') else None
    pw = class_weights(K, g, zero=False) if mode in ('pos_weight', 'both') else None
    if pw is not None and K >= 2:
        pw[0] = 0.0
    return w, pw


def head_forward_ref(mods64, x64):
    return mods64[2](F.relu(mods64[1](F.relu(mods64[0](x64)))))


RELU_MARGIN = 1e-5


def away_from_the_relu_kinks(x, shape, g):
    """Redraw the rows of ``x`` in which a pre-activation of either hidden layer lies within RELU_MARGIN of 0.  relu's derivative
    jumps there: a float32 sum of up to 130 products of order-1 values carries a rounding error of about 1e-6, so a float32
    forward can take the other branch than the float64 reference and that row's gradients then differ by a whole term -- a property
    of the reference's kink, not an error of either side (first draw of the (4133, 130, 128, 128, 32) case: z2[374, 111] =
    2.5e-8, grad x off by 1.5 % of its largest element in that one row).  About one row in 500 is redrawn."""
    B, H0, H1, H2, K = shape
    mods = [m.double() for m in head_modules(H0, H1, H2, K, 3)]
    with torch.no_grad():
        for _ in range(100):
            z1 = mods[0](x.double())
            z2 = mods[1](F.relu(z1))
            bad = (z1.abs().min(1).values < RELU_MARGIN) | (z2.abs().min(1).values < RELU_MARGIN)
            if not bool(bad.any()):
                return x
            x[bad] = torch.randn(int(bad.sum()), H0, generator=g)
    raise AssertionError('no draw of the inputs keeps clear of the relu kinks')


@functools.lru_cache(maxsize=None)
def head_case(shape, mode=None):
    """The inputs and the float64 CPU reference of one fused-head case.  mode None: single-label (F.cross_entropy(weight=));
    else multi-label (F.binary_cross_entropy_with_logits(weight=, pos_weight=)).  -> dict of CPU tensors: x, y, w, pw, go (a
    gradient for the logits), and ref / ref2 = {logits, loss, grads} for loss.backward() and (loss + (logits go).sum())
    .backward(); grads = [x, lin.weight, lin.bias, lin2.weight, ...]."""
    B, H0, H1, H2, K = shape
    g = torch.Generator().manual_seed(1000 * B + H0 + (0 if mode is None else 1 + ML_MODES.index(mode)))
    x = torch.randn(B, H0, generator=g)
    if mode is None:
        y, w, pw = labels_for(B, K, g), class_weights(K, g), None
    else:
        y = (torch.rand(B, K, generator=g) < 0.35).long()
        if B > 10:
            y[3, 0] = 7                                    # a non-zero target counts as 1
        w, pw = ml_weights(K, g, mode)
    go = torch.randn(B, K, generator=g)
    x = away_from_the_relu_kinks(x, shape, g)
    out = {'x': x, 'y': y, 'w': w, 'pw': pw, 'go': go}
    for key, through_logits in (('ref', False), ('ref2', True)):
        mods = [m.double() for m in head_modules(H0, H1, H2, K, 3)]
        xr = x.double().requires_grad_(True)
        lg = head_forward_ref(mods, xr)
        if mode is None:
            loss = F.cross_entropy(lg, y, weight=w.double())
        else:
            loss = F.binary_cross_entropy_with_logits(lg, (y != 0).double(), weight=None if w is None else w.double(),
                                                      pos_weight=None if pw is None else pw.double())
        (loss + (lg * go.double()).sum() if through_logits else loss).backward()
        grads = [xr.grad] + [p.grad for m in mods for p in (m.weight, m.bias)]
        out[key] = {'logits': lg.detach(), 'loss': float(loss.detach()), 'grads': grads}
    return out


GRAD_NAMES = ('x', 'lin.weight', 'lin.bias', 'lin2.weight', 'lin2.bias', 'lin3.weight', 'lin3.bias')


@functools.lru_cache(maxsize=None)
def pair_case(shape, mode=None):
    """One stand-alone case: logits x (B, K) of spread 3, labels / targets, weights, the float64 loss and gradient of
    1.5 * loss."""
    B, K = shape
    g = torch.Generator().manual_seed(77 * B + K + (0 if mode is None else 1 + ML_MODES.index(mode)))
    x = torch.randn(B, K, generator=g) * 3
    if mode is None:
        y, w, pw = labels_for(B, K, g), class_weights(K, g), None
    else:
        y = (torch.rand(B, K, generator=g) < 0.4).long()
        if B > 10:
            y[5, 0] = -3                                   # non-zero: 1
        w, pw = ml_weights(K, g, mode)
    xr = x.double().requires_grad_(True)
    if mode is None:
        loss = F.cross_entropy(xr, y, weight=w.double())
    else:
        loss = F.binary_cross_entropy_with_logits(xr, (y != 0).double(), weight=None if w is None else w.double(),
                                                  pos_weight=None if pw is None else pw.double())
    (loss * 1.5).backward()
    return {'x': x, 'y': y, 'w': w, 'pw': pw, 'loss': float(loss.detach()), 'grad': xr.grad}


# the gate of SubGNN.training_step restated (subgnn_amd/loss_weights.route): (what, loss module factory, hparams, multilabel,
# head supported, expected route)
def route_cases():
    from torch import nn
    w3, w4 = torch.tensor([1.0, 2.0, 0.5]), torch.tensor([1.0, 2.0, 0.5, 3.0])
    return [
        ('bare CE, fused head', lambda: nn.CrossEntropyLoss(), {}, False, True, 'fused_head'),
        ('weighted CE, fused head', lambda: nn.CrossEntropyLoss(weight=w3), {}, False, True, 'fused_head'),
        ('weighted CE, head too wide', lambda: nn.CrossEntropyLoss(weight=w3), {}, False, False, 'standalone'),
        ('weighted CE, fused_head: false', lambda: nn.CrossEntropyLoss(weight=w3), {'fused_head': False}, False, True, 'standalone'),
        ('weighted CE, fused_forward: false', lambda: nn.CrossEntropyLoss(weight=w3), {'fused_forward': False}, False, True, 'library'),
        ('CE reduction=sum', lambda: nn.CrossEntropyLoss(weight=w3, reduction='sum'), {}, False, True, 'library'),
        ('CE ignore_index=0', lambda: nn.CrossEntropyLoss(ignore_index=0), {}, False, True, 'library'),
        ('CE label_smoothing=0.1', lambda: nn.CrossEntropyLoss(weight=w3, label_smoothing=0.1), {}, False, True, 'library'),
        ('CE weight of another length', lambda: nn.CrossEntropyLoss(weight=w4), {}, False, True, 'library'),
        ('CE weight in float64', lambda: nn.CrossEntropyLoss(weight=w3.double()), {}, False, True, 'library'),
        ('a subclass', lambda: type('MyLoss', (nn.CrossEntropyLoss,), {})(), {}, False, True, 'library'),
        ('bare BCE, fused head', lambda: nn.BCEWithLogitsLoss(), {}, True, True, 'fused_head'),
        ('BCE pos_weight, fused head', lambda: nn.BCEWithLogitsLoss(pos_weight=w3), {}, True, True, 'fused_head'),
        ('BCE weight + pos_weight, K > 32', lambda: nn.BCEWithLogitsLoss(weight=w3, pos_weight=w3), {}, True, False, 'standalone'),
        ('BCE pos_weight, fused_multilabel_loss: false', lambda: nn.BCEWithLogitsLoss(pos_weight=w3), {'fused_multilabel_loss': False},
         True, True, 'library'),
        ('BCE reduction=none', lambda: nn.BCEWithLogitsLoss(pos_weight=w3, reduction='none'), {}, True, True, 'library'),
        ('BCE element weight (B, K)', lambda: nn.BCEWithLogitsLoss(weight=torch.ones(2, 3)), {}, True, True, 'library'),
    ]

"""Shared by tests/test_shaped_loss_host.py and tests/test_gpu_shaped_loss.py: the shapes, the inputs and the float64 references of
the shaped loss kernels (label smoothing and focal loss, DESIGN 8p: csrc/head.hip heads_*, csrc/loss.hip *_shaped_kernel /
*_focal_kernel).  References are loss_weights.ShapedLoss in float64 on the CPU; ``numpy_loss_and_grad`` restates the closed forms
in numpy (the host test holds the two against each other on these very cases, constructed rows included).  A case is computed once
per process and handed out unchanged.

What every case carries when it has the rows and classes for it (B >= 31; K >= 2 for a zero weight and a trailing label): rows
ignored with -100 (single-label), one class of weight 0 (and one zero in pos_weight), and four CONSTRUCTED rows, the last four of the
batch, whose target logit leads by >= 40, trails by >= 40, leads by >= 100 and trails by >= 100 (q = 0 in float32, q = 1, exp
underflow).  The one-row shapes can have none of these; with K = 1 a single-label row has q = 0 by itself."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from weighted_loss_cases import (HEAD_SHAPES, PAIR_SHAPES, GRAD_NAMES, RELU_MARGIN, head_modules, labels_for, class_weights, ml_weights,
                                 away_from_the_relu_kinks, head_forward_ref)

# (name, multilabel, label_smoothing, focal_gamma): the modes every shape runs in ...
MODES = [('smooth', False, 0.1, 0.0), ('focal', False, 0.0, 2.0), ('focal_ml', True, 0.0, 2.0)]
# ... and those of the (33, ...) head shape and the (257, 40) pair only
EXTRA_SHAPE, EXTRA_PAIR = (33, 20, 16, 8, 2), (257, 40)
EXTRA_MODES = [('smooth', False, 0.9, 0.0)] + [(nm, ml, 0.0, g) for g in (0.5, 1.0, 5.0) for nm, ml in (('focal', False), ('focal_ml', True))]
LEADS = (40.0, -40.0, 100.0, -100.0)                       # the constructed rows B - 4 .. B - 1: lead (+) or trail (-) by at least |v|
NEW_ENTRIES = ('sgnn_cross_entropy_fwd_shaped', 'sgnn_cross_entropy_bwd_shaped', 'sgnn_bce_logits_fwd_shaped',
               'sgnn_bce_logits_bwd_shaped', 'sgnn_head_fwd_shaped', 'sgnn_head_bwd_shaped', 'sgnn_head_fwd_ml_shaped',
               'sgnn_head_bwd_ml_shaped')
SHAPED_KERNELS = ['heads_fwd_kernel<%s>' % m for m in ('0, 1', '0, 2', '1, 2')] \
    + ['heads_bwd_kernel<%d, %s>' % (nb, m) for m in ('0, 1', '0, 2', '1, 2') for nb in (1, 2, 4)] \
    + ['ce_fwd_shaped_kernel<1>', 'ce_fwd_shaped_kernel<2>', 'ce_bwd_shaped_kernel<1>', 'ce_bwd_shaped_kernel<2>',
       'bce_fwd_focal_kernel', 'bce_bwd_focal_kernel']


def shaped_loss(ml, eps, gamma, w, pw):
    """The reference module in float64 arithmetic (its float32 rows are cast to the logits' dtype in forward)."""
    from subgnn_amd.loss_weights import ShapedLoss
    return ShapedLoss(ml, eps, gamma, weight=w, pos_weight=pw)


# ---- the closed forms of the issue, in numpy float64 ----------------------------------------------------------------------------------

def numpy_loss_and_grad(x, y, w, pw, ml, eps, gamma, g=1.0):
    """(loss, d loss / d logits * g) from the stated formulas.  x (B, K) float64; y int64 (B,) labels or (B, K) targets; w / pw:
    K weights or None."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y)
    B, K = x.shape
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    if ml:
        t = y != 0
        L = np.where(t, np.ones(K) if pw is None else np.asarray(pw, dtype=np.float64), 1.0)
        s = np.where(t, 1.0, -1.0)
        z = s * x
        e = np.exp(-np.abs(z))
        ell = np.log1p(e) + np.maximum(-z, 0.0)
        q = np.where(z >= 0, e / (1 + e), 1 / (1 + e))
        pt = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
        qg = np.where(q > 0, np.power(np.maximum(q, 1e-300), gamma), 0.0)
        loss = (w * L * qg * ell).sum() / (B * K)
        return loss, -s * w * L * qg * (q + gamma * pt * ell) * g / (B * K)
    counted = y != -100
    yy = np.where(counted, y, 0)
    m = x.max(1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(1, keepdims=True)))[:, 0]
    p = np.exp(x - lse[:, None])
    delta = np.zeros_like(x)
    delta[np.arange(B), yy] = 1.0
    wy = np.where(counted, w[yy], 0.0)
    D = wy.sum()
    xy = x[np.arange(B), yy]
    if gamma == 0.0:
        W = w.sum()
        rows = (1 - eps) * wy * (lse - xy) + (eps / K) * counted * (w[None, :] * (lse[:, None] - x)).sum(1)
        grad = ((1 - eps) * wy[:, None] * (p - delta) + (eps / K) * counted[:, None] * (W * p - w[None, :])) * g / D
        return rows.sum() / D, grad
    lp = xy - lse
    pt, q = np.exp(lp), -np.expm1(lp)
    pos = q > 0
    qs = np.where(pos, q, 1.0)
    qg = np.where(pos, np.power(qs, gamma), 0.0)
    f = np.where(pos, qg - gamma * pt * np.power(qs, gamma - 1) * lp, 0.0)
    return (wy * qg * -lp).sum() / D, wy[:, None] * f[:, None] * (p - delta) * g / D


# ---- constructed rows -----------------------------------------------------------------------------------------------------------------

def _extreme_row(mods, H0, g, accept):
    """A row of x whose float64 logits through ``mods`` satisfy ``accept(logits) -> value or None``: random directions at growing
    scales; of 48 directions the accepted one with the smallest largest logit (float32 logits of magnitude 1000 would carry 1e-4
    of rounding into exp)."""
    best = None
    with torch.no_grad():
        for _ in range(48):
            d = torch.randn(H0, generator=g)
            for j in range(1, 13):
                row = d * float(2 ** j)
                lg = head_forward_ref(mods, row.double().unsqueeze(0))[0]
                got = accept(lg)
                if got is not None:
                    if best is None or float(lg.abs().max()) < best[0]:
                        best = (float(lg.abs().max()), row, got)
                    break
    assert best is not None, 'no direction gives the constructed row'
    return best[1], best[2]


def _accept_single(w, lead):
    pos = w > 0

    def accept(lg):
        K = lg.shape[0]
        if lead > 0:
            y = int(lg.argmax())
            others = torch.cat((lg[:y], lg[y + 1:]))
            return y if (bool(pos[y]) and float(lg[y] - others.max()) >= lead) else None
        y = int(torch.where(pos, lg, torch.full_like(lg, float('inf'))).argmin())
        return y if float(lg.max() - lg[y]) >= -lead and K >= 2 else None
    return accept


def _accept_multi(w, pw, lead):
    def accept(lg):
        for c in torch.argsort(lg.abs(), descending=True).tolist():
            if float(lg[c].abs()) < abs(lead):
                return None
            t = int((float(lg[c]) > 0) == (lead > 0))             # the target that makes z = s x lead (+) or trail (-)
            if float(w[c]) > 0 and (t == 0 or float(pw[c]) > 0):  # (an element whose factors are not zero)
                return c, t
        return None
    return accept


@functools.lru_cache(maxsize=None)
def head_case(shape, mode):
    """One fused-head case of ``mode`` = (name, multilabel, eps, gamma).  -> dict of CPU tensors: x, y, w, pw, go (a gradient for
    the logits), extreme (the constructed rows' indices), and ref / ref2 = {logits, loss, grads} for loss.backward() and (loss +
    (logits go).sum()).backward(); grads = [x, lin.weight, lin.bias, lin2.weight, ...]."""
    name, ml, eps, gamma = mode
    B, H0, H1, H2, K = shape
    g = torch.Generator().manual_seed(1000 * B + H0 + 17 * (1 + ['smooth', 'focal', 'focal_ml'].index(name)) + int(100 * (eps + gamma)))
    x = torch.randn(B, H0, generator=g)
    if ml:
        y = (torch.rand(B, K, generator=g) < 0.35).long()
        if B > 10:
            y[3, 0] = 7                                    # a non-zero target counts as 1
        w, pw = ml_weights(K, g, 'both')
    else:
        y, w, pw = labels_for(B, K, g), class_weights(K, g), None
    go = torch.randn(B, K, generator=g)
    x = away_from_the_relu_kinks(x, shape, g)
    extreme = []
    mods = [m.double() for m in head_modules(H0, H1, H2, K, 3)]
    if B >= 31 and (ml or K >= 2):
        for r, lead in zip(range(B - 4, B), LEADS):
            if ml:
                x[r], (c, t) = _extreme_row(mods, H0, g, _accept_multi(w, pw, lead))
                y[r, c] = t
            else:
                x[r], y[r] = _extreme_row(mods, H0, g, _accept_single(w, lead))
            extreme.append(r)
        with torch.no_grad():
            z1 = mods[0](x[extreme].double())
            z2 = mods[1](F.relu(z1))
            assert float(z1.abs().min()) >= RELU_MARGIN and float(z2.abs().min()) >= RELU_MARGIN
    out = {'x': x, 'y': y, 'w': w, 'pw': pw, 'go': go, 'extreme': extreme}
    loss_fn = shaped_loss(ml, eps, gamma, w, pw)
    for key, through_logits in (('ref', False), ('ref2', True)):
        mods = [m.double() for m in head_modules(H0, H1, H2, K, 3)]
        xr = x.double().requires_grad_(True)
        lg = head_forward_ref(mods, xr)
        loss = loss_fn(lg, y)
        (loss + (lg * go.double()).sum() if through_logits else loss).backward()
        grads = [xr.grad] + [p.grad for m in mods for p in (m.weight, m.bias)]
        out[key] = {'logits': lg.detach(), 'loss': float(loss.detach()), 'grads': grads}
    return out


@functools.lru_cache(maxsize=None)
def pair_case(shape, mode):
    """One stand-alone case: logits x (B, K) of spread 3 with the constructed rows set directly, labels / targets, weights, the
    float64 loss and the gradient of 1.5 * loss."""
    name, ml, eps, gamma = mode
    B, K = shape
    g = torch.Generator().manual_seed(77 * B + K + 17 * (1 + ['smooth', 'focal', 'focal_ml'].index(name)) + int(100 * (eps + gamma)))
    x = torch.randn(B, K, generator=g) * 3
    extreme = []
    if ml:
        y = (torch.rand(B, K, generator=g) < 0.4).long()
        if B > 10:
            y[5, 0] = -3                                   # non-zero: 1
        w, pw = ml_weights(K, g, 'both')
        if B >= 31:
            for r, lead in zip(range(B - 4, B), LEADS):    # every column of the row at +-|lead|, targets alternating: z = +-|lead|
                x[r] = lead
                y[r] = torch.arange(K) % 2
                extreme.append(r)
    else:
        y, w, pw = labels_for(B, K, g), class_weights(K, g), None
        if B >= 31 and K >= 2:
            for r, lead in zip(range(B - 4, B), LEADS):
                y[r] = (r * 7) % (K - 1)                   # (class K - 1 has weight 0)
                others = torch.cat((x[r, :int(y[r])], x[r, int(y[r]) + 1:]))
                x[r, int(y[r])] = float(others.max()) + lead
                extreme.append(r)
    xr = x.double().requires_grad_(True)
    loss = shaped_loss(ml, eps, gamma, w, pw)(xr, y)
    (loss * 1.5).backward()
    return {'x': x, 'y': y, 'w': w, 'pw': pw, 'loss': float(loss.detach()), 'grad': xr.grad, 'extreme': extreme}


def all_head_cases():
    return [(s, m) for s in HEAD_SHAPES for m in MODES] + [(EXTRA_SHAPE, m) for m in EXTRA_MODES]


def all_pair_cases():
    return [(s, m) for s in PAIR_SHAPES for m in MODES] + [(EXTRA_PAIR, m) for m in EXTRA_MODES]


def case_id(c):
    shape, (name, ml, eps, gamma) = c
    return '%s-%s-%g' % ('x'.join(str(v) for v in shape), name, eps or gamma)

"""-m gpu: class-weighted losses -- the weighted launches of the fused head (csrc/head.hip: headw_fwd_kernel,
headw_fwd_ml_kernel, headw_bwd_kernel<NB>, headw_bwd_ml_kernel<NB>), the weighted stand-alone pairs (csrc/loss.hip) and the
model path that uses them (hparams['class_weight'] / ['pos_weight'], SubGNN.training_step) against float64 torch on the CPU:
F.cross_entropy(weight=) and F.binary_cross_entropy_with_logits(weight=, pos_weight=).  Tolerances are those of
tests/test_gpu_multilabel_head.py for the same kernels: logits assert_close's default, loss 1e-5 max(1, |ref|), gradients
assert_close(norm_tol=2e-5)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, write_dataset_from_golden
import weighted_loss_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 16                                                 # guard floats on either side of a raw call's buffer
SENTINEL = -777.25


def _ops():
    from subgnn_amd import ops
    return ops


def _dev(t):
    return None if t is None else t.to(DEV)


def _loss_close(got, ref):
    assert abs(float(got) - ref) <= 1e-5 * max(1.0, abs(ref)), (float(got), ref)


def _mods(shape):
    B, H0, H1, H2, K = shape
    return [m.to(DEV) for m in C.head_modules(H0, H1, H2, K, 3)]


def _head(shape, mode, x, mods, case, **kw):
    """ops.fused_head of one case, single-label (mode None) or multi-label."""
    ops = _ops()
    if mode is None:
        return ops.fused_head(x, mods[0], mods[1], mods[2], _dev(case['y']), 0.0, None, class_weight=_dev(case['w']), **kw)
    return ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.0, None, targets=_dev(case['y']), class_weight=_dev(case['w']),
                          pos_weight=_dev(case['pw']), **kw)


def _check_head_case(shape, mode):
    """Values, every gradient, the loss through loss + logits, the call twice bit-identical."""
    B, H0, H1, H2, K = shape
    case = C.head_case(shape, mode)
    mods = _mods(shape)
    params = [p for m in mods for p in (m.weight, m.bias)]
    xg = case['x'].to(DEV).requires_grad_(True)
    lg, loss, acc = _head(shape, mode, xg, mods, case)
    loss.backward()
    ref = case['ref']
    assert_close(lg.detach(), ref['logits'], 'logits')
    print('%s %s: loss %.9g ref %.9g' % (shape, mode, float(loss.detach()), ref['loss']))
    _loss_close(loss.detach(), ref['loss'])
    # the accuracy is unweighted, over all B rows (an ignored row never counts as a hit): the hit count exactly, from the
    # kernel's own logits on the device
    y = case['y'].to(DEV)
    if mode is None:
        hits = int(((lg.detach().argmax(1) == y) & (y >= 0)).sum())
    else:
        hits = int(((torch.sigmoid(lg.detach()) > 0.5) == (y != 0)).all(1).sum())
    assert acc.shape == (1,) and round(float(acc) * B) == hits, (float(acc) * B, hits)
    assert float(acc) == float(torch.tensor(float(hits), dtype=torch.float32) / B)
    for got, want, nm in zip([xg.grad] + [p.grad for p in params], ref['grads'], C.GRAD_NAMES):
        assert_close(got, want, 'grad ' + nm, norm_tol=2e-5)
    # twice the same call: bit-identical (fixed summation orders, the ticket leaves its counter at zero)
    lg3, loss3, acc3 = _head(shape, mode, case['x'].to(DEV), mods, case)
    assert torch.equal(lg3, lg.detach()) and torch.equal(loss3, loss.detach()) and torch.equal(acc3, acc)
    # a gradient that arrives through the logits as well as the loss
    for p in params:
        p.grad = None
    xg2 = case['x'].to(DEV).requires_grad_(True)
    lg2, loss2, _ = _head(shape, mode, xg2, mods, case)
    (loss2 + (lg2 * case['go'].to(DEV)).sum()).backward()
    for got, want, nm in zip([xg2.grad] + [p.grad for p in params], case['ref2']['grads'], C.GRAD_NAMES):
        assert_close(got, want, 'grad %s through loss + logits' % nm, norm_tol=2e-5)


@pytest.mark.parametrize('shape', C.HEAD_SHAPES)
def test_weighted_head_single_label_matches_torch(shape):
    """ops.fused_head(labels, class_weight=) == the head + F.cross_entropy(weight=) of float64 torch: weights in [0.1, 10], one
    class at weight 0 (K >= 2), every seventh row ignored (B >= 10; a one-row, one-class case can have neither without a
    denominator of 0, which test_edge_rows covers)."""
    _check_head_case(shape, None)


@pytest.mark.parametrize('mode', C.ML_MODES)
@pytest.mark.parametrize('shape', C.HEAD_SHAPES)
def test_weighted_head_multi_label_matches_torch(shape, mode):
    """ops.fused_head(targets=, class_weight=, pos_weight=) == the head + F.binary_cross_entropy_with_logits(weight=,
    pos_weight=) of float64 torch, with pos_weight only, weight only and both (a zero in each given row when K >= 2)."""
    _check_head_case(shape, mode)


# ---- raw entries: guarded buffers -----------------------------------------------------------------------------------------------------

class Guarded:
    """A device buffer of n elements between two runs of GUARD sentinel elements."""

    def __init__(self, n, dtype=torch.float32, fill=None):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL if dtype == torch.float32 else -77, dtype=dtype, device=DEV)
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill, dtype=dtype).reshape(-1))

    @property
    def t(self):
        return self.buf[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        s = SENTINEL if self.buf.dtype == torch.float32 else -77
        return bool((self.buf[:GUARD] == s).all()) and bool((self.buf[GUARD + self.n:] == s).all())


def _raw_head(shape, z1, mods, labels, w, p=0.0, rng=None, weighted_entry=True, g_loss=1.0):
    """sgnn_head_fwd[_weighted] + sgnn_head_bwd[_weighted] on guarded buffers -> dict of Guarded (a1, a2, logits, lse, out, dz1,
    partial, w)."""
    from subgnn_amd import _lib
    ops = _ops()
    lib = _lib.load()
    B, H0, H1, H2, K = shape
    b = {'a1': Guarded(B * H1), 'a2': Guarded(B * H2), 'logits': Guarded(B * K), 'lse': Guarded(B + 1), 'out': Guarded(3),
         'dz1': Guarded(B * H1), 'w': None if w is None else Guarded(K, fill=w)}
    ws = ops._head_workspace(torch.device(DEV), B)
    st = ops._stream()
    P, nb = int(lib.sgnn_head_partial_floats(H1, H2, K)), int(lib.sgnn_head_blocks(B))
    b['partial'] = Guarded(nb * P)
    W2, b2, W3, b3 = (t.detach().contiguous() for t in (mods[1].weight, mods[1].bias, mods[2].weight, mods[2].bias))
    head = (ops._ptr(z1), B, H1, H2, K, ops._ptr(W2), ops._ptr(b2), ops._ptr(W3), ops._ptr(b3), ops._ptr(labels), float(p), ops._ptr(rng),
            b['a1'].ptr, b['a2'].ptr, b['logits'].ptr, b['lse'].ptr, b['out'].ptr, ops._ptr(ws), ws.numel() * 4, st)
    wp = None if w is None else b['w'].ptr
    rc = lib.sgnn_head_fwd_weighted(*head, wp) if weighted_entry else lib.sgnn_head_fwd(*head)
    assert rc == 0, rc
    g = torch.tensor([g_loss], dtype=torch.float32, device=DEV)
    rows = ctypes.c_void_p(b['out'].t.data_ptr() + 8)
    tail = (b['logits'].ptr, b['lse'].ptr, ops._ptr(labels), ops._ptr(g), None, rows, b['a1'].ptr, b['a2'].ptr, ops._ptr(W2), ops._ptr(W3),
            B, H1, H2, K, float(p), b['dz1'].ptr, b['partial'].ptr, st)
    rc = lib.sgnn_head_bwd_weighted(*tail, wp) if weighted_entry else lib.sgnn_head_bwd(*tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return b


def _raw_inputs(shape, seed=9):
    B, H0, H1, H2, K = shape
    g = torch.Generator().manual_seed(seed)
    mods = _mods(shape)
    x = torch.randn(B, H0, generator=g).to(DEV)
    z1 = torch.addmm(mods[0].bias.detach(), x, mods[0].weight.detach().t()).contiguous()
    return g, mods, z1


SMALL = (70, 9, 12, 6, 4)                                  # three chunks of 32 rows, the last one short


def test_edge_rows():
    """Every row ignored -> NaN (0 / 0, as torch); every counted row in a class of weight 0 -> NaN, as torch; a label outside
    [0, K) other than -100 (K and -1) -> NaN, with the guard words around the weight row and every output intact (w[y] is not
    read for it: the row is K floats between sentinels)."""
    ops = _ops()
    B, H0, H1, H2, K = SMALL
    g, mods, z1 = _raw_inputs(SMALL)
    x = torch.randn(B, H0, generator=g).to(DEV)
    w = torch.tensor([2.0, 0.0, 0.5, 3.0])
    ignored = torch.full((B,), -100, dtype=torch.int64)
    _, loss, acc = ops.fused_head(x, mods[0], mods[1], mods[2], ignored.to(DEV), 0.0, None, class_weight=w.to(DEV))
    assert torch.isnan(loss) and float(acc) == 0.0
    assert torch.isnan(F.cross_entropy(torch.zeros(B, K), ignored, weight=w))
    zero_class = ignored.clone()
    zero_class[::3] = 1                                      # the only counted rows are of class 1: weight 0
    xg = x.clone().requires_grad_(True)
    _, loss, _ = ops.fused_head(xg, mods[0], mods[1], mods[2], zero_class.to(DEV), 0.0, None, class_weight=w.to(DEV))
    assert torch.isnan(loss)
    assert torch.isnan(F.cross_entropy(torch.randn(B, K, generator=g), zero_class, weight=w))
    for bad in (K, -1):
        y = torch.randint(0, K, (B,), generator=g)
        y[40] = bad
        b = _raw_head(SMALL, z1, mods, y.to(DEV), w)
        assert torch.isnan(b['out'].t[0]), (bad, b['out'].t)
        for name, buf in b.items():
            assert buf.intact(), (bad, name)
        assert torch.equal(b['w'].t.cpu(), w)
        # the rows of good labels still have their gradient structure: finite logits and activations everywhere
        assert torch.isfinite(b['logits'].t).all() and torch.isfinite(b['a1'].t).all()
    # the stand-alone pair: the same three
    xs = torch.randn(B, K, generator=g).to(DEV)
    assert torch.isnan(ops.cross_entropy_with_accuracy(xs, ignored.to(DEV), weight=w.to(DEV))[0])
    assert torch.isnan(ops.cross_entropy_with_accuracy(xs, zero_class.to(DEV), weight=w.to(DEV))[0])
    y = torch.randint(0, K, (B,), generator=g)
    y[40] = K
    assert torch.isnan(ops.cross_entropy_with_accuracy(xs, y.to(DEV), weight=w.to(DEV))[0])


def test_identity_with_the_bare_launches():
    """class_weight = None through the new entry IS the existing entry (bit for bit, forward and backward); class weights of
    1.0 give the bare result bit for bit too (multiplying by 1.0 and summing ones are exact) -- fused head and stand-alone pair,
    loss, logits and every gradient."""
    ops = _ops()
    B, H0, H1, H2, K = SMALL
    g, mods, z1 = _raw_inputs(SMALL)
    y = C.labels_for(B, K, g).to(DEV)
    bare = _raw_head(SMALL, z1, mods, y, None, weighted_entry=False)
    null = _raw_head(SMALL, z1, mods, y, None, weighted_entry=True)
    ones = _raw_head(SMALL, z1, mods, y, torch.ones(K), weighted_entry=True)
    for name in ('a1', 'a2', 'logits', 'lse', 'out', 'dz1', 'partial'):
        assert torch.equal(bare[name].t, null[name].t), name
        assert torch.equal(bare[name].t, ones[name].t), name
        assert bare[name].intact() and null[name].intact() and ones[name].intact(), name
    assert float(bare['out'].t[2]) == float((y >= 0).sum()) == float(bare['lse'].t[B])
    # through ops, with autograd
    x = torch.randn(B, H0, generator=g).to(DEV)
    res = []
    for w in (None, torch.ones(K, device=DEV)):
        for m in mods:
            m.zero_grad()
        xg = x.clone().requires_grad_(True)
        lg, loss, acc = ops.fused_head(xg, mods[0], mods[1], mods[2], y, 0.0, None, class_weight=w)
        loss.backward()
        res.append([lg.detach(), loss.detach(), acc, xg.grad] + [p.grad.clone() for m in mods for p in (m.weight, m.bias)])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    xs = torch.randn(B, K, generator=g).to(DEV)
    res = []
    for w in (None, torch.ones(K, device=DEV)):
        xg = xs.clone().requires_grad_(True)
        loss, acc = ops.cross_entropy_with_accuracy(xg, y, weight=w)
        (loss * 1.5).backward()
        res.append((loss.detach(), acc, xg.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # multi-label: None / None through the new keywords is the existing launch
    t = (torch.rand(B, K, generator=g) < 0.4).long().to(DEV)
    a = ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.0, None, targets=t)
    b = ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.0, None, targets=t, class_weight=None, pos_weight=None)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    a = ops.bce_with_logits_and_accuracy(xs, t)
    b = ops.bce_with_logits_and_accuracy(xs, t, weight=None, pos_weight=None)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_multi_label_null_rows_through_the_raw_entry_are_the_bare_launch():
    from subgnn_amd import _lib
    ops = _ops()
    lib = _lib.load()
    B, H0, H1, H2, K = SMALL
    g, mods, z1 = _raw_inputs(SMALL)
    t = (torch.rand(B, K, generator=g) < 0.4).long().to(DEV)
    W2, b2, W3, b3 = (p.detach().contiguous() for p in (mods[1].weight, mods[1].bias, mods[2].weight, mods[2].bias))
    ws = ops._head_workspace(torch.device(DEV), B)
    P, nb = int(lib.sgnn_head_partial_floats(H1, H2, K)), int(lib.sgnn_head_blocks(B))
    got = []
    for weighted in (False, True):
        b = {'a1': Guarded(B * H1), 'a2': Guarded(B * H2), 'logits': Guarded(B * K), 'out': Guarded(3), 'dz1': Guarded(B * H1),
             'partial': Guarded(nb * P)}
        head = (ops._ptr(z1), B, H1, H2, K, ops._ptr(W2), ops._ptr(b2), ops._ptr(W3), ops._ptr(b3), ops._ptr(t), 0.0, None, b['a1'].ptr,
                b['a2'].ptr, b['logits'].ptr, b['out'].ptr, ops._ptr(ws), ws.numel() * 4, ops._stream())
        assert (lib.sgnn_head_fwd_ml_weighted(*head, None, None) if weighted else lib.sgnn_head_fwd_ml(*head)) == 0
        gl = torch.ones(1, device=DEV)
        tail = (b['logits'].ptr, ops._ptr(t), ops._ptr(gl), None, ctypes.c_void_p(b['out'].t.data_ptr() + 8), b['a1'].ptr, b['a2'].ptr,
                ops._ptr(W2), ops._ptr(W3), B, H1, H2, K, 0.0, b['dz1'].ptr, b['partial'].ptr, ops._stream())
        assert (lib.sgnn_head_bwd_ml_weighted(*tail, None, None) if weighted else lib.sgnn_head_bwd_ml(*tail)) == 0
        torch.cuda.synchronize()
        got.append(b)
    for name in got[0]:
        assert torch.equal(got[0][name].t, got[1][name].t) and got[1][name].intact(), name


def test_multi_label_extreme_logits_stay_finite():
    """Logits of +-100 and +-2^-24 with pos_weight 0, 1 and 50 (each combination a column: lin3.weight = 0, lin3.bias = the
    logits), rows of all-zero and all-one targets: loss and gradients finite and equal to float64 torch's."""
    ops = _ops()
    vals = [100.0, -100.0, 2.0 ** -24, -2.0 ** -24]
    v = torch.tensor([a for a in vals for _ in range(3)])
    pw = torch.tensor([0.0, 1.0, 50.0] * 4)
    cw = torch.tensor([0.5, 2.0, 1.0, 3.0] * 3)
    K = v.numel()
    t = torch.stack([torch.zeros(K), torch.ones(K)]).long()
    for w in (None, cw):
        br = v.double().clone().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(br.expand(2, K), t.double(), weight=None if w is None else w.double(),
                                                 pos_weight=pw.double())
        ref.backward()
        mods = [m.to(DEV) for m in C.head_modules(5, 4, 3, K, 1)]
        mods[2].weight.data.zero_()
        mods[2].bias.data.copy_(v.to(DEV))
        x = torch.randn(2, 5, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
        lg, loss, _ = ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.0, None, targets=t.to(DEV), class_weight=_dev(w),
                                     pos_weight=pw.to(DEV))
        loss.backward()
        assert torch.equal(lg.detach().cpu(), v.repeat(2, 1))
        assert torch.isfinite(loss) and torch.isfinite(mods[2].bias.grad).all() and torch.isfinite(x.grad).all()
        _loss_close(loss.detach(), float(ref.detach()))
        assert_close(mods[2].bias.grad, br.grad, 'grad lin3.bias', norm_tol=2e-5)
        # the stand-alone pair on the same logits
        xs = v.repeat(2, 1).to(DEV).requires_grad_(True)
        loss, _ = ops.bce_with_logits_and_accuracy(xs, t.to(DEV), weight=_dev(w), pos_weight=pw.to(DEV))
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(xs.grad).all()
        _loss_close(loss.detach(), float(ref.detach()))
        assert_close(xs.grad.sum(0), br.grad, 'grad logits', norm_tol=2e-5)


def test_dropout_masks_do_not_depend_on_the_loss_mode():
    """p = 0.3, the same {seed, step}: logits, a1, a2 and the state after a weighted call equal those of a bare call."""
    shape = (3000, 40, 64, 32, 4)
    B, H0, H1, H2, K = shape
    g, mods, z1 = _raw_inputs(shape, seed=1)
    y = torch.randint(0, K, (B,), generator=g).to(DEV)
    w = C.class_weights(K, g)
    got = []
    for weights, weighted in ((None, False), (w, True)):
        rng = torch.tensor([1234, 5], dtype=torch.int64, device=DEV)
        b = _raw_head(shape, z1, mods, y, weights, p=0.3, rng=rng, weighted_entry=weighted)
        assert rng.tolist() == [1234, 6]
        got.append(b)
    for name in ('logits', 'a1', 'a2'):
        assert torch.equal(got[0][name].t, got[1][name].t), name
    assert float((got[0]['a1'].t == 0).float().mean()) > 0.3                # masks were drawn
    assert not torch.equal(got[0]['out'].t[:1], got[1]['out'].t[:1])          # ... and the weights applied
    # through ops, multi-label: the weighted call's logits are the bare call's
    ops = _ops()
    x = torch.randn(B, H0, generator=g).to(DEV)
    t = (torch.rand(B, K, generator=g) < 0.5).long().to(DEV)
    r0 = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    lg_a, _, _ = ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.3, r0, targets=t)
    r1 = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    lg_b, _, _ = ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.3, r1, targets=t, pos_weight=w.to(DEV))
    assert torch.equal(lg_a, lg_b) and r0.tolist() == r1.tolist() == [1234, 1]


# ---- the stand-alone pairs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,K', C.PAIR_SHAPES)
def test_weighted_cross_entropy_pair_matches_torch(B, K):
    ops = _ops()
    case = C.pair_case((B, K))
    xg = case['x'].to(DEV).requires_grad_(True)
    y, w = case['y'].to(DEV), case['w'].to(DEV)
    loss, acc = ops.cross_entropy_with_accuracy(xg, y, weight=w)
    (loss * 1.5).backward()
    _loss_close(loss.detach(), case['loss'])
    hits = int(((xg.detach().argmax(1) == y) & (y >= 0)).sum())
    assert round(float(acc) * B) == hits
    assert_close(xg.grad, case['grad'], 'grad logits', norm_tol=2e-5)
    loss2, acc2 = ops.cross_entropy_with_accuracy(case['x'].to(DEV), y, weight=w)
    assert torch.equal(loss2, loss.detach()) and torch.equal(acc2, acc)


@pytest.mark.parametrize('mode', C.ML_MODES)
@pytest.mark.parametrize('B,K', C.PAIR_SHAPES)
def test_weighted_bce_pair_matches_torch(B, K, mode):
    ops = _ops()
    case = C.pair_case((B, K), mode)
    xg = case['x'].to(DEV).requires_grad_(True)
    t = case['y'].to(DEV)
    loss, acc = ops.bce_with_logits_and_accuracy(xg, t, weight=_dev(case['w']), pos_weight=_dev(case['pw']))
    (loss * 1.5).backward()
    _loss_close(loss.detach(), case['loss'])
    hits = int(((torch.sigmoid(xg.detach()) > 0.5) == (t != 0)).all(1).sum())
    assert round(float(acc) * B) == hits
    assert_close(xg.grad, case['grad'], 'grad logits', norm_tol=2e-5)
    loss2, acc2 = ops.bce_with_logits_and_accuracy(case['x'].to(DEV), t, weight=_dev(case['w']), pos_weight=_dev(case['pw']))
    assert torch.equal(loss2, loss.detach()) and torch.equal(acc2, acc)


def test_pairs_write_inside_their_outputs():
    """The raw entries of both weighted pairs at (257, 40) -- two workgroups forward, K above the head's limit -- on guarded
    buffers, with a label of K among the rows: every guard word intact, the weight rows unchanged."""
    from subgnn_amd import _lib
    ops = _ops()
    lib = _lib.load()
    B, K = 257, 40
    case = C.pair_case((B, K))
    x = case['x'].to(DEV).contiguous()
    y = case['y'].clone()
    y[200] = K
    y = y.to(DEV)
    w = Guarded(K, fill=case['w'])
    lse, res, grad = Guarded(B + 1), Guarded(2), Guarded(B * K)
    wsb = int(lib.sgnn_cross_entropy_workspace_bytes(B))
    ws = Guarded(wsb // 4 + 1)
    st = ops._stream()
    assert lib.sgnn_cross_entropy_fwd_weighted(ops._ptr(x), ops._ptr(y), B, K, lse.ptr, res.ptr, ctypes.c_void_p(res.t.data_ptr() + 4),
                                               ws.ptr, wsb, st, w.ptr) == 0
    gl = torch.ones(1, device=DEV)
    assert lib.sgnn_cross_entropy_bwd_weighted(ops._ptr(x), ops._ptr(y), lse.ptr, ops._ptr(gl), B, K, grad.ptr, st, w.ptr) == 0
    torch.cuda.synchronize()
    assert torch.isnan(res.t[0])
    for name, b in (('w', w), ('lse', lse), ('res', res), ('grad', grad), ('ws', ws)):
        assert b.intact(), name
    assert torch.equal(w.t.cpu(), case['w']) and bool((grad.t.view(B, K)[200] == 0).all())
    mc = C.pair_case((B, K), 'both')
    t = mc['y'].to(DEV)
    cw, pw = Guarded(K, fill=mc['w']), Guarded(K, fill=mc['pw'])
    res, grad = Guarded(2), Guarded(B * K)
    wsb = int(lib.sgnn_bce_logits_workspace_bytes(B))
    ws = Guarded(wsb // 4 + 1)
    xm = mc['x'].to(DEV).contiguous()
    assert lib.sgnn_bce_logits_fwd_weighted(ops._ptr(xm), ops._ptr(t), B, K, res.ptr, ctypes.c_void_p(res.t.data_ptr() + 4), ws.ptr, wsb,
                                            st, cw.ptr, pw.ptr) == 0
    assert lib.sgnn_bce_logits_bwd_weighted(ops._ptr(xm), ops._ptr(t), ops._ptr(gl), B, K, grad.ptr, st, cw.ptr, pw.ptr) == 0
    torch.cuda.synchronize()
    _loss_close(res.t[0], mc['loss'])
    assert_close(grad.t.view(B, K) * 1.5, mc['grad'], 'grad logits', norm_tol=2e-5)
    for name, b in (('weight', cw), ('pos_weight', pw), ('res', res), ('grad', grad), ('ws', ws)):
        assert b.intact(), name


# ---- the model ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def datasets(tmp_path_factory):
    return write_datasets(tmp_path_factory.mktemp('weighted'))


def write_datasets(root):
    """The ``tiny`` golden (single-label) and the density golden turned multi-label as tests/test_gpu_multilabel_head.py does
    it (every third label a pair), in one project root."""
    from conftest import load_golden
    tiny = load_golden('tiny')
    write_dataset_from_golden(tiny, root, 'tiny')
    golden = load_golden('density')
    write_dataset_from_golden(golden, root, 'ml', with_ego=False)
    f = os.path.join(str(root), 'ml', 'subgraphs.pth')
    out = []
    for i, r in enumerate(open(f).read().splitlines()):
        c = r.split('\t')
        lab = int(c[1])
        c[1] = '%d-%d' % (lab, (lab + 1) % 3) if i % 3 == 0 else str(lab)
        out.append('\t'.join(c))
    open(f, 'w').write('\n'.join(out) + '\n')
    return root, {'tiny': tiny, 'ml': golden}


def _model(datasets, name, **over):
    from subgnn_amd import config
    from subgnn_amd.SubGNN import SubGNN, dataset_paths
    root, goldens = datasets
    config.PROJECT_ROOT = root
    hp = dict(goldens[name].hp)
    hp.update({'seed': goldens[name].seed, 'lin_dropout': 0.0, 'lstm_dropout': 0.0})
    if name == 'ml':
        hp['neigh_sample_border_size'] = 2
    hp.update(over)
    torch.manual_seed(0)
    return SubGNN(hp, **dataset_paths(name)), hp


def _step_gradients(datasets, name, **over):
    """One training step's loss and every parameter gradient, from the same initial state and the same draws."""
    m, hp = _model(datasets, name, **over)
    torch.manual_seed(5)
    m.prepare_data()
    m.train()
    opt = m.configure_optimizers()
    B = min(int(hp['batch_size']), len(m.train_sub_G))
    batch = m.make_batch('train', torch.arange(B))
    out = m.training_step(batch, 0)
    opt.zero_grad(set_to_none=True)
    m.backward(None, out['loss'], opt, 0)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return m, float(out['loss'].detach()), grads, batch


ROUTES = (('fused', {}), ('standalone', {'fused_head': False}), ('library', {'fused_forward': False}))


@pytest.mark.parametrize('name,weights', [('tiny', {'class_weight': 'balanced'}), ('ml', {'pos_weight': 'balanced'}),
                                          ('ml', {'pos_weight': 'balanced', 'class_weight': [0.5, 2.0, 1.5]})])
def test_model_routes_agree(datasets, name, weights, monkeypatch):
    """One training step's loss and every parameter gradient agree between the fused head, the stand-alone pair (fused_head:
    false) and the library (fused_forward: false); the kernel routes never reach the library's loss function, and the loss is not
    the bare model's."""
    from subgnn_amd import ops
    res = {}
    for route, over in ROUTES:
        calls = {'n': 0}
        lib_fn = 'binary_cross_entropy_with_logits' if name == 'ml' else 'cross_entropy'
        orig = getattr(F, lib_fn)

        def counted(*a, _orig=orig, _calls=calls, **k):
            _calls['n'] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(F, lib_fn, counted)
        seen = {'head': 0, 'pair': 0}
        o_head, o_ce, o_bce = ops.fused_head, ops.cross_entropy_with_accuracy, ops.bce_with_logits_and_accuracy

        def head(*a, _s=seen, **k):
            _s['head'] += int(k.get('class_weight') is not None or k.get('pos_weight') is not None)
            return o_head(*a, **k)

        def pair(fn, _s=seen):
            def f(*a, **k):
                _s['pair'] += int(k.get('weight') is not None or k.get('pos_weight') is not None)
                return fn(*a, **k)
            return f
        monkeypatch.setattr(ops, 'fused_head', head)
        monkeypatch.setattr(ops, 'cross_entropy_with_accuracy', pair(o_ce))
        monkeypatch.setattr(ops, 'bce_with_logits_and_accuracy', pair(o_bce))
        try:
            m, loss, grads, _ = _step_gradients(datasets, name, **dict(weights, **over))
        finally:
            monkeypatch.undo()
        print(name, weights, route, 'loss %.9g' % loss, seen, calls)
        assert (seen['head'] > 0, seen['pair'] > 0, calls['n'] > 0) == {'fused': (True, False, False), 'standalone': (False, True, False),
                                                                       'library': (False, False, True)}[route], (route, seen, calls)
        res[route] = (loss, grads)
    ref_loss, ref_grads = res['library']
    assert np.isfinite(ref_loss)
    for route in ('fused', 'standalone'):
        loss, grads = res[route]
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (route, loss, ref_loss)
        assert grads.keys() == ref_grads.keys() and len(grads) > 10
        for k in grads:
            assert_close(grads[k], ref_grads[k], '%s: grad %s' % (route, k))
    for k in res['fused'][1]:
        assert_close(res['fused'][1][k], res['standalone'][1][k], 'fused against stand-alone: grad ' + k, norm_tol=2e-5)
    _, bare_loss, _, _ = _step_gradients(datasets, name)
    assert abs(bare_loss - ref_loss) > 1e-4 * abs(ref_loss), (bare_loss, ref_loss)


@pytest.mark.parametrize('name,weights', [('tiny', {'class_weight': 'balanced'}), ('ml', {'pos_weight': 'balanced'})])
def test_validation_loss_is_the_modules(datasets, name, weights):
    """val_test_step's loss is ``self.loss`` applied by hand to its logits -- on the device and on host copies (what the
    recorded validation hands val_test_outputs)."""
    m, hp = _model(datasets, name, **weights)
    torch.manual_seed(5)
    m.prepare_data()
    m.eval()
    with torch.no_grad():
        batch = m.make_batch('val', torch.arange(min(int(hp['batch_size']), len(m.val_sub_G))))
        out = m.validation_step(batch, 0)
        logits, labels = out['val_logits'], out['val_labels']
        if name == 'ml':
            w, pw = m.loss.weight, m.loss.pos_weight
            assert pw is not None and pw.is_cuda
            by_hand = F.binary_cross_entropy_with_logits(logits, labels.type_as(logits), weight=w, pos_weight=pw)
            on_host = F.binary_cross_entropy_with_logits(logits.cpu().double(), labels.cpu().double(), pos_weight=pw.cpu().double())
        else:
            w = m.loss.weight
            assert w is not None and w.is_cuda
            by_hand = F.cross_entropy(logits, labels, weight=w)
            on_host = F.cross_entropy(logits.cpu().double(), labels.cpu(), weight=w.cpu().double())
        assert torch.equal(out['val_loss'], by_hand)
        host = m.val_test_outputs('val', logits.cpu(), labels.cpu())
        assert not host['val_loss'].is_cuda
        _loss_close(host['val_loss'], float(on_host))
        _loss_close(out['val_loss'], float(on_host))
        assert m.loss.weight is None or m.loss.weight.is_cuda               # the module itself stayed where it was


@pytest.mark.parametrize('name,weights', [('tiny', {'class_weight': 'balanced'}), ('ml', {'pos_weight': 'balanced'})])
def test_recorded_and_eager_epochs_agree(datasets, name, weights):
    """Two epochs of the Trainer with hip_graph_step True and False on a weighted model: the weights are static device tensors
    and the denominator is formed on the device, so the recorded step replays the weighted launches -- the training losses of both
    epochs agree BIT FOR BIT.  The validation loss is not the training step's: with hip_graph_step the trainer evaluates
    ``self.loss`` on HOST copies of an epoch's logits (Trainer._validation_outputs: torch's CPU kernels), without it on the device,
    so its last bits follow the float32 summation order of two different reductions -- for bare losses too (measured on the
    MI355X, eager / recorded: the bare tiny model 1.08256578 / 1.0825659 in epoch 1 and 1.07966197 / 1.07966208 in epoch 2, the
    bare multi-label model 0.701057434 / 0.701057315 in epoch 1; with class_weight 'balanced' 1.01461744 / 1.01461756 and with
    pos_weight 'balanced' 0.847019613 / 0.847019434 in epoch 2; every training loss equal in all four).  It is held
    to the 1e-6 that the existing recorded-versus-eager tests ask of it for bare losses (tests/test_gpu_multilabel_head.py,
    tests/test_gpu_train_driver.py)."""
    from subgnn_amd.train_config import Trainer
    runs = {}
    for graph_step in (False, True):
        m, hp = _model(datasets, name, **weights)
        tr = Trainer(2, hp.get('grad_clip', 0.0), log=lambda *a, **k: None, hip_graph_step=graph_step)
        torch.manual_seed(5)
        tr.fit(m)
        assert tr.hip_graph_step == graph_step                               # the step was recorded, not abandoned
        runs[graph_step] = {'train': [h['train_loss'] for h in tr.history], 'val': [h['val_loss'] for h in tr.history]}
        assert all(np.isfinite(runs[graph_step]['train'] + runs[graph_step]['val']))
    for k in ('train', 'val'):
        print(name, k, 'eager', ['%.9g' % v for v in runs[False][k]], 'recorded', ['%.9g' % v for v in runs[True][k]])
    assert runs[False]['train'] == runs[True]['train'], runs
    for a, b in zip(runs[False]['val'], runs[True]['val']):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), runs


def test_a_loss_assigned_by_hand_is_applied(datasets):
    """model.loss = nn.CrossEntropyLoss(weight=w): the step's loss is the weighted one, through the weighted launch (the library's
    loss function is not reached); label_smoothing = 0.1 goes through the library and gives torch's value."""
    m, hp = _model(datasets, 'tiny')
    torch.manual_seed(5)
    m.prepare_data()
    m.train()
    batch = m.make_batch('train', torch.arange(min(int(hp['batch_size']), len(m.train_sub_G))))
    labels = batch['label'].squeeze(-1)
    K = m.num_classes
    w = C.class_weights(K, torch.Generator().manual_seed(4), zero=False).to(DEV)
    with torch.no_grad():
        m.eval()                                                             # (the same logits as the training step: no dropout)
        logits = m._forward_batch('train', batch)
        m.train()
    bare = float(m.training_step(batch, 0)['loss'])
    _loss_close(bare, float(F.cross_entropy(logits.double().cpu(), labels.cpu())))
    m.loss = torch.nn.CrossEntropyLoss(weight=w)
    orig = F.cross_entropy

    def boom(*a, **k):
        raise AssertionError('F.cross_entropy was reached in training_step')
    F.cross_entropy = boom
    try:
        got = float(m.training_step(batch, 0)['loss'])
    finally:
        F.cross_entropy = orig
    want = float(F.cross_entropy(logits.double().cpu(), labels.cpu(), weight=w.double().cpu()))
    print('bare %.9g  weighted %.9g  torch %.9g' % (bare, got, want))
    _loss_close(got, want)
    assert abs(got - bare) > 1e-4 * abs(bare)
    m.loss = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)
    got = float(m.training_step(batch, 0)['loss'])
    want = float(F.cross_entropy(logits.double().cpu(), labels.cpu(), weight=w.double().cpu(), label_smoothing=0.1))
    _loss_close(got, want)

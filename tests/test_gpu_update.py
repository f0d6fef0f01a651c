"""-m gpu: the update layer (subgnn_amd/csrc/update.hip through ops.update_layer / ops.update_layers and through the library's
entries directly) against the float64 CPU reference of tests/update_cases.py, at every launch form, row edge, chunk count,
body count and gradient subset (tests/test_update_cases_host.py shows on the CPU which form each case reaches).  ``grid`` cases
are compared with torch.equal -- no result of theirs depends on the order of a sum -- and ``float`` cases within the bounds of
tests/test_gpu_float.py's update tests.  Then what no reference can show: that stores stay inside their tensors, that a refused
call writes nothing, and that NaN and Inf come out as torch.relu gives them."""
import collections

import numpy as np
import pytest
import torch

import update_cases as UC
from helpers import REL_TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUT_NORM_TOL, GRAD_NORM_TOL = 1e-5, 2e-5         # tests/test_gpu_float.py::test_update_layer_matches_torch
NAMES = ('x', 'aggr', 'W', 'b')
PATTERN = 0x7FA5A5A5                             # as float32 a NaN with a payload: nothing the kernels compute
BAD_ARG, UNSUPPORTED_D = -1, -5


def _ops():
    from subgnn_amd import ops
    return ops


def _lib():
    from subgnn_amd import _lib
    return _lib.load()


def _case(name):
    return next(c for c in UC.CASES if c.name == name)


def _run(ops, case, only=None):
    """One forward + backward of the case on the device -> [{'out', 'x', 'aggr', 'W', 'b': gradient or None} per body].
    only = k: body k alone, through ops.update_layer."""
    inp = UC.inputs(case)
    picked = [(body, b) for k, (body, b) in enumerate(zip(case.bodies, inp['bodies'])) if only is None or k == only]
    leaves = [{n: (None if b[n] is None else b[n].to(DEV).requires_grad_(w)) for n, w in zip(NAMES, body.grads)} for body, b in picked]
    if case.via == 'layer' or only is not None:
        outs = [ops.update_layer(lv['x'], lv['aggr'], lv['W'], lv['b']) for lv in leaves]
    else:
        outs = ops.update_layers([ops.PendingUpdate(lv['x'], lv['aggr'], lv['W'], lv['b'], (case.R, 1)) for lv in leaves])
    assert len(outs) == len(leaves)
    loss = None
    for out, (body, b) in zip(outs, picked):
        if b['go'] is not None and out.requires_grad:
            term = (out * b['go'].to(DEV)).sum()
            loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
    torch.cuda.synchronize()
    return [dict({'out': out.detach()}, **{n: (None if t is None else t.grad) for n, t in lv.items()}) for out, lv in zip(outs, leaves)]


def _same_bits(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a, b), what


def _compare(case, got, ref, what, name):
    assert got.shape == ref.shape and got.dtype == torch.float32, what
    if case.kind == 'grid':
        ref = ref.float().to(got.device)
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            i = tuple(int(v) for v in bad[0])
            raise AssertionError('%s: %d of %d elements differ, the first at %r: got %.9g, want %.9g'
                                 % (what, bad.shape[0], got.numel(), i, float(got[i]), float(ref[i])))
    else:
        assert_close(got, ref, what, tol=REL_TOL, norm_tol=OUT_NORM_TOL if name == 'out' else GRAD_NORM_TOL)


def _counted(monkeypatch, lib, names):
    calls = collections.Counter()
    for name in names:
        def counted(*a, _f=getattr(lib, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


@pytest.mark.parametrize('case', UC.CASES, ids=lambda c: c.name)
def test_update_matches_float64_reference(case, monkeypatch):
    """The output and every requested gradient against update_cases.reference (float64, CPU): bit for bit on the grid,
    within the float bounds else; a gradient nobody asked for, or of a body whose output nobody reads, is None; a chunked
    aggregate's gradient is (chunks, R, D) with the same values in every chunk; the bodies go through as many
    sgnn_update_*_many launches as update_cases.forms says, and each equals, bit for bit, the same body run alone; a second
    run repeats the bits."""
    ops, lib = _ops(), _lib()
    ref = UC.reference(case)
    with monkeypatch.context() as mp:
        calls = _counted(mp, lib, ('sgnn_update_fwd_many', 'sgnn_update_bwd_many'))
        got = _run(ops, case)
    f = UC.forms(case)
    groups = [case.bodies[lo:lo + UC.MAX_BODIES] for lo in range(0, len(case.bodies), UC.MAX_BODIES)] if f['many'] else []
    assert calls['sgnn_update_fwd_many'] == f['many'] == len(groups)
    assert calls['sgnn_update_bwd_many'] == sum(1 for g in groups if any(b.go and any(b.grads) for b in g))
    for k, (body, g, r) in enumerate(zip(case.bodies, got, ref)):
        _compare(case, g['out'], r['out'], '%s out of body %d' % (case.name, k), 'out')
        for n in NAMES:
            what = '%s gradient of %s of body %d' % (case.name, n, k)
            if r[n] is None:
                assert g[n] is None, what + ': one arrived that nobody asked for'
                continue
            assert g[n] is not None, what + ': none arrived'
            _compare(case, g[n], r[n], what, n)
        if body.chunks and g['aggr'] is not None:
            assert g['aggr'].shape == (body.chunks, case.R, case.D)
            assert all(torch.equal(g['aggr'][0], g['aggr'][j]) for j in range(1, body.chunks))
    again = _run(ops, case)
    for k, (g, g2) in enumerate(zip(got, again)):
        for n in ('out',) + NAMES:
            _same_bits(g[n], g2[n], '%s: %s of body %d differs between two runs' % (case.name, n, k))
    if case.via == 'layers':
        for k in range(len(case.bodies)):
            alone = _run(ops, case, only=k)[0]
            for n in ('out',) + NAMES:
                _same_bits(got[k][n], alone[n], '%s: %s of body %d differs from the body run alone' % (case.name, n, k))


def test_no_rows():
    """R == 0: an empty output; the backward gives grad_W and grad_b of exact zeros and empty grad_x / grad_aggr."""
    case = _case('no-rows-64')
    got = _run(_ops(), case)[0]
    D = case.D
    assert got['out'].shape == (0, D) and got['x'].shape == (0, D) and got['aggr'].shape == (0, D)
    assert got['W'].shape == (D, 2 * D) and got['b'].shape == (D,)
    assert int((got['W'].view(torch.int32) != 0).sum()) == 0 and int((got['b'].view(torch.int32) != 0).sum()) == 0


# ---- the library's entries, called directly ---------------------------------------------------------------------------------------
class _Guarded:
    """n float32 words between two guards of 32 D words, all pre-filled with PATTERN."""

    def __init__(self, n, D):
        self.n, self.g = n, 32 * D
        self.buf = torch.full((2 * self.g + n,), PATTERN, dtype=torch.int32, device=DEV)
        self.t = self.buf[self.g:self.g + n].view(torch.float32)

    def check(self, what, written):
        inner = self.buf[self.g:self.g + self.n]
        assert bool((self.buf[:self.g] == PATTERN).all()), what + ': a store in front of the tensor'
        assert bool((self.buf[self.g + self.n:] == PATTERN).all()), what + ': a store behind the tensor'
        if written is True:
            assert bool((inner != PATTERN).all()), what + ': %d words were never written' % int((inner == PATTERN).sum())
        elif written is False:
            assert bool((inner == PATTERN).all()), what + ': written by a call that must not write it'


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _table(ops, ts):
    return ops._ptr_table([t.t if isinstance(t, _Guarded) else t for t in ts])


@pytest.mark.parametrize('D', UC.DIMS)
@pytest.mark.parametrize('R', [1, 33, 4097, 16385])
def test_stores_stay_inside(R, D):
    """sgnn_update_fwd_chunks / sgnn_update_fwd and sgnn_update_bwd write every word of out, aggr_sum, grad_x, grad_aggr,
    grad_W, grad_b and nothing in the 32 D words in front of and behind each, nor around the workspace."""
    ops, lib = _ops(), _lib()
    P, st = ops._ptr, ops._stream()
    k = 3 if R < UC.KSPLIT_BELOW else 1
    x, a, W, b, go = (_randn(*s, seed=R + D + i) for i, s in enumerate(((R, D), (k, R, D), (D, 2 * D), (D,), (R, D))))
    out, total = _Guarded(R * D, D), _Guarded(R * D, D)
    if k > 1:
        assert lib.sgnn_update_fwd_chunks(P(x), P(a), k, P(W), P(b), R, D, P(out.t), P(total.t), st) == 0
        aggr = total.t
    else:
        assert lib.sgnn_update_fwd(P(x), P(a), P(W), P(b), R, D, P(out.t), st) == 0
        aggr = a[0]
    torch.cuda.synchronize()
    out.check('out', True)
    total.check('aggr_sum', k > 1)
    assert_close(out.t.view(R, D), torch.relu(torch.cat([x, a.sum(0)], 1).double() @ W.double().t() + b.double()), 'out',
                 norm_tol=OUT_NORM_TOL)
    wsb = lib.sgnn_update_bwd_workspace_bytes(R, D)
    assert wsb == UC.workspace_bytes(R, D) and wsb % 4 == 0
    gx, ga, gW, gb, ws = _Guarded(R * D, D), _Guarded(R * D, D), _Guarded(D * 2 * D, D), _Guarded(D, D), _Guarded(wsb // 4, D)
    assert lib.sgnn_update_bwd(P(go), P(out.t), P(x), P(aggr), P(W), R, D, P(gx.t), P(ga.t), P(gW.t), P(gb.t), P(ws.t), wsb, st) == 0
    torch.cuda.synchronize()
    for t, what in ((gx, 'grad_x'), (ga, 'grad_aggr'), (gW, 'grad_W'), (gb, 'grad_b')):
        t.check(what, True)
    ws.check('workspace', None)
    out.check('out after the backward', True)


@pytest.mark.parametrize('D', UC.DIMS)
@pytest.mark.parametrize('R', [1, 33])
def test_stores_of_several_bodies_stay_inside(R, D):
    """The same for sgnn_update_fwd_many / sgnn_update_bwd_many with three bodies of 1, 2 and 3 chunks; body 1 receives no
    gradient: every word of its gradients keeps the pattern."""
    ops, lib = _ops(), _lib()
    st, n, chunks = ops._stream(), 3, (1, 2, 3)
    xs = [_randn(R, D, seed=10 * j + 1) for j in range(n)]
    ags = [_randn(c, R, D, seed=10 * j + 2) for j, c in enumerate(chunks)]
    Ws = [_randn(D, 2 * D, seed=10 * j + 3) for j in range(n)]
    bs = [_randn(D, seed=10 * j + 4) for j in range(n)]
    gos = [_randn(R, D, seed=5), None, _randn(R, D, seed=25)]
    outs = [_Guarded(R * D, D) for _ in range(n)]
    sums = [None] + [_Guarded(R * D, D) for _ in range(n - 1)]
    nch = np.array(chunks, dtype=np.int64)
    tb = [_table(ops, v) for v in (xs, ags, Ws, bs, outs, sums)]
    assert lib.sgnn_update_fwd_many(n, tb[0].ctypes.data, tb[1].ctypes.data, nch.ctypes.data, tb[2].ctypes.data, tb[3].ctypes.data, R, D,
                                    tb[4].ctypes.data, tb[5].ctypes.data, st) == 0
    torch.cuda.synchronize()
    for j in range(n):
        outs[j].check('out of body %d' % j, True)
        if sums[j] is not None:
            sums[j].check('aggr_sum of body %d' % j, True)
        assert_close(outs[j].t.view(R, D), torch.relu(torch.cat([xs[j], ags[j].sum(0)], 1).double() @ Ws[j].double().t() + bs[j].double()),
                     'out of body %d' % j, norm_tol=OUT_NORM_TOL)
    per = lib.sgnn_update_bwd_workspace_bytes(R, D)
    gxs, gas = [_Guarded(R * D, D) for _ in range(n)], [_Guarded(R * D, D) for _ in range(n)]
    gWs, gbs = [_Guarded(D * 2 * D, D) for _ in range(n)], [_Guarded(D, D) for _ in range(n)]
    ws = _Guarded(n * per // 4, D)
    kept = [ags[0][0], sums[1].t, sums[2].t]
    tg = [_table(ops, v) for v in (gos, outs, xs, kept, Ws, gxs, gas, gWs, gbs)]
    assert lib.sgnn_update_bwd_many(n, *(t.ctypes.data for t in tg[:5]), R, D, *(t.ctypes.data for t in tg[5:]), ops._ptr(ws.t), n * per, st) == 0
    torch.cuda.synchronize()
    for j in range(n):
        for t, what in ((gxs[j], 'grad_x'), (gas[j], 'grad_aggr'), (gWs[j], 'grad_W'), (gbs[j], 'grad_b')):
            t.check('%s of body %d' % (what, j), j != 1)
    ws.check('workspace', None)


@pytest.mark.parametrize('D', UC.DIMS)
@pytest.mark.parametrize('R,k', [(33, 2), (33, 70), (4095, 3), (4095, 70)])
def test_chunk_adding_is_the_sum_in_chunk_order(R, k, D):
    """sgnn_update_fwd_chunks: aggr_sum is ((a[0] + a[1]) + a[2]) + ... in float32, bit for bit (the kernel makes the same
    plain adds in the same order), and out is, bit for bit, what sgnn_update_fwd writes for that sum."""
    ops, lib = _ops(), _lib()
    P, st = ops._ptr, ops._stream()
    x, a, W, b = (_randn(*s, seed=R + D + k + i) for i, s in enumerate(((R, D), (k, R, D), (D, 2 * D), (D,))))
    out, total, plain = (torch.full((R, D), float('nan'), device=DEV) for _ in range(3))
    assert lib.sgnn_update_fwd_chunks(P(x), P(a), k, P(W), P(b), R, D, P(out), P(total), st) == 0
    want = a[0].clone()
    for j in range(1, k):
        want = want + a[j]
    assert lib.sgnn_update_fwd(P(x), P(want), P(W), P(b), R, D, P(plain), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(total, want), 'aggr_sum is not the chunks added in order'
    assert not plain.isnan().any() and torch.equal(out, plain)


def test_refused_calls_write_nothing():
    """Every argument error of the update entries, with real device tensors large enough for the call had it been taken: the
    code the header names comes back and every output keeps its bytes."""
    ops, lib = _ops(), _lib()
    from subgnn_amd._lib import ERRORS
    P, st = ops._ptr, ops._stream()
    RA, DA = UC.KSPLIT_BELOW, 128                                    # the allocation: the largest shape any call below names
    x, W, b, go = _randn(RA, DA, seed=1), _randn(DA, 2 * DA, seed=2), _randn(DA, seed=3), _randn(RA, DA, seed=4)
    a = _randn(2, RA, DA, seed=5)
    act = torch.relu(_randn(RA, DA, seed=6))                         # an ``out`` for the backward calls
    out, total, gx, ga = (_Guarded(RA * DA, DA) for _ in range(4))
    gW, gb = _Guarded(DA * 2 * DA, DA), _Guarded(DA, DA)
    wsb = UC.MAX_BODIES * max(lib.sgnn_update_bwd_workspace_bytes(RA, DA), lib.sgnn_update_bwd_workspace_bytes(RA - 1, DA))
    ws = _Guarded(wsb // 4, DA)
    written = (out, total, gx, ga, gW, gb, ws)

    def many_fwd(n, R, D, chunks=None, sums=True):
        m = max(n, 1)
        nch = np.array(chunks or [1] * m, dtype=np.int64)
        tb = [_table(ops, [t] * m) for t in (x, a, W, b, out, total if sums else None)]
        return lib.sgnn_update_fwd_many(n, tb[0].ctypes.data, tb[1].ctypes.data, nch.ctypes.data, tb[2].ctypes.data, tb[3].ctypes.data,
                                        R, D, tb[4].ctypes.data, tb[5].ctypes.data, st)

    def many_bwd(n, R, D):
        m = max(n, 1)
        tb = [_table(ops, [t] * m) for t in (go, act, x, a, W, gx, ga, gW, gb)]
        return lib.sgnn_update_bwd_many(n, *(t.ctypes.data for t in tb[:5]), R, D, *(t.ctypes.data for t in tb[5:]), P(ws.t), wsb, st)

    def bwd(R, D, x_=x, bytes_=wsb):
        return lib.sgnn_update_bwd(P(go), P(act), P(x_), P(a), P(W), R, D, P(gx.t), P(ga.t), P(gW.t), P(gb.t), P(ws.t), bytes_, st)

    small = lib.sgnn_update_bwd_workspace_bytes(33, 64)
    calls = [
        ('fwd_chunks, 2 chunks of 4096 rows', lambda: lib.sgnn_update_fwd_chunks(P(x), P(a), 2, P(W), P(b), RA, 64, P(out.t), P(total.t), st), BAD_ARG),
        ('fwd_chunks, 0 chunks', lambda: lib.sgnn_update_fwd_chunks(P(x), P(a), 0, P(W), P(b), 33, 64, P(out.t), P(total.t), st), BAD_ARG),
        ('fwd_chunks, 4097 chunks', lambda: lib.sgnn_update_fwd_chunks(P(x), P(a), 4097, P(W), P(b), 33, 64, P(out.t), P(total.t), st), BAD_ARG),
        ('fwd, D = 48', lambda: lib.sgnn_update_fwd(P(x), P(a), P(W), P(b), 33, 48, P(out.t), st), UNSUPPORTED_D),
        ('fwd_chunks, D = 48', lambda: lib.sgnn_update_fwd_chunks(P(x), P(a), 2, P(W), P(b), 33, 48, P(out.t), P(total.t), st), UNSUPPORTED_D),
        ('bwd, D = 48', lambda: bwd(33, 48), UNSUPPORTED_D),
        ('fwd_many, D = 48', lambda: many_fwd(2, 33, 48), UNSUPPORTED_D),
        ('bwd_many, D = 48', lambda: many_bwd(2, 33, 48), UNSUPPORTED_D),
        ('fwd_many, n = 0', lambda: many_fwd(0, 33, 64), BAD_ARG),
        ('fwd_many, n = 9', lambda: many_fwd(9, 33, 64), BAD_ARG),
        ('fwd_many, 4096 rows', lambda: many_fwd(2, RA, 64), BAD_ARG),
        ('bwd_many, n = 0', lambda: many_bwd(0, 33, 64), BAD_ARG),
        ('bwd_many, n = 9', lambda: many_bwd(9, 33, 64), BAD_ARG),
        ('bwd_many, 4096 rows', lambda: many_bwd(2, RA, 64), BAD_ARG),
        ('bwd, a workspace one byte short', lambda: bwd(33, 64, bytes_=small - 1), BAD_ARG),
        ('bwd, grad_W without x', lambda: bwd(33, 64, x_=None), BAD_ARG),
        ('fwd_many, 2 chunks and no aggr_sum', lambda: many_fwd(2, 33, 64, chunks=[1, 2], sums=False), BAD_ARG),
    ]
    for what, call, want in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == want, '%s: %s, not %s' % (what, ERRORS.get(rc, rc), ERRORS[want])
        for t in written:
            t.check(what, False)
    # the same arguments, in order, are taken
    assert bwd(33, 64, bytes_=small) == 0
    torch.cuda.synchronize()
    for t, n in ((gx, 33 * 64), (ga, 33 * 64), (gW, 64 * 128), (gb, 64)):
        assert bool((t.buf[t.g:t.g + n] != PATTERN).all())


def test_no_rows_direct():
    """R == 0 with the NULL pointers of empty tensors: both entries return SGNN_OK; grad_W and grad_b become exact zeros and
    nothing around them is touched."""
    ops, lib = _ops(), _lib()
    P, st, D = ops._ptr, ops._stream(), 64
    W = _randn(D, 2 * D, seed=1)
    gW, gb = _Guarded(D * 2 * D, D), _Guarded(D, D)
    assert lib.sgnn_update_fwd(None, None, P(W), None, 0, D, None, st) == 0
    assert lib.sgnn_update_bwd(None, None, None, None, P(W), 0, D, None, None, P(gW.t), P(gb.t), None, 0, st) == 0
    torch.cuda.synchronize()
    for t, what in ((gW, 'grad_W'), (gb, 'grad_b')):
        t.check(what, True)
        assert int((t.buf[t.g:t.g + t.n] != 0).sum()) == 0, what


# ---- NaN and Inf -------------------------------------------------------------------------------------------------------------------
def _poisoned(b, R):
    """The body's inputs with a NaN in one element of row R // 3 of x and +Inf in one element of row 2 R // 3 of aggr."""
    rn, ri = R // 3, 2 * R // 3
    x, a = b['x'].clone(), b['aggr'].clone()
    x[rn, 5] = float('nan')
    if a.dim() == 3:
        a[-1, ri, 7] = float('inf')                                  # (in the last chunk alone)
    else:
        a[ri, 7] = float('inf')
    return dict(b, x=x, aggr=a), rn, ri


def _check_non_finite(got, clean, bad, b, rn, ri, D, what):
    ref = torch.relu(UC.pre_activation(bad))                             # float64, CPU: torch.relu keeps a NaN
    assert ref[rn].isnan().all() and ref.isnan().sum() == D
    got_c, clean_c = got.cpu(), clean.cpu()
    assert got_c[rn].isnan().all(), '%s: the row with a NaN came out as %r' % (what, got_c[rn][:8].tolist())
    pos = b['W'][:, D + 7] > 0
    assert (b['W'][:, D + 7] != 0).all() and pos.any() and (~pos).any()
    assert (got_c[ri][pos] == float('inf')).all(), what + ': +Inf x a positive weight'
    assert (got_c[ri][~pos] == 0).all(), what + ': +Inf x a negative weight'
    others = torch.ones(got_c.shape[0], dtype=torch.bool)
    others[[rn, ri]] = False
    assert torch.equal(got_c[others], clean_c[others]), what + ': a row without a non-finite input changed'
    assert torch.equal(got_c.isnan(), ref.isnan()) and torch.equal(got_c.isinf(), ref.isinf()), what
    fin = ref.isfinite()
    assert_close(got_c[fin], ref[fin], what, norm_tol=OUT_NORM_TOL)


@pytest.mark.parametrize('R', [33, 4097, 16385])
def test_non_finite_values_come_out_as_torch_relu_gives_them(R):
    """One test per forward kernel.  A NaN pre-activation is a NaN output (a diverged weight must reach the loss: the
    learning-rate range test and the search's pruning read it there), +Inf comes out as +Inf or 0 by the weight's sign, and
    every other row keeps its bits."""
    ops = _ops()
    case = _case('rows-float-%d-64' % R)
    b = UC.inputs(case)['bodies'][0]
    bad, rn, ri = _poisoned(b, R)
    dev = lambda d: [d[n].to(DEV) for n in NAMES]
    with torch.no_grad():
        got, clean = ops.update_layer(*dev(bad)), ops.update_layer(*dev(b))
    torch.cuda.synchronize()
    _check_non_finite(got, clean, bad, b, rn, ri, case.D, 'R = %d' % R)


def test_non_finite_values_through_several_bodies():
    ops = _ops()
    case = _case('bodies-3-33-64-float')
    bodies = UC.inputs(case)['bodies'][:2]                               # (R, D) and (3, R, D) aggregates
    bads = [_poisoned(b, case.R) for b in bodies]
    pend = lambda ds: [ops.PendingUpdate(*(d[n].to(DEV) for n in NAMES), (case.R, 1)) for d in ds]
    with torch.no_grad():
        got, clean = ops.update_layers(pend([bad for bad, _, _ in bads])), ops.update_layers(pend(bodies))
    torch.cuda.synchronize()
    for k, (b, (bad, rn, ri)) in enumerate(zip(bodies, bads)):
        _check_non_finite(got[k], clean[k], bad, b, rn, ri, case.D, 'body %d' % k)

"""-m gpu: the walk aggregator's kernels (subgnn_amd/csrc/lstm.hip), called through the library's entries directly, against the
float64 CPU references of tests/lstm_cases.py: the recurrence at tile heights 2, 4 and 8 with full and ragged last tiles (its
output AND the activations it keeps for the backward, the backward on its own and chained), the row GEMMs in both launch forms
on both sides of the switch, and the tails (tests/test_lstm_cases_host.py shows on the CPU which form each case reaches).
``grid`` cases are compared with torch.equal -- no result of theirs depends on the order of a sum -- and ``float`` cases within
the project's bounds.  Then what no reference can show: that stores stay inside their tensors (every output lies between two
bands of a NaN pattern, and every word of it must be overwritten), that a refused or empty call writes nothing, and that a
sequence's bits do not depend on the tile height it was computed at.  A few calls through ``ops`` at the end.

Every comparison prints its measured errors (pytest -s): 'ERR <kernel> <case> <element-wise> <whole-tensor>'."""
import pytest
import torch

import lstm_cases as LC
from helpers import REL_TOL, assert_close, norm_err, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUT_NORM_TOL, GRAD_NORM_TOL = 1e-5, 2e-5         # tests/test_gpu_update.py's, the walk-aggregator test's of tests/test_gpu_float.py
PATTERN = 0x7FA5A5A5                             # as float32 a NaN with a payload: nothing the kernels compute
GUARD = 4096                                     # words in front of and behind every output (a multiple of 4: float4 stores stay aligned)
BAD_ARG, UNSUPPORTED_D = -1, -5
_ids = lambda c: c.name


def _ops():
    from subgnn_amd import ops
    return ops


def _lib():
    from subgnn_amd import _lib
    return _lib.load()


class _Guarded:
    """n float32 words between two guards of GUARD words, all pre-filled with PATTERN."""

    def __init__(self, n, shape=None):
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), PATTERN, dtype=torch.int32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(torch.float32)
        if shape is not None:
            self.t = self.t.view(*shape)

    def check(self, what, written):
        inner = self.buf[GUARD:GUARD + self.n]
        assert bool((self.buf[:GUARD] == PATTERN).all()), what + ': a store in front of the tensor'
        assert bool((self.buf[GUARD + self.n:] == PATTERN).all()), what + ': a store behind the tensor'
        if written:
            assert bool((inner != PATTERN).all()), what + ': %d words were never written' % int((inner == PATTERN).sum())
        else:
            assert bool((inner == PATTERN).all()), what + ': written by a call that must not write it'


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, what
    if not torch.equal(_bits(a), _bits(b)):
        bad = (_bits(a) != _bits(b)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d elements differ in their bits, the first at %r: %.9g and %.9g'
                             % (what, bad.shape[0], a.numel(), i, float(a[i]), float(b[i])))


def _compare(kind, got, ref, kernel, what, norm_tol):
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, what
    got = got.cpu()
    print('ERR %s %s %.3e %.3e' % (kernel, what.replace(' ', '_'), rel_err(got, ref), norm_err(got, ref)))
    if kind == 'grid':
        ref = ref.float()
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            i = tuple(int(v) for v in bad[0])
            raise AssertionError('%s: %d of %d elements differ, the first at %r: got %.9g, want %.9g'
                                 % (what, bad.shape[0], got.numel(), i, float(got[i]), float(ref[i])))
    else:
        assert_close(got, ref, what, tol=REL_TOL, norm_tol=norm_tol)


# ---- the recurrence -------------------------------------------------------------------------------------------------------------
def _to_dev(inp, rows=None):
    """The device operands of rinputs: W_hh and b_hh of each direction as tensors of their own; rows: the first ``rows`` sequences."""
    pre_x, dy = (inp['pre_x'], inp['dy']) if rows is None else (inp['pre_x'][:, :rows].contiguous(), inp['dy'][:rows].contiguous())
    return {'pre_x': pre_x.to(DEV), 'dy': dy.to(DEV), 'whh': [inp['whh'][d].clone().to(DEV) for d in (0, 1)],
            'bhh': [None if b is None else b.clone().to(DEV) for b in inp['bhh']]}


def _forward(d, B, T, H, what):
    ops, lib = _ops(), _lib()
    P = ops._ptr
    out = {'y': _Guarded(B * T * 2 * H, (B, T, 2 * H)), 'gates': _Guarded(2 * B * T * 4 * H, (2, B, T, 4 * H)),
           'cell': _Guarded(2 * B * T * H, (2, B, T, H)), 'hprev': _Guarded(2 * B * T * H, (2, B, T, H))}
    assert tuple(d['pre_x'].shape) == (2, B, T, 4 * H) and all(tuple(w.shape) == (4 * H, H) for w in d['whh'])
    rc = lib.sgnn_lstm_fwd(P(d['pre_x']), P(d['whh'][0]), P(d['whh'][1]), P(d['bhh'][0]), P(d['bhh'][1]), B, T, H, P(out['y'].t),
                           P(out['gates'].t), P(out['cell'].t), P(out['hprev'].t), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, what
    for k, g in out.items():
        g.check('%s %s' % (what, k), True)
    return {k: g.t for k, g in out.items()}


def _backward(d, gates, cell, B, T, H, what):
    ops, lib = _ops(), _lib()
    P = ops._ptr
    assert tuple(gates.shape) == (2, B, T, 4 * H) and tuple(cell.shape) == (2, B, T, H) and tuple(d['dy'].shape) == (B, T, 2 * H)
    assert gates.is_contiguous() and cell.is_contiguous()
    dg = _Guarded(2 * B * T * 4 * H, (2, B, T, 4 * H))
    rc = lib.sgnn_lstm_bwd(P(d['whh'][0]), P(d['whh'][1]), P(gates), P(cell), P(d['dy']), B, T, H, P(dg.t), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, what
    dg.check(what + ' dgates', True)
    return dg.t


@pytest.mark.parametrize('case', LC.RCASES, ids=_ids)
def test_recurrence_matches_float64_reference(case):
    """sgnn_lstm_fwd: y, gates, cell and hprev against lstm_cases.lstm_ref; hprev is +0.0 at each direction's first step and,
    bit for bit, the direction's output of the step before else.  sgnn_lstm_bwd: fed the float32-rounded REFERENCE gates and
    cell states, against float64 arithmetic on those same values (the backward judged on its own), and chained after the
    device's forward against lstm_ref.  Every output is written in full and nothing around it."""
    B, T, H = case.B, case.T, case.H
    inp, ref = LC.rinputs(case), LC.rreference(case)
    d = _to_dev(inp)
    got = _forward(d, B, T, H, case.name)
    for k in ('y', 'gates', 'cell', 'hprev'):
        _compare('float', got[k], ref[k], 'lstm_fwd', '%s %s' % (case.name, k), OUT_NORM_TOL)
    hp, y = got['hprev'], got['y']
    assert int((_bits(hp[0, :, 0]) != 0).sum()) == 0 and int((_bits(hp[1, :, T - 1]) != 0).sum()) == 0, 'hprev of a first step is not +0.0'
    if T > 1:
        _same_bits(hp[0, :, 1:], y[:, :-1, :H], case.name + ': forward hprev against y of the step before')
        _same_bits(hp[1, :, :-1], y[:, 1:, H:], case.name + ': reverse hprev against y of the step before')
    g32, c32 = ref['gates'].float(), ref['cell'].float()
    fed = _backward(d, g32.to(DEV), c32.to(DEV), B, T, H, case.name + ' fed')
    _compare('float', fed, LC.lstm_bwd_ref(inp['whh'], g32, c32, inp['dy']), 'lstm_bwd_fed', case.name + ' dgates fed', GRAD_NORM_TOL)
    chained = _backward(d, got['gates'], got['cell'], B, T, H, case.name + ' chained')
    _compare('float', chained, ref['dgates'], 'lstm_bwd_chained', case.name + ' dgates chained', GRAD_NORM_TOL)


@pytest.mark.parametrize('H', LC.HIDDEN)
@pytest.mark.parametrize('B', LC.TILE_PAIRS)
def test_a_sequence_does_not_depend_on_the_tile_height(B, H):
    """The k order of a sequence's dot products and the order of its partial sums are the same in every instantiation: the
    first five sequences of a launch at tile height 4 (B = 769) equal, bit for bit, forward and backward, a launch of those
    five alone (height 2).

    At height 8 (B = 2053) they do not, and the two launches are held to the float bounds instead (each against the other; each
    also meets them against float64 in test_recurrence_matches_float64_reference).  Measured: at H = 32 and 64 the forward is bit-equal and 9 % of dgates differ in
    their last bits; at H = 128, 25 % of y and, chained after it, 28 % of dgates do (the test prints the counts: pytest -s).  The
    instantiations differ in floating-point contraction alone.  The owner lanes of height 8 carry two (sequence, unit) pairs,
    the compiler packs products of the two-pair code into two-wide multiplies (v_pk_mul_f32), and a product that went into a
    pair is no longer fused with the add that follows it: in the assembly of lstm_bwd_kernel<32, 2> ``1.f - tc * tc`` is one
    v_fma_f32 (-tc, tc, 1.0), in lstm_bwd_kernel<32, 8> tc * tc is half of a v_pk_mul_f32 followed by v_sub_f32; the tanh
    sequence in front of it is instruction for instruction the same, and the dot products are explicit fmaf in one k order.  Built with -ffp-contract=off, height 8 equals height 2 bit for bit at every H, forward and backward."""
    case = next(c for c in LC.RCASES if (c.B, c.H, c.bias) == (B, H, 'both'))
    n, T = LC.TILE_SMALL, case.T
    assert LC.tile(B) != LC.tile(n)
    inp = LC.rinputs(case)
    big, small = _to_dev(inp), _to_dev(inp, rows=n)
    fb, fs = _forward(big, B, T, H, case.name), _forward(small, n, T, H, case.name + ' alone')
    db = _backward(big, fb['gates'], fb['cell'], B, T, H, case.name)
    ds = _backward(small, fs['gates'], fs['cell'], n, T, H, case.name + ' alone')
    pairs = [('y', fb['y'][:n], fs['y'])] + [(k, fb[k][:, :n], fs[k]) for k in ('gates', 'cell', 'hprev')] + [('dgates', db[:, :n], ds)]
    for k, a, b in pairs:
        differ = int((_bits(a) != _bits(b)).sum())
        print('TILE %s %s: %d of %d elements differ in their bits' % (case.name, k, differ, a.numel()))
        if LC.tile(B) == 4:
            _same_bits(a, b, k)
        else:
            _compare('float', a, b.cpu().double(), 'tile_height', '%s %s against height 2' % (case.name, k),
                     GRAD_NORM_TOL if k == 'dgates' else OUT_NORM_TOL)


# ---- the row GEMMs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.GCASES, ids=_ids)
def test_row_gemm_matches_float64_reference(case):
    """sgnn_rows_gemm (out of every direction, x_copy bit-equal to the gathered rows) and sgnn_rows_gemm_nt: bit for bit on
    the grid, within the float bounds else; every word of out and x_copy written and nothing around them."""
    ops, lib = _ops(), _lib()
    P, st = ops._ptr, ops._stream()
    inp = LC.ginputs(case)
    ref = LC.gemm_ref(case, inp)
    R, K, N = case.R, case.K, case.N
    W = [w.to(DEV) for w in inp['W']]
    assert all(w.is_contiguous() for w in W)
    if case.op == 'nt':
        A = inp['A'].to(DEV)
        assert tuple(A.shape) == (2, R, K) and all(tuple(w.shape) == (K, N) for w in W) and len(W) == 2
        out = _Guarded(R * N, (R, N))
        rc = lib.sgnn_rows_gemm_nt(P(A), R, K, P(W[0]), P(W[1]), N, P(out.t), st)
        torch.cuda.synchronize()
        assert rc == 0
        out.check(case.name + ' out', True)
        _compare(case.kind, out.t, ref, 'rows_gemm_nt', case.name, GRAD_NORM_TOL)
        return
    X = inp['X'].to(DEV)
    ids = None if inp['ids'] is None else inp['ids'].to(DEV)
    b = [None] * 2 if inp['b'] is None else [v.to(DEV) for v in inp['b']] + [None]
    ldx = K + case.pad
    assert X.shape[1] == ldx and X.shape[0] == (LC.TABLE_ROWS if case.ids else R) and all(tuple(w.shape) == (N, K) for w in W)
    assert ids is None or (ids.shape == (R,) and 0 <= int(ids.min()) and int(ids.max()) < X.shape[0])
    out = _Guarded(case.dirs * R * N, (case.dirs, R, N))
    xc = _Guarded(R * K, (R, K)) if case.copy else None
    rc = lib.sgnn_rows_gemm(P(X), P(ids), ldx, R, K, P(W[0]), P(W[1]) if case.dirs == 2 else None, P(b[0]), P(b[1]), N, P(out.t),
                            P(xc.t) if xc is not None else None, st)
    torch.cuda.synchronize()
    assert rc == 0
    out.check(case.name + ' out', True)
    _compare(case.kind, out.t, ref, 'rows_gemm_' + LC.gemm_form(K)[0], case.name, OUT_NORM_TOL)
    if xc is not None:
        xc.check(case.name + ' x_copy', True)
        _same_bits(xc.t.cpu(), LC.gathered(case, inp), case.name + ' x_copy')


# ---- the tails ------------------------------------------------------------------------------------------------------------------------
def _tail(case, inp):
    """sgnn_lstm_tail_fwd, then sgnn_lstm_tail_bwd on the s the forward kept -> {'s', 'X', 'dy', 'dW' or None, 'db' or None}."""
    ops, lib = _ops(), _lib()
    P, st = ops._ptr, ops._stream()
    n, nw, T, H2, D = case.P, case.n_walks, case.T, case.H2, case.D
    y, W, dX = inp['y'].to(DEV), inp['W'].to(DEV), inp['dX'].to(DEV)
    b = None if inp['b'] is None else inp['b'].to(DEV)
    assert tuple(y.shape) == (n * nw, T, H2) and tuple(W.shape) == (D, H2) and tuple(dX.shape) == (n, D)
    g = {'s': _Guarded(n * H2, (n, H2)), 'X': _Guarded(n * D, (n, D)), 'dy': _Guarded(n * nw * T * H2, (n * nw, T, H2)),
         'dW': _Guarded(D * H2, (D, H2)), 'db': _Guarded(D, (D,))}
    rc = lib.sgnn_lstm_tail_fwd(P(y), n, nw, T, H2, case.last_only, P(W), P(b), D, P(g['s'].t), P(g['X'].t), st)
    torch.cuda.synchronize()
    assert rc == 0
    for k in ('s', 'X'):
        g[k].check('%s %s' % (case.name, k), True)
    for k in ('dy', 'dW', 'db'):
        g[k].check('%s %s after the forward' % (case.name, k), False)
    rc = lib.sgnn_lstm_tail_bwd(P(dX), P(g['s'].t), n, nw, T, H2, case.last_only, P(W), D, P(g['dy'].t),
                                P(g['dW'].t) if case.dW else None, P(g['db'].t) if case.db else None, st)
    torch.cuda.synchronize()
    assert rc == 0
    g['dy'].check(case.name + ' dy', True)
    g['dW'].check(case.name + ' dW_lin', case.dW)
    g['db'].check(case.name + ' db_lin', case.db)
    return {k: (v.t if k in ('s', 'X', 'dy') or getattr(case, k) else None) for k, v in g.items()}


@pytest.mark.parametrize('case', LC.TCASES, ids=_ids)
def test_tail_matches_float64_reference(case):
    """s, X, dy, dW_lin and db_lin: bit for bit on the grid, within the float bounds else; with last_only dy is +0.0 off the
    last step; a gradient that is not asked for (NULL) is not written, the others are all the same."""
    inp = LC.tinputs(case)
    ref = LC.tail_ref(case, inp)
    got = _tail(case, inp)
    for k in ('s', 'X', 'dy', 'dW', 'db'):
        if got[k] is not None:
            fwd = k in ('s', 'X')
            _compare(case.kind, got[k], ref[k], 'lstm_tail_fwd' if fwd else 'lstm_tail_bwd', '%s %s' % (case.name, k),
                     OUT_NORM_TOL if fwd else GRAD_NORM_TOL)
    if case.last_only and case.T > 1:
        assert int((_bits(got['dy'][:, :-1]) != 0).sum()) == 0, 'dy off the last step is not +0.0'


# ---- calls that are refused, calls with nothing to do ----------------------------------------------------------------------------
def test_refused_and_empty_calls_write_nothing():
    """Every argument error of the entries, with real device tensors large enough for the call had it been taken: the code
    the header names comes back and every output keeps its bytes.  (The forward tail holds H2 floats in LDS and refuses
    H2 > 8192, the backward tail D floats and refuses D > 8192.)  Calls over no sequence, no step, no row or no patch return
    SGNN_OK and write nothing either."""
    ops, lib = _ops(), _lib()
    from subgnn_amd._lib import ERRORS
    P, st = ops._ptr, ops._stream()
    rnd = lambda *s: torch.randn(*s, generator=torch.Generator().manual_seed(sum(s))).to(DEV)
    B, T, H = 3, 2, 64                                                # the allocation of the recurrence calls (H = 48 needs less)
    pre_x, whh, bhh, dy = rnd(2, B, T, 4 * H), [rnd(4 * H, H), rnd(4 * H, H)], [rnd(4 * H), rnd(4 * H)], rnd(B, T, 2 * H)
    gates_in, cell_in = rnd(2, B, T, 4 * H), rnd(2, B, T, H)
    y, gates, cell, hprev, dgates = (_Guarded(n) for n in (B * T * 2 * H, 2 * B * T * 4 * H, 2 * B * T * H, 2 * B * T * H, 2 * B * T * 4 * H))
    R, K, N = 5, 16, 8                                                # the GEMM calls: X (R, 32) is wide enough for every K and ldx below
    X, Wg, bg, A, Wn = rnd(R, 32), [rnd(N, 32), rnd(N, 32)], [rnd(N), rnd(N)], rnd(2, R, 32), [rnd(32, N), rnd(32, N)]
    out, xc, dx = _Guarded(2 * R * N), _Guarded(R * 32), _Guarded(R * N)
    big = LC.TAIL_MAX + 1                                             # the tails: one patch, one walk, one step
    ty, tW, tdX, ts = rnd(1, 1, big), rnd(big), rnd(1, big), rnd(1, big)
    s_out, Xo, tdy, tdW, tdb = (_Guarded(big) for _ in range(5))
    written = (y, gates, cell, hprev, dgates, out, xc, dx, s_out, Xo, tdy, tdW, tdb)

    def fwd(B_, T_, H_):
        return lib.sgnn_lstm_fwd(P(pre_x), P(whh[0]), P(whh[1]), P(bhh[0]), P(bhh[1]), B_, T_, H_, P(y.t), P(gates.t), P(cell.t), P(hprev.t), st)

    def bwd(B_, T_, H_):
        return lib.sgnn_lstm_bwd(P(whh[0]), P(whh[1]), P(gates_in), P(cell_in), P(dy), B_, T_, H_, P(dgates.t), st)

    def gemm(R_=R, K_=K, N_=N, ldx=32):
        return lib.sgnn_rows_gemm(P(X), None, ldx, R_, K_, P(Wg[0]), P(Wg[1]), P(bg[0]), P(bg[1]), N_, P(out.t), P(xc.t), st)

    def nt(R_=R, K_=K, N_=N, W1=Wn[1]):
        return lib.sgnn_rows_gemm_nt(P(A), R_, K_, P(Wn[0]), P(W1), N_, P(dx.t), st)

    def tail_fwd(n, H2, D):
        return lib.sgnn_lstm_tail_fwd(P(ty), n, 1, 1, H2, 1, P(tW), None, D, P(s_out.t), P(Xo.t), st)

    def tail_bwd(n, H2, D):
        return lib.sgnn_lstm_tail_bwd(P(tdX), P(ts), n, 1, 1, H2, 1, P(tW), D, P(tdy.t), P(tdW.t), P(tdb.t), st)

    calls = [
        ('lstm_fwd, H = 48', lambda: fwd(B, T, 48), UNSUPPORTED_D),
        ('lstm_bwd, H = 48', lambda: bwd(B, T, 48), UNSUPPORTED_D),
        ('lstm_fwd, H = 256', lambda: fwd(1, 1, 256), UNSUPPORTED_D),
        ('rows_gemm, K = 4', lambda: gemm(K_=4), BAD_ARG),
        ('rows_gemm, K = 0', lambda: gemm(K_=0), BAD_ARG),
        ('rows_gemm, K = 12', lambda: gemm(K_=12), BAD_ARG),
        ('rows_gemm, K = 20', lambda: gemm(K_=20), BAD_ARG),
        ('rows_gemm, ldx = 8 < K', lambda: gemm(ldx=8), BAD_ARG),
        ('rows_gemm, ldx = 18', lambda: gemm(ldx=18), BAD_ARG),
        ('rows_gemm, N = 0', lambda: gemm(N_=0), BAD_ARG),
        ('rows_gemm_nt, K = 8', lambda: nt(K_=8), BAD_ARG),
        ('rows_gemm_nt, K = 24', lambda: nt(K_=24), BAD_ARG),
        ('rows_gemm_nt, W1 null', lambda: nt(W1=None), BAD_ARG),
        ('rows_gemm_nt, N = 0', lambda: nt(N_=0), BAD_ARG),
        ('lstm_tail_fwd, H2 = 8193', lambda: tail_fwd(1, big, 1), BAD_ARG),
        ('lstm_tail_bwd, D = 8193', lambda: tail_bwd(1, 1, big), BAD_ARG),
        ('lstm_fwd, B = 0', lambda: fwd(0, T, H), 0),
        ('lstm_fwd, T = 0', lambda: fwd(B, 0, H), 0),
        ('lstm_bwd, B = 0', lambda: bwd(0, T, H), 0),
        ('lstm_bwd, T = 0', lambda: bwd(B, 0, H), 0),
        ('rows_gemm, R = 0', lambda: gemm(R_=0), 0),
        ('rows_gemm_nt, R = 0', lambda: nt(R_=0), 0),
        ('lstm_tail_fwd, no patch', lambda: tail_fwd(0, 1, 1), 0),
        ('lstm_tail_bwd, no patch', lambda: tail_bwd(0, 1, 1), 0),
    ]
    for what, call, want in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == want, '%s: %s, not %s' % (what, ERRORS.get(rc, rc), ERRORS.get(want, want))
        for t in written:
            t.check(what, False)


# ---- through ops ------------------------------------------------------------------------------------------------------------------------
def _lstm_params(m):
    return [getattr(m, '%s_l0%s' % (n, sfx)) for sfx in ('', '_reverse') for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


@pytest.mark.parametrize('route', ['layer', 'fused', 'fused-ids'])
@pytest.mark.parametrize('B,T,H,I', [(770, 2, 64, 40), (2050, 2, 32, 32)])
def test_layers_through_ops_match_nn_lstm_in_float64(B, T, H, I, route):
    """ops.bilstm_layer and ops.bilstm_layer_fused (dense, and with the embedding lookup as its operand load) at tile heights
    4 and 8 with ragged last tiles, I = 40 included: the output, dx or the table's gradient (PAD row 0 takes none) and all
    eight parameter gradients against nn.LSTM(bidirectional=True).double() on the CPU."""
    ops = _ops()
    assert LC.tile(B) in (4, 8) and B % LC.tile(B) != 0 and ops.lstm_fused_supported(I, H)
    torch.manual_seed(B + H + I)
    ref = torch.nn.LSTM(I, H, num_layers=1, batch_first=True, bidirectional=True)
    params = [p.detach().clone().to(DEV).requires_grad_() for p in _lstm_params(ref)]
    ref = ref.double()
    go = torch.randn(B, T, 2 * H)
    if route == 'fused-ids':
        n_rows = 301
        table = torch.randn(n_rows, I) * 0.5
        table[0] = 0
        ids = torch.randint(0, n_rows, (B, T))
        ids[0, 0], ids[1, 0], ids[2] = 0, n_rows - 1, ids[3]                          # PAD, the last row, repeated ids
        leaf = table.double().requires_grad_()
        yr, _ = ref(leaf[ids])
        src = table.to(DEV).requires_grad_()
        y = ops.bilstm_layer_fused(src, params, ids=ids.to(DEV))
    else:
        x = torch.randn(B, T, I)
        leaf = x.double().requires_grad_()
        yr, _ = ref(leaf)
        src = x.to(DEV).requires_grad_()
        y = ops.bilstm_layer(src, params) if route == 'layer' else ops.bilstm_layer_fused(src, params)
    (yr * go.double()).sum().backward()
    (y * go.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    what = '%s %d-%d-%d-%d' % (route, B, T, H, I)
    _compare('float', y.detach(), yr.detach(), 'ops_' + route, what + ' y', OUT_NORM_TOL)
    want = leaf.grad.clone()
    if route == 'fused-ids':
        assert float(src.grad[0].abs().max()) == 0.0
        want[0] = 0
    _compare('float', src.grad, want, 'ops_' + route, what + ' d input', GRAD_NORM_TOL)
    for p, q, nm in zip(params, _lstm_params(ref), ('w_ih', 'w_hh', 'b_ih', 'b_hh', 'w_ih_r', 'w_hh_r', 'b_ih_r', 'b_hh_r')):
        _compare('float', p.grad, q.grad, 'ops_' + route, '%s d %s' % (what, nm), GRAD_NORM_TOL)


@pytest.mark.parametrize('last', [0, 1])
def test_tail_through_ops(last):
    """ops.lstm_tail at (3, 2, 3, 260, 300): second trips of the loops over H2 and D, D H2 off a multiple of 256."""
    ops = _ops()
    case = next(c for c in LC.TCASES if c.kind == 'float' and (c.P, c.n_walks, c.T, c.H2, c.D, c.last_only) == (3, 2, 3, 260, 300, last))
    inp = LC.tinputs(case)
    ref = LC.tail_ref(case, inp)
    y, W, b = (inp[k].to(DEV).requires_grad_() for k in ('y', 'W', 'b'))
    X = ops.lstm_tail(y, W, b, case.n_walks, last_only=bool(last))
    (X * inp['dX'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _compare('float', X.detach(), ref['X'], 'ops_tail', case.name + ' X', OUT_NORM_TOL)
    for t, k in ((y, 'dy'), (W, 'dW'), (b, 'db')):
        _compare('float', t.grad, ref[k], 'ops_tail', '%s %s' % (case.name, k), GRAD_NORM_TOL)

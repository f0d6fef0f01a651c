"""Without a GPU: the calls of tests/test_gpu_lstm.py reach every tile height of the recurrence with full and ragged last tiles on
both sides of both thresholds, both launch forms of sgnn_rows_gemm with and without a chunk tail, and the tails' second loop
trips; the constants lstm_cases restates are the ones written in lstm.hip and ops.py; lstm_ref is nn.LSTM in float64; the grid
inputs make every result independent of the order of every sum; and the float inputs meet the GPU test's bounds when the same
operation is evaluated in float32 on the CPU.

Measured float32-on-CPU errors against float64 (element-wise helpers.rel_err / whole-tensor helpers.norm_err), i.e. what the
bounds REL_TOL = 1e-4 and 1e-5 (forward) / 2e-5 (gradients) have to leave room for:
    recurrence   y, gates, cell, hprev 1.6e-5 / 2.5e-7;  dgates 5.9e-6 / 1.8e-7 fed, 7.2e-6 / 2.2e-7 chained
    rows_gemm    1.7e-5 / 4.3e-7        rows_gemm_nt   1.7e-5 / 4.4e-7
    tails        forward 5.0e-6 / 2.1e-7,  backward 1.0e-5 / 5.8e-7
(the two tests below print them: pytest -s)"""
import os
import re

import pytest
import torch

import lstm_cases as LC
from helpers import REL_TOL, assert_close, norm_err, rel_err

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
OUT_NORM_TOL, GRAD_NORM_TOL = 1e-5, 2e-5         # the bounds of tests/test_gpu_lstm.py
_ids = lambda c: c.name
FORWARD = ('y', 'gates', 'cell', 'hprev')


def test_case_names_are_unique():
    for cases in (LC.RCASES, LC.GCASES, LC.TCASES):
        names = [c.name for c in cases]
        assert len(set(names)) == len(names)
    assert 20 <= sum(c.op == 'gemm' for c in LC.GCASES) <= 30 and 10 <= sum(c.op == 'nt' for c in LC.GCASES) <= 14


def test_constants_are_the_sources():
    src = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'lstm.hip')).read()
    ops_src = open(os.path.join(REPO, 'subgnn_amd', 'ops.py')).read()
    for line, count in (
            ('static int lstm_tile(int64_t B) { return B >= %d ? 8 : (B >= %d ? 4 : 2); }' % (LC.TILE8_FROM, LC.TILE4_FROM), 1),
            ('return (hidden_size == 128 || hidden_size == 64 || hidden_size == 32) ? 1 : 0;', 1),
            ('#define LSTM_KC %d\n' % LC.KC, 1),
            ('if (K >= %d && K %% %d == 0)\n        hipLaunchKernelGGL(rows_gemm_ksplit_kernel,' % (LC.KSPLIT_FROM, LC.KSPLIT_MULTIPLE), 1),
            ('constexpr int OWN = (BT * H + G - 1) / G;', 2),                               # forward and backward
            ('constexpr int G = 4 * H;', 2),
            ('const int Kh = K / 2;', 1), ('const int Kq = K / 8,', 1), ('const int Kh = K / 4;', 1),
            ('if (kc + 4 * c < Kh)', 2), ('if (kc + 4 * c < Kq)', 1),                      # the chunk-tail guards
            ('K < 8 || K % 8 != 0 || N < 1 || ldx < K || ldx % 4 != 0) return SGNN_ERR_BAD_ARG;', 1),
            ('K < 16 || K % 16 != 0 || N < 1) return SGNN_ERR_BAD_ARG;', 1),
            ('H2 > %d || D < 1) return SGNN_ERR_BAD_ARG;' % LC.TAIL_MAX, 1),
            ('D < 1 || D > %d) return SGNN_ERR_BAD_ARG;' % LC.TAIL_MAX, 1),
            ('c < H2; c += %d)' % LC.TAIL_STRIDE, 2), ('d < D; d += %d)' % LC.TAIL_STRIDE, 3)):
        assert src.count(line) == count, line
    assert sorted(int(h) for h in re.findall(r'hidden_size == (\d+)', src.split('sgnn_lstm_supported(int64_t hidden_size)')[1]
                                             .split('}')[0])) == sorted(LC.HIDDEN)
    assert re.search(r'^LSTM_OWN_GEMM_MAX_H = %d\b' % LC.OWN_GEMM_MAX_H, ops_src, re.M)
    assert [LC.tile(B) for B in (1, 767, 768, 2047, 2048, 10 ** 6)] == [2, 2, 4, 4, 8, 8]
    assert [[LC.own(H, BT) for BT in (2, 4, 8)] for H in LC.HIDDEN] == [[1, 1, 2]] * 3
    assert LC.gemm_form(120) == ('single', 60, True) and LC.gemm_form(128) == ('ksplit', 16, False)
    assert LC.gemm_form(136) == ('single', 68, True) and LC.gemm_form(160) == ('ksplit', 20, True)
    assert LC.gemm_form(64) == ('single', 32, False) and LC.gemm_form(256) == ('ksplit', 32, False)


def test_recurrence_cases_reach_every_tile_form():
    for H in LC.HIDDEN:
        here = [c for c in LC.RCASES if c.H == H]
        plain = {c.B for c in here if c.bias == 'both'}
        # both sides of both thresholds
        assert plain >= {LC.TILE4_FROM - 1, LC.TILE4_FROM, LC.TILE4_FROM + 1, LC.TILE8_FROM - 1, LC.TILE8_FROM, LC.TILE8_FROM + 1}
        for BT in (2, 4, 8):
            at = [c.B for c in here if LC.tile(c.B) == BT and c.bias == 'both']
            assert any(B % BT == 0 for B in at), (H, BT)              # a full last tile ...
            assert any(B % BT != 0 for B in at), (H, BT)                          # ... and a ragged one
            assert {c.bias for c in here if LC.tile(c.B) == BT} == {'both', 'none', 'fwd'}, (H, BT)
        # every count of valid sequences in a ragged last tile of height 4; at height 8 one (slot 1 empty) and five (slot 1 partly valid)
        assert {B % 4 for B in plain if LC.tile(B) == 4} >= {0, 1, 3}
        assert {B % 8 for B in plain if LC.tile(B) == 8} >= {0, 1, 5}
        assert any(LC.own(H, LC.tile(B)) == 2 and 4 < B % 8 < 8 for B in plain), 'no partly valid second owner slot'
        assert {c.T for c in here} >= {1, 2, 3, 4, 20}
    for B in LC.TILE_PAIRS:
        assert LC.tile(B) != LC.tile(LC.TILE_SMALL) and all(any(c.B == B and c.H == H for c in LC.RCASES) for H in LC.HIDDEN)
    assert {LC.tile(B) for B in LC.TILE_PAIRS} == {4, 8} and LC.tile(LC.TILE_SMALL) == 2
    assert max(c.B * c.T * c.H for c in LC.RCASES) == 2053 * 3 * 128                      # nothing larger: the tests stay quick


def test_gemm_cases_reach_both_forms_and_every_edge():
    gemm = [c for c in LC.GCASES if c.op == 'gemm']
    nt = [c for c in LC.GCASES if c.op == 'nt']
    assert {c.K for c in gemm} == {8, 24, 40, 64, 72, 120, 128, 136, 160, 256}
    assert {c.K for c in nt} == {16, 48, 80, 128, 256, 512}
    assert {c.N for c in LC.GCASES} == {1, 31, 32, 33, 40, 128, 512} and {c.N for c in nt} >= {1, 31, 32, 33, 40, 128}
    for cases in (gemm, nt):
        assert {c.R for c in cases} == {1, 31, 32, 33, 65}
    for kind in ('grid', 'float'):
        forms = {LC.gemm_form(c.K)[::2] for c in gemm if c.kind == kind}
        assert forms == {('single', False), ('single', True), ('ksplit', False), ('ksplit', True)}, kind
        assert {LC.gemm_nt_form(c.K)[1] for c in nt if c.kind == kind} == {False, True}
        # the switch with other things equal
        at = lambda K: {c._replace(name='', K=0, seed=0) for c in gemm if c.K == K and c.kind == kind}
        assert at(120) & at(128), kind
        assert {c.dirs for c in gemm if c.kind == kind} == {1, 2} and {c.bias for c in gemm if c.kind == kind} == {True, False}
        assert {c.pad for c in gemm if c.kind == kind} == {0, 4}
        assert {(c.ids, c.copy) for c in gemm if c.kind == kind} == {(False, False), (False, True), (True, False), (True, True)}
    g = lambda K: {c._replace(name='', K=0, seed=0) for c in gemm if c.K == K and c.kind == 'grid'}
    assert g(120) & g(128) & g(136) & g(160)
    for c in gemm:
        inp = LC.ginputs(c)
        assert inp['X'].shape[1] == c.K + c.pad and (c.pad == 0 or bool((inp['X'][:, c.K:] == LC.PAD_VALUE).all()))
        if c.ids:
            ids = inp['ids']
            assert ids.dtype == torch.int64 and ids.shape == (c.R,) and int(ids.min()) >= 0 and int(ids.max()) == LC.TABLE_ROWS - 1
            if c.R >= 3:
                assert int(ids.min()) == 0 and len(set(ids.tolist())) < c.R                # first row, last row, a repeated id
    assert any(c.ids and c.R >= 3 for c in gemm)
    # a product shape: K = 40 into N = 4 H, and the input gradient back to N = 40 from K = 4 H = 256
    assert any(c.K == 40 and c.N == 128 and c.ids and c.copy for c in gemm) and any(c.K == 256 and c.N == 40 for c in nt)


def test_tail_cases_take_second_trips_and_every_null():
    shapes = {(c.P, c.n_walks, c.T, c.H2, c.D) for c in LC.TCASES}
    assert shapes == set(LC.TAIL_SHAPES) and (1, 1, 1, 2, 1) in shapes
    for shape in LC.TAIL_SHAPES:
        assert {(c.kind, c.last_only) for c in LC.TCASES if (c.P, c.n_walks, c.T, c.H2, c.D) == shape and c.bias and c.dW and c.db} \
            == {('grid', 0), ('grid', 1), ('float', 0), ('float', 1)}
    assert any(c.H2 > LC.TAIL_STRIDE and c.D > LC.TAIL_STRIDE for c in LC.TCASES)          # second trips of both strided loops
    assert any((c.D * c.H2) % 256 != 0 for c in LC.TCASES) and any(c.D * c.H2 > 256 and (c.D * c.H2) % 256 != 0 for c in LC.TCASES)
    assert any(c.n_walks == 1 and c.T == 1 for c in LC.TCASES)
    assert any(not c.bias for c in LC.TCASES) and any(not c.dW for c in LC.TCASES) and any(not c.db for c in LC.TCASES)


# ---- the reference is the LSTM --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,I,B,T', [(32, 24, 5, 4), (64, 40, 3, 1), (32, 32, 2, 7)])
def test_lstm_ref_is_nn_lstm_in_float64(H, I, B, T):
    """y, dx, and the weight and bias gradients of both directions, put together from lstm_ref's dgates and hprev the way
    include/subgnn_hip.h tells the caller to, against nn.LSTM(bidirectional=True).double() and autograd."""
    torch.manual_seed(H + I + B + T)
    m = torch.nn.LSTM(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, T, 2 * H, dtype=torch.float64)
    yr, _ = m(x)
    (yr * dy).sum().backward()
    P = lambda n, d: getattr(m, n + '_l0' + ('_reverse' if d else ''))
    x2 = x.detach().reshape(B * T, I)
    pre_x = torch.stack([(x2 @ P('weight_ih', d).detach().t() + P('bias_ih', d).detach()).view(B, T, 4 * H) for d in (0, 1)])
    whh = torch.stack([P('weight_hh', d).detach() for d in (0, 1)])
    r = LC.lstm_ref(pre_x, whh, [P('bias_hh', d).detach() for d in (0, 1)], dy)
    close = lambda a, b, what: assert_close(a, b, what, tol=1e-12)
    close(r['y'], yr.detach(), 'y')
    dG = r['dgates'].view(2, B * T, 4 * H)
    close((dG[0] @ P('weight_ih', 0).detach() + dG[1] @ P('weight_ih', 1).detach()).view(B, T, I), x.grad, 'dx')
    for d in (0, 1):
        close(dG[d].t() @ x2, P('weight_ih', d).grad, 'dW_ih[%d]' % d)
        close(dG[d].t() @ r['hprev'][d].reshape(B * T, H), P('weight_hh', d).grad, 'dW_hh[%d]' % d)
        close(dG[d].sum(0), P('bias_ih', d).grad, 'db_ih[%d]' % d)
        close(dG[d].sum(0), P('bias_hh', d).grad, 'db_hh[%d]' % d)
    # the documented layout: hprev is 0 at a direction's first step and the direction's previous output else
    assert float(r['hprev'][0, :, 0].abs().max()) == 0.0 and float(r['hprev'][1, :, T - 1].abs().max()) == 0.0
    for t in range(1, T):
        assert torch.equal(r['hprev'][0, :, t], r['y'][:, t - 1, :H]) and torch.equal(r['hprev'][1, :, t - 1], r['y'][:, t, H:])
    # a null bias is a bias of zeros
    z = LC.lstm_ref(pre_x, whh, [None, torch.zeros(4 * H, dtype=torch.float64)], dy)
    n = LC.lstm_ref(pre_x, whh, [torch.zeros(4 * H, dtype=torch.float64), None], dy)
    assert all(torch.equal(z[k], n[k]) for k in z)


# ---- float32 on the CPU meets the bounds, grid inputs are exact -------------------------------------------------------------------
def _worst(worst, key, a, b):
    w = worst.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], rel_err(a, b)), max(w[1], norm_err(a, b))


def test_float32_recurrence_meets_the_gpu_bounds():
    worst = {}
    for case in LC.RCASES:
        inp, ref = LC.rinputs(case), LC.rreference(case)
        got = LC.lstm_ref(inp['pre_x'], inp['whh'], inp['bhh'], inp['dy'], dtype=torch.float32)
        for k in FORWARD:
            assert got[k].dtype == torch.float32
            assert_close(got[k], ref[k], '%s %s' % (case.name, k), tol=REL_TOL, norm_tol=OUT_NORM_TOL)
            _worst(worst, 'forward', got[k], ref[k])
        assert_close(got['dgates'], ref['dgates'], case.name + ' dgates chained', tol=REL_TOL, norm_tol=GRAD_NORM_TOL)
        _worst(worst, 'dgates chained', got['dgates'], ref['dgates'])
        # fed the float32-rounded reference activations, judged against float64 arithmetic on those same values
        g32, c32 = ref['gates'].float(), ref['cell'].float()
        fed = LC.lstm_bwd_ref(inp['whh'], g32, c32, inp['dy'], dtype=torch.float32)
        want = LC.lstm_bwd_ref(inp['whh'], g32, c32, inp['dy'])
        assert_close(fed, want, case.name + ' dgates fed', tol=REL_TOL, norm_tol=GRAD_NORM_TOL)
        _worst(worst, 'dgates fed', fed, want)
    for k, (e, n) in worst.items():
        print('recurrence %s: element-wise %.2e, norm %.2e' % (k, e, n))


def test_float32_gemms_and_tails_meet_the_gpu_bounds():
    worst = {}
    for case in LC.GCASES:
        if case.kind == 'float':
            inp = LC.ginputs(case)
            got, ref = LC.gemm_ref(case, inp, torch.float32), LC.gemm_ref(case, inp)
            bound = OUT_NORM_TOL if case.op == 'gemm' else GRAD_NORM_TOL
            assert_close(got, ref, case.name, tol=REL_TOL, norm_tol=bound)
            _worst(worst, case.op, got, ref)
    for case in LC.TCASES:
        if case.kind == 'float':
            inp = LC.tinputs(case)
            got, ref = LC.tail_ref(case, inp, torch.float32), LC.tail_ref(case, inp)
            for k in ('s', 'X', 'dy', 'dW', 'db'):
                fwd = k in ('s', 'X')
                assert_close(got[k], ref[k], '%s %s' % (case.name, k), tol=REL_TOL, norm_tol=OUT_NORM_TOL if fwd else GRAD_NORM_TOL)
                _worst(worst, 'tail forward' if fwd else 'tail backward', got[k], ref[k])
    for k, (e, n) in worst.items():
        print('%s: element-wise %.2e, norm %.2e' % (k, e, n))


def _integers(t):
    return t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= LC.GRID_MAX


def test_grid_float32_equals_float64():
    for case in LC.GCASES:
        if case.kind == 'grid':
            inp = LC.ginputs(case)
            ops = [inp['A']] + inp['W'] if case.op == 'nt' else [LC.gathered(case, inp)] + inp['W'] + (inp['b'] or [])
            assert all(_integers(t) for t in ops), case.name
            got, ref = LC.gemm_ref(case, inp, torch.float32), LC.gemm_ref(case, inp)
            assert got.dtype == torch.float32 and torch.equal(got.double(), ref), case.name
            assert float(ref.abs().max()) > 0
    for case in LC.TCASES:
        if case.kind == 'grid':
            inp = LC.tinputs(case)
            assert all(_integers(t) for t in inp.values() if t is not None), case.name
            got, ref = LC.tail_ref(case, inp, torch.float32), LC.tail_ref(case, inp)
            for k in ref:
                assert got[k].dtype == torch.float32 and torch.equal(got[k].double(), ref[k]), (case.name, k)
            if case.last_only and case.T > 1:
                assert float(ref['dy'][:, :-1].abs().max()) == 0.0 and float(ref['dy'][:, -1].abs().max()) > 0

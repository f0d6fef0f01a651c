"""-m gpu: the message-passing layer body (subgnn_amd/csrc/mpn.hip through ops.mpn) against the float64 CPU reference of
tests/mpn_cases.py, at every shape, flag and gradient choice its kernels and ops._MPN branch on
(tests/test_mpn_cases_host.py shows on the CPU which branch each case reaches).  The inputs lie on dyadic grids on which no
result depends on the order of a sum (mpn_cases.exact), so outputs and gradients are compared with ``torch.equal``: one
wrong, missing or doubled term fails.  Every case is exact (tests/test_mpn_cases_host.py asserts it): there is no tolerance."""
import collections
import ctypes

import pytest
import torch

import mpn_cases as MC
from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_MPN_LAUNCHING = ('sgnn_mpn_fwd', 'sgnn_mpn_fwd_many', 'sgnn_mpn_bwd', 'sgnn_mpn_bwd_edges', 'sgnn_mpn_bwd_edges_many',
                  'sgnn_mpn_bwd_wp_partial', 'sgnn_mpn_bwd_shared_det')


def _ops():
    from subgnn_amd import ops
    return ops


def _dev(t):
    return None if t is None else t.to(DEV)


class _Counting:
    """The loaded library, counting the calls of each entry."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        f = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] += 1
            return f(*a)
        return counted


def _run(ops, case):
    """One forward + backward of the case on the device -> ([(agg, z) per body], {leaf name: gradient or None})."""
    inp = MC.inputs(case)
    want = dict(MC.leaf_names(case))
    src = {'dense': ops.SRC_DENSE, 'gather': ops.SRC_GATHER, 'shared': ops.SRC_SHARED}[case.src]
    leaves = {'x': inp['x'].to(DEV).clone().requires_grad_(want['x'])}
    x = leaves['x']
    if case.tap is not None:
        x = ops.tap_table(x, half=inp['half'].half().to(DEV) if inp['half'] is not None else None)
    outs, loss = [], None
    with ops.deterministic(case.det):
        for k, b in enumerate(inp['bodies']):
            R, A = b['R'], b['A']
            wp = leaves['wp%d' % k] = b['wp'].to(DEV).clone().requires_grad_(want['wp%d' % k])
            bp = leaves['bp%d' % k] = b['bp'].to(DEV).clone().requires_grad_(want['bp%d' % k])
            sims, ids, rm, col = _dev(b['sims']), _dev(b['ids']), _dev(b['row_mask']), _dev(b['sim_col'])
            plan = None
            if case.plan:
                plan = ops.mpn_edge_plan(sims, ids, rm, R=R, A=A, D=case.D, max_key=case.N, id_div=case.id_div, sim_col=col,
                                         sims_per_edge=case.sel == 'edge')
            outs.append(ops.mpn(x, wp, bp, sims, src=src, R=R, A=A, ids=ids, id_div=case.id_div, edge_mask=_dev(b['edge_mask']),
                                row_mask=rm, sim_col=col, sims_per_edge=case.sel == 'edge', edge_plan=plan, relu_z=case.relu,
                                keep_chunks=bool(case.bodies), lazy=bool(case.bodies)))
        if case.bodies:
            assert ops.lazy_mpn_pending() == sum(1 for R, A in case.bodies if R and A)
            ops.flush_lazy_mpn()
            outs = [(agg.sum(0) if agg.dim() == 3 else agg, z) for agg, z in outs]      # the anchor-chunk partials, as update_layer adds them
    for (agg, z), b in zip(outs, inp['bodies']):
        for t, go, used in ((agg, b['gagg'], case.outs[0]), (z, b['gz'], case.outs[1])):
            if used and t.requires_grad:
                term = (t * go.to(DEV)).sum()
                loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
    torch.cuda.synchronize()
    return [(a.detach(), z.detach()) for a, z in outs], {n: t.grad for n, t in leaves.items()}


def _compare(got, ref, what):
    assert got.shape == ref.shape and got.dtype == torch.float32, what
    ref = ref.float().to(got.device)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d elements differ, the first at %r: got %.9g, want %.9g'
                             % (what, bad.shape[0], got.numel(), i, float(got[i]), float(ref[i])))


@pytest.mark.parametrize('case', MC.CASES, ids=lambda c: c.name)
def test_mpn_matches_float64_reference(case, monkeypatch):
    """agg, z and every requested gradient against mpn_cases.reference (float64, CPU), bit for bit; a gradient nobody can receive is None; row 0 of the table's gradient is zero; the call makes the library calls
    mpn_cases.entries says it makes; deterministic cases run twice and repeat their bits."""
    ops = _ops()
    from subgnn_amd import _lib
    for name, value in case.knobs:
        monkeypatch.setattr(ops, name, value)
    lib = _Counting(_lib.load())
    ref_out, ref_g = MC.reference(case)
    with monkeypatch.context() as mp:
        mp.setattr(_lib, 'load', lambda: lib)
        out, grads = _run(ops, case)
    assert {k: v for k, v in lib.calls.items() if k in _MPN_LAUNCHING} == dict(MC.entries(case))
    assert ops.lazy_mpn_pending() == 0
    for k, ((agg, z), (agg_r, z_r)) in enumerate(zip(out, ref_out)):
        _compare(agg, agg_r, '%s agg of body %d' % (case.name, k))
        _compare(z, z_r, '%s z of body %d' % (case.name, k))
    for name, _ in MC.leaf_names(case):
        if ref_g[name] is None:
            assert grads[name] is None, 'a gradient of %s where none can arrive' % name
            continue
        assert grads[name] is not None, 'no gradient of ' + name
        _compare(grads[name], ref_g[name].view_as(grads[name]), '%s gradient of %s' % (case.name, name))
    if case.src == 'gather' and grads['x'] is not None:
        assert float(grads['x'][0].abs().max()) == 0.0, 'the PAD row of the table received a gradient'
    if case.det:
        out2, grads2 = _run(ops, case)
        for (a, z), (a2, z2) in zip(out, out2):
            assert torch.equal(a, a2) and torch.equal(z, z2), 'an output differs between two runs'
        for name in grads:
            assert (grads[name] is None) == (grads2[name] is None)
            assert grads[name] is None or torch.equal(grads[name], grads2[name]), 'the gradient of %s differs between two runs' % name


def _poisoned(monkeypatch):
    """torch.empty hands out float32 device buffers filled with -7: a refused call must leave them as they are."""
    made, plain = [], torch.empty

    def empty_filled(*a, **k):
        t = plain(*a, **k)
        if t.is_cuda and t.dtype == torch.float32:
            made.append(t.fill_(-7.0))
        return t
    monkeypatch.setattr(torch, 'empty', empty_filled)
    return made


@pytest.mark.parametrize('D,kw,err', [(6, {}, 'SGNN_ERR_UNSUPPORTED_D'), (512, {}, 'SGNN_ERR_UNSUPPORTED_D'),
                                       (64, {'id_div': 0}, 'SGNN_ERR_BAD_ARG')], ids=['D=6', 'D=512', 'id_div=0'])
def test_mpn_check_refuses_before_any_launch(D, kw, err, monkeypatch):
    """mpn_check: a width that is not 4 x a power of two up to 256, or id_div < 1 -> SubgnnHipError from sgnn_mpn_fwd, and
    the output buffers keep their bytes."""
    ops = _ops()
    from subgnn_amd._lib import SubgnnHipError
    R, A, N = 9, 5, 20
    g = torch.Generator().manual_seed(D)
    E = torch.randn(N + 1, D, generator=g).to(DEV)
    ids = torch.randint(0, N + 1, (R, A), generator=g).to(DEV)
    sims = torch.rand(R, N, generator=g).to(DEV)
    wp, bp = torch.randn(D, generator=g).to(DEV), torch.zeros(1, device=DEV)
    with monkeypatch.context() as mp:
        made = _poisoned(mp)
        with pytest.raises(SubgnnHipError, match='sgnn_mpn_fwd failed: ' + err):
            ops.mpn(E, wp, bp, sims, src=ops.SRC_GATHER, R=R, A=A, ids=ids, **kw)
    torch.cuda.synchronize()
    assert sorted(t.numel() for t in made) == sorted([R * A, R * D]) and all((t == -7.0).all() for t in made)


def test_mpn_check_refuses_a_half_table_for_shared_anchors():
    """x_f16 is the GATHER table's: with SHARED anchors every entry returns SGNN_ERR_BAD_ARG (ops never builds such a call,
    so the library is called directly) and writes nothing."""
    ops = _ops()
    from subgnn_amd import _lib
    lib = _lib.load()
    R, A, D = 9, 5, 64
    g = torch.Generator().manual_seed(1)
    X, sims = torch.randn(A, D, generator=g).to(DEV), torch.rand(R, A, generator=g).to(DEV)
    wp, bp = torch.randn(D, generator=g).to(DEV), torch.zeros(1, device=DEV)
    a = ops._mpn_args(ops.SRC_SHARED, X, None, 1, None, None, sims, None, True, wp, bp, R, A, D)
    a.x_f16 = 1
    agg, z = torch.full((R, D), -7.0, device=DEV), torch.full((R, A), -7.0, device=DEV)
    gx, gwp = torch.full((A, D), -7.0, device=DEV), torch.full((D,), -7.0, device=DEV)
    ws = torch.empty(lib.sgnn_mpn_bwd_shared_det_workspace_bytes(R, A, D) // 4 + 1, device=DEV)
    assert lib.sgnn_mpn_fwd_chunks(ctypes.byref(a)) == 1
    for what, rc in (('sgnn_mpn_fwd', lib.sgnn_mpn_fwd(ctypes.byref(a), ops._ptr(agg), ops._ptr(z), ops._stream())),
                     ('sgnn_mpn_bwd', lib.sgnn_mpn_bwd(ctypes.byref(a), ops._ptr(agg), ops._ptr(z), ops._ptr(gx), ops._ptr(gwp), ops._stream())),
                     ('sgnn_mpn_bwd_shared_det', lib.sgnn_mpn_bwd_shared_det(ctypes.byref(a), ops._ptr(agg), ops._ptr(z), ops._ptr(gx), ops._ptr(gwp),
                                                                             None, ops._ptr(ws), ws.numel() * 4, ops._stream()))):
        with pytest.raises(_lib.SubgnnHipError, match=what + ' failed: SGNN_ERR_BAD_ARG'):
            _lib.check(rc, what)
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in (agg, z, gx, gwp))
    a.x_f16 = 0                                                      # the same arguments without the flag are taken
    _lib.check(lib.sgnn_mpn_fwd(ctypes.byref(a), ops._ptr(agg), ops._ptr(z), ops._stream()), 'sgnn_mpn_fwd')
    torch.cuda.synchronize()
    assert_close(agg, sims.double() @ X.double(), 'agg without the flag', norm_tol=1e-6)

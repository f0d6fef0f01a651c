"""-m gpu: the table-gradient scatter (subgnn_amd/csrc/scatter.hip through ops.scatter_add_rows, ops._GradAcc.flush and
ops.sort_edges_by_key) against the float64 CPU reference of tests/scatter_cases.py at every launch form, with constructed key
layouts for the carry protocol and repeated members for the ``arg`` mode (tests/test_scatter_cases_host.py shows on the CPU which
instantiation and which branches each case reaches), and its first producer, ops.cc_embed (subgnn_amd/csrc/embed.hip), against
oracle.float_half.cc_embeddings in float64.  ``grid`` cases are compared with torch.equal -- no result of theirs depends on the
order of a sum -- and ``float`` cases within the bounds of tests/test_gpu_float.py's scatter tests."""
import collections

import pytest
import torch

import scatter_cases as SC
from helpers import REL_TOL, assert_close
from oracle import float_half as FH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NORM_TOL = 1e-5                                  # tests/test_gpu_float.py's scatter tests
LIST_ARGS = ('G', 'edge_row', 'edges_per_row', 'c1', 'c2', 'v', 'arg')


def _ops():
    from subgnn_amd import ops
    return ops


def _lib():
    from subgnn_amd import _lib
    return _lib.load()


def _case(name):
    return next(c for c in SC.CASES if c.name == name)


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _counted(monkeypatch, lib, names):
    calls = collections.Counter()
    for name in names:
        def counted(*a, _f=getattr(lib, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def _scatter(ops, table, d, **kw):
    args = {k: d[k] for k in LIST_ARGS}
    if kw.get('together') is not None:
        assert args.pop('arg') is None
    return ops.scatter_add_rows(table, d['keys'], **args, **kw)


def _run(ops, case, presort=False):
    """The case's table after its lists on the device: a single list through ops.scatter_add_rows, the lists of a ``multi``
    case through an ops._GradAcc -- they wait for its flush and go through ONE sgnn_scatter_add_rows_multi."""
    inp = SC.inputs(case)
    lists = [_dev(d) for d in inp['lists']]
    table0 = inp['table0'].to(DEV)
    if case.family != 'multi':
        table = table0.clone()
        pre = ops.sort_edges_by_key(lists[0]['keys'], inp['n_rows'] - 1) if presort else None
        _scatter(ops, table, lists[0], presorted=pre)
        torch.cuda.synchronize()
        return table
    owner = torch.nn.Parameter(torch.zeros(inp['n_rows'], case.D, device=DEV))
    acc = ops._GradAcc(owner)
    buf = acc.buffer(tuple(owner.shape), torch.device(DEV))
    buf.copy_(table0)
    for d in lists:
        _scatter(ops, buf, d, together=acc)
    assert len(acc.jobs) == sum(1 for n in case.spec.sizes if SC.waits_for_flush(n, case.D))
    assert torch.equal(buf, table0), 'a pending list was added before the flush'
    with pytest.MonkeyPatch.context() as mp:
        calls = _counted(mp, _lib(), ('sgnn_scatter_add_rows_multi', 'sgnn_scatter_add_rows_sorted'))
        acc.flush()
    assert not acc.jobs and calls['sgnn_scatter_add_rows_multi'] == 1 and calls['sgnn_scatter_add_rows_sorted'] == 0
    torch.cuda.synchronize()
    return buf


def _compare(case, got, ref, what):
    assert got.shape == ref.shape and got.dtype == torch.float32, what
    if case.kind == 'grid':
        ref = ref.float().to(got.device)
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            i = tuple(int(v) for v in bad[0])
            raise AssertionError('%s: %d of %d elements differ (%d table rows), the first at %r: got %.9g, want %.9g'
                                 % (what, bad.shape[0], got.numel(), bad[:, 0].unique().numel(), i, float(got[i]), float(ref[i])))
    else:
        assert_close(got, ref, what, tol=REL_TOL, norm_tol=NORM_TOL)


# ---- the scatter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SC.CASES, ids=lambda c: c.name)
def test_scatter_matches_float64_reference(case):
    """The table after the case's lists against scatter_cases.reference (float64, CPU): bit for bit on the grid, within the
    float bounds else; a second run repeats the bits; the lists of a multi case scattered one after the other give the same
    table (the same bits on the grid)."""
    ops = _ops()
    ref = SC.reference(case)
    got = _run(ops, case)
    _compare(case, got, ref, case.name)
    again = _run(ops, case)
    assert torch.equal(got, again), '%s: two runs differ' % case.name
    if case.family == 'multi':
        inp = SC.inputs(case)
        one_by_one = inp['table0'].to(DEV).clone()
        for d in inp['lists']:
            _scatter(ops, one_by_one, _dev(d))
        _compare(case, one_by_one, ref, case.name + ' (one list after the other)')
        if case.kind == 'grid':
            assert torch.equal(got, one_by_one)


@pytest.mark.parametrize('name', ['boundaries-run16-D64-pad-1', 'boundaries-run64-D128-pad+1', 'arg-small-D64-div', 'arg-large-D64-list',
                                  'forms-65537-D64-float', 'forms-15-D64-float'])
def test_a_kept_order_gives_the_same_bits_as_sorting_inside(name):
    ops, case = _ops(), _case(name)
    a, b = _run(ops, case), _run(ops, case, presort=True)
    assert torch.equal(a, b)
    _compare(case, b, SC.reference(case), name)


def test_unsupported_width_is_refused_and_nothing_is_written():
    ops = _ops()
    from subgnn_amd._lib import SubgnnHipError
    D = SC.MAX_D + 1
    keys = torch.arange(1, 9, dtype=torch.int32, device=DEV)
    table = torch.ones(10, D, device=DEV)
    with pytest.raises(SubgnnHipError, match='SGNN_ERR_UNSUPPORTED_D'):
        ops.scatter_add_rows(table, keys, G=torch.ones(8, D, device=DEV))
    torch.cuda.synchronize()
    assert bool((table == 1).all())
    with pytest.raises(ValueError):
        SC.form(keys.numel(), D)


@pytest.mark.parametrize('case', SC.SORT_CASES, ids=lambda c: '%d-%d-%s' % c)
def test_sort_is_the_stable_sort(case):
    """sort_one_wg_kernel at every items-per-lane form, and with every key the value its padding ties with."""
    keys = SC.sort_keys(case)
    sk, order = _ops().sort_edges_by_key(keys.to(DEV), case.max_key)
    want_k, want_o = torch.sort(keys, stable=True)
    assert sk.dtype == torch.int32 and order.dtype == torch.int32
    assert torch.equal(sk.cpu(), want_k) and torch.equal(order.cpu().long(), want_o)


# ---- ops.cc_embed -------------------------------------------------------------------------------------------------------------------
CC_DIMS = (4, 8, 12, 64, 128, 256, 260)
NEG_IDS = (1, 2, 3)                              # table rows that are negative in every column
SPARE = 40                                       # an id no set lists (the arena's tail holds it)


@pytest.fixture(params=['sorted', 'atomics'])
def det(request):
    from subgnn_amd import ops
    ops.DETERMINISTIC = request.param == 'sorted'
    yield request.param
    ops.DETERMINISTIC = True


def _draw(g, kind, *shape):
    if kind == 'grid':
        return torch.randint(-SC.GRID_MAX, SC.GRID_MAX + 1, shape, generator=g).to(torch.float32)
    return torch.randn(*shape, generator=g)


def _cc_inputs(kind, D, seed, S=60, L=9):
    """(table (SPARE + 1, D) with row 0 = 0, padded sets (S, L), grad_out (S, D)).  Set 1 is empty, set 2 lists only rows that are
    negative everywhere over its full length (its max stays negative), set 3 does over 4 entries (its max is PAD's 0: no
    gradient), set 4 repeats a member; the others have random lengths, set 0 the full one.  Grid values are exact in half."""
    g = torch.Generator().manual_seed(seed)
    E = _draw(g, kind, SPARE + 1, D)
    E[0] = 0
    E[list(NEG_IDS)] = -1 - E[list(NEG_IDS)].abs().clamp(max=1)
    cc = torch.randint(1, SPARE, (S, L), generator=g)
    lens = torch.randint(0, L + 1, (S,), generator=g)
    cc[2:4] = torch.randint(1, 4, (2, L), generator=g)
    cc[4, :5] = torch.tensor([7, 8, 7, 9, 7])[:L]
    lens[:5] = torch.tensor([L, 0, L, 4, 5]).clamp(max=L)
    cc[torch.arange(L).view(1, L) >= lens.view(S, 1)] = 0
    return E, cc, _draw(g, kind, S, D)


def _cc_reference(table, cc, gout, agg):
    Ec = table.double().requires_grad_(True)
    ref = FH.cc_embeddings(Ec, cc.unsqueeze(1), agg).squeeze(1)
    (ref * gout.double()).sum().backward()
    return ref.detach(), Ec.grad


def _cc_compare(kind, got, ref, what):
    if kind == 'grid':
        ref = ref.float().to(got.device)
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            i = tuple(int(v) for v in bad[0])
            raise AssertionError('%s: %d elements differ, the first at %r: got %.9g, want %.9g' % (what, bad.shape[0], i, float(got[i]), float(ref[i])))
    else:
        assert_close(got, ref, what)


@pytest.mark.parametrize('kind', ['grid', 'float'])
@pytest.mark.parametrize('agg', ['sum', 'max'])
@pytest.mark.parametrize('D', CC_DIMS)
def test_cc_embed_matches_the_oracle(D, agg, kind, det, monkeypatch):
    """Forward and table gradient at every width class: one float4 per row, widths that are no multiple of 64, and D = 260, which
    the sorted backward does not take -- it goes to the atomics kernel whatever DETERMINISTIC says."""
    ops = _ops()
    E, cc, gout = _cc_inputs(kind, D, D)
    ref, ref_grad = _cc_reference(E, cc, gout, agg)
    assert float(ref[1].abs().max()) == 0.0                                  # the empty set
    if agg == 'max':                                                         # all-negative members: alone, and with padding behind them
        assert (ref[2] < 0).all() and float(ref[3].abs().max()) == 0.0 and float(ref_grad[list(NEG_IDS)].abs().max()) > 0
    calls = _counted(monkeypatch, _lib(), ('sgnn_cc_embed_bwd', 'sgnn_scatter_add_rows_sorted'))
    Eg = E.to(DEV).requires_grad_(True)
    out = ops.cc_embed(Eg, ops.Ragged.from_padded(cc.to(DEV)), agg, padded_len=cc.shape[1])
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    atomics = det == 'atomics' or D > SC.MAX_D
    assert (calls['sgnn_cc_embed_bwd'], calls['sgnn_scatter_add_rows_sorted']) == ((1, 0) if atomics else (0, 1))
    _cc_compare(kind, out, ref, 'cc_embed %s forward' % agg)
    _cc_compare(kind, Eg.grad, ref_grad, 'cc_embed %s gradient' % agg)
    assert float(Eg.grad[0].abs().max()) == 0.0 and float(Eg.grad[SPARE].abs().max()) == 0.0


@pytest.mark.parametrize('kind', ['grid', 'float'])
@pytest.mark.parametrize('agg', ['sum', 'max'])
@pytest.mark.parametrize('D', [8, 64, 256])
def test_cc_embed_reads_the_half_table_and_hands_the_gradient_to_the_fp32_one(D, agg, kind, det):
    """ops.tap_table(E, half=H) with H holding OTHER values than E: the output follows H (sgnn_cc_embed_fwd_f16), the gradient
    arrives in E.grad."""
    ops = _ops()
    E, cc, gout = _cc_inputs(kind, D, D + 1)
    H = _cc_inputs(kind, D, D + 2)[0].half()
    assert not torch.equal(H.float(), E)
    ref, ref_grad = _cc_reference(H, cc, gout, agg)
    Eg = E.to(DEV).requires_grad_(True)
    tapped = ops.tap_table(Eg, half=H.to(DEV))
    out = ops.cc_embed(tapped, ops.Ragged.from_padded(cc.to(DEV)), agg, padded_len=cc.shape[1])
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _cc_compare(kind, out, ref, 'cc_embed %s forward from the half table' % agg)
    _cc_compare(kind, Eg.grad, ref_grad, 'cc_embed %s gradient' % agg)
    assert float(Eg.grad[0].abs().max()) == 0.0


@pytest.mark.parametrize('kind', ['grid', 'float'])
@pytest.mark.parametrize('agg', ['sum', 'max'])
@pytest.mark.parametrize('how', ['stride', 'stride-presorted', 'arena'])
def test_cc_embed_backward_forms(how, agg, kind):
    """The fixed-stride sets (PAD entries are members; with and without a kept order) and ragged sets in a node arena longer than
    ptr[-1] whose tail holds a valid id: it receives no gradient."""
    ops = _ops()
    D = 64
    E, cc, gout = _cc_inputs(kind, D, 3)
    S, L = cc.shape
    ref, ref_grad = _cc_reference(E, cc, gout, agg)
    Eg = E.to(DEV).requires_grad_(True)
    if how == 'arena':
        lens = (cc != 0).sum(1)
        ptr = torch.zeros(S + 1, dtype=torch.int64)
        ptr[1:] = lens.cumsum(0)
        nodes = torch.cat([cc[cc != 0], torch.full((37,), SPARE)]).to(torch.int32)
        sets = ops.Ragged(ptr.to(DEV), nodes.to(DEV), max_len=L)
        out = ops.cc_embed(Eg, sets, agg, padded_len=L)
    else:
        nodes = cc.reshape(-1).to(torch.int32).to(DEV)
        sets = ops.Ragged((torch.arange(S + 1) * L).to(DEV), nodes, max_len=L)
        pre = ops.sort_edges_by_key(nodes, SPARE) if how == 'stride-presorted' else None
        out = ops.cc_embed(Eg, sets, agg, padded_len=L, stride=L, presorted=pre)
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _cc_compare(kind, out, ref, 'cc_embed %s forward (%s)' % (agg, how))
    _cc_compare(kind, Eg.grad, ref_grad, 'cc_embed %s gradient (%s)' % (agg, how))
    assert float(Eg.grad[SPARE].abs().max()) == 0.0 and float(Eg.grad[0].abs().max()) == 0.0


@pytest.mark.parametrize('agg', ['sum', 'max'])
def test_cc_embed_grid_stride_loop(agg, det):
    """33 000 sets of up to 2 members at D = 128: n_sets * D / 4 is just above the 4096 blocks x 256 lanes one pass covers."""
    ops = _ops()
    S, L, D = 33000, 2, 128
    assert S * D // 4 > 4096 * 256 > (S - 1000) * D // 4
    E, cc, gout = _cc_inputs('grid', D, 9, S=S, L=L)
    ref, ref_grad = _cc_reference(E, cc, gout, agg)
    Eg = E.to(DEV).requires_grad_(True)
    out = ops.cc_embed(Eg, ops.Ragged.from_padded(cc.to(DEV)), agg, padded_len=L)
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert float(ref_grad.abs().max()) < SC.EXACT_BELOW
    _cc_compare('grid', out, ref, 'cc_embed %s forward' % agg)
    _cc_compare('grid', Eg.grad, ref_grad, 'cc_embed %s gradient' % agg)


# ---- the max aggregator's ties ------------------------------------------------------------------------------------------------------
TIE_TABLE = [[0, 0, 0, 0], [1, -1, 0, -2], [1, -1, -1, -2], [-1, -1, 0, 0]]
TIE_SETS = [[1, 2, 0], [2, 1, 0], [1, 2, 3], [3, 0, 0]]
TIE_ARG = [[1, 0, 1, 0], [2, 0, 1, 0], [1, 1, 1, 3], [0, 0, 3, 3]]          # the member that gets column d's gradient (0: PAD, nobody)


def _tie_run(ops, table, half):
    E = torch.tensor(table, dtype=torch.float32)
    E = torch.cat([E, torch.zeros(E.shape[0], 4)], 1)                         # D = 8; the added columns are all ties
    cc = torch.tensor(TIE_SETS)
    gout = torch.arange(1, 4 * 8 + 1, dtype=torch.float32).view(4, 8)        # no two gradients are equal
    ref, ref_grad = _cc_reference(E, cc, gout, 'max')
    Eg = E.to(DEV).requires_grad_(True)
    src = ops.tap_table(Eg, half=E.half().to(DEV)) if half else Eg
    out = ops.cc_embed(src, ops.Ragged.from_padded(cc.to(DEV)), 'max', padded_len=cc.shape[1])
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.cpu(), Eg.grad.cpu(), ref, ref_grad, gout


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
def test_cc_embed_max_ties_go_where_the_oracle_sends_them(half, det):
    """Among members the first in set order gets the gradient; a member whose value is exactly 0 while the others are negative
    ties with the padding behind it and gets it too (x.max(dim) names the first maximal entry, the members come first); a
    column whose maximum is the padding's 0 alone gives no gradient."""
    out, grad, ref, ref_grad, gout = _tie_run(_ops(), TIE_TABLE, half)
    want = torch.zeros(4, 8, dtype=torch.float64)
    for s, row in enumerate(TIE_ARG):
        for d, member in enumerate(row + [TIE_SETS[s][0]] * 4):               # all-zero columns: the first member
            if member:
                want[member, d] += float(gout[s, d])
    assert torch.equal(ref_grad, want), 'the oracle is not what this test says it is'
    assert torch.equal(out.double(), ref)
    assert torch.equal(grad.double(), ref_grad), 'got\n%r\nwant\n%r' % (grad, ref_grad)


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
@pytest.mark.parametrize('agg', ['sum', 'max'])
def test_cc_embed_keeps_a_nan_member(agg, half):
    """A NaN in a member's row is a NaN in the set's output, as torch.max / torch.sum give it: first, in the middle and last in
    the set, with and without padding behind it -- a diverged table must not produce a finite loss."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    E = torch.randn(12, 8, generator=g)
    E[0] = 0
    E[5, 2], E[5, 6] = float('nan'), float('nan')
    cc = torch.tensor([[5, 1, 2, 3], [1, 5, 2, 3], [1, 2, 3, 5], [5, 1, 0, 0], [1, 5, 0, 0], [5, 0, 0, 0], [1, 2, 3, 4], [5, 5, 1, 0]])
    table = E.half().float() if half else E
    ref = FH.cc_embeddings(table.double(), cc.unsqueeze(1), agg).squeeze(1)
    assert ref[:6, [2, 6]].isnan().all() and ref.isnan().sum() == 14
    Eg = E.to(DEV)
    src = ops.tap_table(Eg, half=E.half().to(DEV)) if half else Eg
    with torch.no_grad():
        out = ops.cc_embed(src, ops.Ragged.from_padded(cc.to(DEV)), agg, padded_len=cc.shape[1]).cpu()
    assert torch.equal(out.isnan(), ref.isnan()), 'NaN outputs\n%r\nwant\n%r' % (out.isnan().nonzero().tolist(), ref.isnan().nonzero().tolist())
    fin = ~ref.isnan()
    assert_close(out[fin], ref[fin], 'the finite outputs')

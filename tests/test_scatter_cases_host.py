"""Without a GPU: the calls of tests/test_gpu_scatter.py reach every scatter_runs_kernel instantiation that scatter.hip's two
dispatch blocks name, every flush destination, the chain lengths around SC_AHEAD, a repeated member split by a run boundary at
both run lengths and every items-per-lane form of the one-workgroup sort -- said from scatter_cases.classify, a restatement of
the kernels' rules, so that a later change of SC_RUN or SC_AHEAD fails here instead of silently un-testing a branch.  The
constants scatter_cases restates are the ones in scatter.hip and ops.py, the grid inputs make every result independent of the
order of every sum, and the ``arg`` reference is what autograd gives for a max over a padded set."""
import os
import re

import pytest
import torch

import scatter_cases as SC
from helpers import REL_TOL, assert_close

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NORM_TOL = 1e-5                                  # the bound of tests/test_gpu_float.py's scatter tests
_ids = lambda c: c.name
GRID = [c for c in SC.CASES if c.kind == 'grid']
FLOAT = [c for c in SC.CASES if c.kind == 'float']


def _case(name):
    return next(c for c in SC.CASES if c.name == name)


def _source():
    return open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'scatter.hip')).read()


def test_case_names_are_unique():
    names = [c.name for c in SC.CASES]
    assert len(set(names)) == len(names)


def test_constants_are_the_sources():
    src = _source()
    defines = {k: int(v) for k, v in re.findall(r'^#define (SC_\w+) (\d+)\b', src, re.M)}
    mine = {'SC_RUN': SC.RUN, 'SC_RUN_SMALL': SC.RUN_SMALL, 'SC_SMALL_EDGES': SC.SMALL_EDGES, 'SC_AHEAD': SC.AHEAD, 'SC_MAXC': SC.MAXC,
            'SC_ONE_WG': SC.ONE_WG, 'SC_MAX_JOBS': SC.MAX_JOBS}
    assert {k: defines.get(k) for k in mine} == mine
    # the conditions as the source writes them
    for line, count in (('return n_edges <= SC_SMALL_EDGES ? SC_RUN_SMALL : SC_RUN;', 1),
                        ('if (run_len == SC_RUN_SMALL) {', 2),
                        ('else if (D <= 64 && !arg && n_runs <= %d) hipLaunchKernelGGL((scatter_runs_kernel<64, 1>)' % SC.LARGE_RUNS, 1),
                        ('else if (D <= 64 && !arg) hipLaunchKernelGGL((scatter_runs_kernel<8, 1>)', 1),
                        ('if (D > 64 * SC_MAXC) return SGNN_ERR_UNSUPPORTED_D;', 2),
                        ('if (n > SC_ONE_WG) return false;', 1),
                        ('if (m <= 1024 * IPT)', 1),
                        ('for (int64_t from = 0; from < n_lists; from += SC_MAX_JOBS) {', 1)):
        assert src.count(line) == count, line
    ipts = re.search(r'((?:SC_ONE_WG_CASE\(\d+\) ?)+)\n#undef SC_ONE_WG_CASE', src).group(1)
    assert tuple(int(v) for v in re.findall(r'\((\d+)\)', ipts)) == SC.IPTS and 1024 * SC.IPTS[-1] == SC.ONE_WG
    from subgnn_amd import ops
    assert ops.SCATTER_MAX_D == SC.MAX_D and ops.SCATTER_TOGETHER_BELOW == SC.TOGETHER_BELOW
    ops_src = open(os.path.join(REPO, 'subgnn_amd', 'ops.py')).read()
    assert ops_src.count('if together is not None and presorted is None and arg is None and E < SCATTER_TOGETHER_BELOW and D <= 256') == 1


def _instantiations(block):
    out = set()
    for args in re.findall(r'scatter_runs_kernel<([^>]*)>\)', block):
        a = [{'SC_RUN_SMALL': SC.RUN_SMALL, 'SC_RUN': SC.RUN, 'true': True, 'false': False}.get(t.strip(), t.strip()) for t in args.split(',')]
        a = [v if isinstance(v, bool) else int(v) for v in a] + [SC.RUN, False][len(a) - 2:]
        out.add(tuple(a))
    return out


def test_cases_reach_every_instantiation_of_both_dispatch_blocks():
    src = _source()
    single = src[src.index('extern "C" int sgnn_scatter_add_rows_sorted('):src.index('extern "C" int64_t sgnn_scatter_add_rows_multi_workspace_bytes')]
    multi = src[src.index('extern "C" int sgnn_scatter_add_rows_multi('):]
    want_single, want_multi = _instantiations(single), _instantiations(multi)
    assert len(want_single) == 8 and len(want_multi) == 6
    assert all(not f[3] for f in want_single) and all(f[3] for f in want_multi)
    for kind in ('grid', 'float'):
        got = {SC.case_form(c) for c in SC.CASES if c.kind == kind}
        assert got == want_single | want_multi, kind
    # per family: boundaries at every instantiation without arg, arg at all six with it, multi at all six of its own
    assert {SC.case_form(c) for c in GRID if c.family == 'boundaries'} == want_single - {(16, 1, SC.RUN, False)}
    assert {SC.case_form(c) for c in GRID if c.family == 'arg'} == want_single - {(64, 1, SC.RUN, False), (8, 1, SC.RUN, False)}
    assert {SC.case_form(c) for c in GRID if c.family == 'multi'} == want_multi
    # the thresholds from both sides, both addressings and all three term sets at a small and a large form
    sizes = {c.spec.E for c in GRID if c.family == 'forms' and c.D == 64}
    assert sizes >= {1, SC.RUN_SMALL - 1, SC.RUN_SMALL, SC.RUN_SMALL + 1, SC.SMALL_EDGES, SC.SMALL_EDGES + 1,
                     SC.LARGE_RUNS * SC.RUN, SC.LARGE_RUNS * SC.RUN + 1}
    for E in (17, SC.SMALL_EDGES + 1):
        assert {(c.spec.rows, c.spec.terms) for c in GRID if c.family == 'forms' and c.spec.E == E and c.D == 64} \
            == {(r, t) for r in ('div', 'list') for t in ('G', 'v', 'both')}
    assert SC.form(SC.LARGE_RUNS * SC.RUN, 64) == (64, 1, SC.RUN, False) and SC.form(SC.LARGE_RUNS * SC.RUN + 1, 64) == (8, 1, SC.RUN, False)
    assert {c.D for c in SC.CASES} == {8, 64, 128, 200, 256}
    with pytest.raises(ValueError):
        SC.form(100, SC.MAX_D + 1)
    for fam in ('forms', 'boundaries', 'arg', 'multi'):
        assert any(c.table0 for c in GRID if c.family == fam) and any(not c.table0 for c in GRID if c.family == fam)
    assert max(SC.spec_edges(c) for c in SC.CASES) == SC.LARGE_RUNS * SC.RUN + 1            # nothing larger: the tests stay quick


@pytest.mark.parametrize('case', [c for c in GRID if c.family == 'boundaries'], ids=_ids)
def test_boundary_cases_walk_the_carry_protocol(case):
    a, _, R, _ = SC.case_form(case)
    f = SC.classification(case)
    assert f['dest'] == {'head', 'run-on', 'tail', 'owned', 'pad'}
    assert f['boundary_on_run_end'] >= 6                                    # a segment ends exactly where a run ends
    assert f['tail_then_segments_then_head'] >= 1 and f['head_and_tail'] >= 1
    links = [n for _, n, _ in f['chains']]
    assert all(n >= 1 for n in links)
    assert set(links) >= set(SC.CHAIN_RUNS) | {SC.LAST_CHAIN_RUNS + 1}
    assert set(SC.CHAIN_RUNS) >= {1, SC.AHEAD, SC.AHEAD + 1, 2 * SC.AHEAD + 1}
    start, n, end = f['chains'][-1]                                         # the largest key's chain ends in the last, partial run
    assert end == f['n_runs'] - 1 and n == SC.LAST_CHAIN_RUNS + 1 and start + n == end
    assert 0 < f['last_cnt'] == SC.LAST_CNT < min(a, SC.AHEAD)
    # the PAD prefix: exactly one run / one edge less / one edge more
    pad = case.spec.pad
    assert int((SC.inputs(case)['lists'][0]['keys'] == 0).sum()) == R + pad
    assert (f['pad_run_exact'], f['pad_run_then_pad_start']) == ((1, 0) if pad == 0 else (0, 1) if pad == 1 else (0, 0))
    want_skipped = (R + pad) // a if pad >= 0 else (R - 1) // a
    assert f['skipped_groups'] == want_skipped
    assert f['skipped_then_read'] == (1 if pad == -1 and a < R else 0)


def test_named_boundary_cases_hold_a_skipped_group_at_every_ahead():
    """An AHEAD group whose last key is PAD (its rows are not read) in front of one that is read, in the same run."""
    for name, ahead in (('boundaries-run16-D256-pad-1', 8), ('boundaries-run64-D128-pad-1', 16), ('boundaries-run64-D200-pad-1', 8),
                        ('boundaries-run64-large-D64-pad-1', 8)):
        c = _case(name)
        assert SC.case_form(c)[0] == ahead and SC.classification(c)['skipped_then_read'] == 1, name
    for name in ('boundaries-run16-D64-pad+0', 'boundaries-run64-D8-pad+0'):                 # AHEAD = RUN: the whole run is the group
        c = _case(name)
        assert SC.case_form(c)[0] == SC.case_form(c)[2] and SC.classification(c)['skipped_groups'] == 1, name


@pytest.mark.parametrize('case', [c for c in GRID if c.family == 'arg'], ids=_ids)
def test_arg_cases_split_a_repeated_member_by_a_run_boundary(case):
    f = SC.classification(case)
    d = SC.inputs(case)['lists'][0]
    R = SC.case_form(case)[2]
    assert R == (SC.RUN_SMALL if case.name.startswith('arg-small') else SC.RUN)
    assert int((d['keys'] == 0).sum()) % R == R - 1
    assert f['split_repeats'] >= 3                 # keys 1, 3 (1 | 2) and 4 (2 | 1)
    assert f['repeat_after_other_row'] >= 1        # key 2: the run ends in another set's entry, the repeat opens the next run
    assert f['repeats_inside'] >= 4
    sk, rows = SC.sorted_view(d)
    for key, want in ((1, [0, 0]), (2, [1, 2, 2]), (3, [3, 3, 3]), (4, [4, 4, 4])):
        at = int((sk == key).nonzero()[0])
        assert rows[at:at + len(want)].tolist() == want
        assert at % R == (R - 2 if key == 4 else R - 1), key
    # the repeats matter: the argmax names the repeated member in some column whose gradient is not 0
    for row, key in ((0, 1), (2, 2), (3, 3), (4, 4), (5, 20)):
        assert ((d['arg'][row] == key) & (d['G'][row] != 0)).any(), (row, key)
    assert (d['edge_row'] is None) == (case.spec.rows == 'div')
    src_rows = SC.source_rows(d)
    assert bool((src_rows[1:] >= src_rows[:-1]).all())                      # a set's entries are adjacent


@pytest.mark.parametrize('case', [c for c in GRID if c.family != 'multi'], ids=_ids)
def test_restated_carry_protocol_gives_the_reference(case):
    """scatter_cases.emulate -- pieces to the table, to head slots and to tail slots by flush's rules, chains walked from the
    tails -- is the reference: the rules ``classify`` reports branches of are the ones that make the sums right."""
    assert torch.equal(SC.emulate(case), SC.reference(case))


def _wrong_rows(case, mutate):
    got, ref = SC.emulate(case, mutate), SC.reference(case)
    return set((got != ref).any(1).nonzero().view(-1).tolist())


@pytest.mark.parametrize('case', [c for c in GRID if c.family == 'boundaries'], ids=_ids)
def test_boundary_cases_would_see_a_dropped_last_link(case):
    """Were scatter_chains_kernel to leave out the last link of a chain, every constructed hub -- chains of 1, SC_AHEAD,
    SC_AHEAD + 1 and 2 SC_AHEAD + 1 links, the two hubs around the run with two carries, the chain into the last run --
    would come out different from the reference: its last link's partial sum is not 0."""
    n_rows = SC.inputs(case)['n_rows']
    hubs = {3, 5, 7, 9, 10, 13, n_rows - 1}
    sk = torch.sort(SC.inputs(case)['lists'][0]['keys'].long())[0]
    R = SC.case_form(case)[2]
    assert [int((sk == k).sum()) for k in (3, 5, 7, 9)] == [3 + w * R for w in SC.CHAIN_RUNS]
    assert _wrong_rows(case, 'drop_last_link') >= hubs
    assert not _wrong_rows(case, 'last_row')                                # (no arg: nothing to hand over)


@pytest.mark.parametrize('case', [c for c in GRID if c.family == 'arg'], ids=_ids)
def test_arg_cases_would_see_a_last_row_that_is_not_handed_over(case):
    """Were every run to start with last_row = -1, the members whose repeats a run boundary splits (keys 1, 3, 4) would be
    counted twice; key 2, whose run-opening repeat follows ANOTHER set's entry, must not change."""
    wrong = _wrong_rows(case, 'last_row')
    assert wrong >= {1, 3, 4} and 2 not in wrong


def test_arg_reference_is_autograd_of_max_over_a_padded_set():
    """Three sets over a table of 6 rows: a member listed twice, a set shorter than the padding, ties among members."""
    D, A = 4, 3
    E = torch.tensor([[0, 0, 0, 0], [1, -1, 2, -2], [1, 2, -1, -2], [-1, -1, -1, -1], [2, 0, 0, -1], [0, 1, 1, 1]], dtype=torch.float64)
    sets = torch.tensor([[1, 2, 1], [3, 0, 0], [4, 5, 4]])
    G = torch.tensor([[1, 2, -1, 2], [2, 2, 1, -1], [-2, 1, 1, 2]], dtype=torch.float64)
    Et = E.clone().requires_grad_(True)
    val, idx = torch.nn.functional.embedding(sets, Et, padding_idx=0).max(dim=1)
    (val * G).sum().backward()
    arg = torch.gather(sets.unsqueeze(2).expand(-1, -1, D), 1, idx.unsqueeze(1)).squeeze(1)
    assert arg.tolist() == [[1, 2, 1, 1], [0, 0, 0, 0], [4, 5, 5, 5]]             # the first maximal entry in set order; PAD beats negatives
    case = SC.Case('tiny', 'arg', 'grid', D, SC.Arg(3, 'div'))
    inp = {'n_rows': 6, 'table0': torch.zeros(6, D), 'lists': [{'keys': sets.view(-1).to(torch.int32), 'G': G.float(), 'edge_row': None,
                                                                  'edges_per_row': A, 'c1': None, 'c2': None, 'v': None, 'arg': arg.to(torch.int32)}]}
    got = SC.evaluate(case, inp, torch.float64)
    assert torch.equal(got, Et.grad) and float(got[1].abs().sum()) > 0
    # counted once per listing, set 0's member 1 would come out doubled
    twice = SC.evaluate(case, dict(inp, lists=[dict(inp['lists'][0], arg=None)]), torch.float64)
    assert torch.equal(twice[1], 2 * G[0]) and not torch.equal(got[1], twice[1] * (arg[0] == 1))


def test_multi_cases_cover_the_pack_launches_and_the_list_kinds():
    multi = [c for c in GRID if c.family == 'multi']
    for c in multi:
        sizes = c.spec.sizes
        assert all(SC.waits_for_flush(n, c.D) == (n > 0) for n in sizes) and sum(1 for n in sizes if n) >= 2
        hub = [int((d['keys'] == 11).sum()) for d in SC.inputs(c)['lists'] if d['keys'].numel() > 20]
        assert hub and all(n > 0 for n in hub)                                     # one target every list adds to
    assert not SC.waits_for_flush(SC.TOGETHER_BELOW, 64) and not SC.waits_for_flush(100, 64, arg=True)
    assert not SC.waits_for_flush(100, 64, presorted=True) and not SC.waits_for_flush(0, 64)
    assert {tuple(SC.pack_launches(c.spec.sizes)) for c in multi} >= {(3,), (4,), (SC.MAX_JOBS, 1)}
    big = [c for c in multi if sum(c.spec.sizes) > SC.SMALL_EDGES]
    assert {c.D for c in big} == {64, 128, 200} and all(max(c.spec.sizes) < SC.TOGETHER_BELOW for c in big)
    assert any(0 in c.spec.sizes[1:-1] for c in multi)                             # a list without edges between two others
    for c in multi:                                                                # a list without G, explicit rows, both terms
        kinds = {(d['G'] is None, d['edge_row'] is not None, d['c1'] is not None, d['c2'] is not None) for d in SC.inputs(c)['lists']}
        assert kinds >= {(True, False, False, True), (False, True, False, False), (False, False, True, True)}, c.name


def test_sort_cases_reach_every_items_per_lane_form():
    assert {SC.sort_ipt(c.n) for c in SC.SORT_CASES} == set(SC.IPTS)
    assert {SC.sort_ipt(c.n) for c in SC.SORT_CASES if c.fill == 'random'} >= {1, 2, 3, 4, 5, 6, 8} - {4}
    sizes = {c.n for c in SC.SORT_CASES}
    for i in SC.IPTS[:-1]:
        assert {1024 * i, 1024 * i + 1} <= sizes or i == 4, i                      # (4096 / 4097: tests/test_gpu_float.py)
    assert SC.sort_ipt(SC.ONE_WG) == 8 and SC.sort_ipt(SC.ONE_WG + 1) is None and SC.sort_ipt(7169) == 8 and SC.sort_ipt(6145) == 8
    # every key the value the 0xFFFFFFFF padding ties with once the sort reads ``bits`` bits only
    full = [c for c in SC.SORT_CASES if c.fill == 'max']
    assert {c.max_key for c in full} == {1, 1023, 65535, (1 << 31) - 1} and {c.n for c in full} == {1000, 8191}
    for c in full:
        assert c.max_key == (1 << SC.key_bits(c.max_key)) - 1 and bool((SC.sort_keys(c) == c.max_key).all())
        assert c.n % 1024 != 0                                                     # the sort's last lanes hold padding
    assert {(c.n, c.max_key) for c in SC.SORT_CASES if c.fill == 'zero'} == {(c.n, c.max_key) for c in full}
    assert [SC.key_bits(m) for m in (0, 1, 2, 1023, 1024, 65535, (1 << 31) - 1)] == [1, 1, 2, 10, 11, 16, 31]


@pytest.mark.parametrize('case', GRID, ids=_ids)
def test_grid_float32_in_two_orders_equals_float64(case):
    inp = SC.inputs(case)                                                          # (asserts the 2^24 condition)
    ref = SC.reference(case)
    for d in inp['lists']:
        for t in (d['G'], d['c1'], d['c2'], d['v']):
            assert t is None or t.numel() == 0 or (t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= SC.GRID_MAX)
    assert float(SC.evaluate(case, inp, torch.float64, absolute=True).max()) < SC.EXACT_BELOW
    for reverse in (False, True):
        got = SC.evaluate(case, inp, torch.float32, reverse=reverse)
        assert got.dtype == torch.float32 and torch.equal(got.double(), ref), reverse
    assert torch.equal(ref[0], inp['table0'][0].double())                          # row 0 is never touched
    assert (ref != inp['table0'].double()).any() or SC.spec_edges(case) < 20
    assert bool(inp['table0'].any()) == case.table0


@pytest.mark.parametrize('case', FLOAT, ids=_ids)
def test_float32_evaluation_meets_the_gpu_tolerances(case):
    """The bounds tests/test_gpu_scatter.py asserts are the ones a plain float32 evaluation of the same sums keeps."""
    got = SC.evaluate(case, SC.inputs(case), torch.float32)
    assert_close(got, SC.reference(case), case.name, tol=REL_TOL, norm_tol=NORM_TOL)

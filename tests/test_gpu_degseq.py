"""-m gpu: the degree-sequence kernels (csrc/degree_sequence.hip) at every list length, table form and hub form of
degseq_cases.py, against the C oracle.  Exact.  test_degseq_cases_host.py shows, without a GPU, that the cases reach the
paths they are named after."""
import ctypes
import time

import numpy as np
import pytest
import torch

import degseq_cases as D
from oracle import cbind
from test_gpu_integer import DEV, _ops

pytestmark = pytest.mark.gpu
_SETUP = {}

FORMS = {
    'streamed': dict(search_long_lists=False),
    'searched': dict(hub_bitmaps=False),
    'bitmaps_records': dict(),
    'bitmaps_self_loops_in_flight': dict(use_self_loop_table=False),
}


def _groups():
    return {'wave': [c['nodes'] for c in D.wave_cases()], 'block': [c['nodes'] for c in D.block_cases()], 'many': D.many_sets()}


def shared():
    """The ladder on the device (with its degree dict), the three groups of sets as Ragged, and the oracle's answers: built
    once, never written."""
    if not _SETUP:
        ops = _ops()
        L = D.ladder()
        _SETUP['L'] = L
        _SETUP['dg'] = ops.DeviceGraph(L.rowptr, L.col, L.G.node_order, DEV, full_degree=L.full_degree)
        rp, col = L.multigraph_csr()
        _SETUP['multi_csr'] = (rp, col)
        _SETUP['multi'] = ops.DeviceGraph(rp, col, L.G.node_order, DEV, full_degree=L.full_degree)
        for name, sets in _groups().items():
            _SETUP[name] = (sets, ops.Ragged.from_lists(sets, DEV), cbind.ragged(sets))
        _SETUP['ref'] = {}
    return _SETUP


def oracle(group, multi, use_dict, srt):
    S = shared()
    key = (group, multi, use_dict, srt)
    if key not in S['ref']:
        L = S['L']
        rp, col = S['multi_csr'] if multi else (L.rowptr, L.col)
        ptr, flat = S[group][2]
        S['ref'][key] = cbind.degree_sequence(rp, col, L.full_degree if use_dict else None, ptr, flat, srt)
    return S['ref'][key]


def _same(got, want, what):
    n = len(want)
    got = got.cpu().numpy()[:n]
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError('%s: %d of %d entries differ, first at %d: got %d, oracle %d'
                             % (what, len(bad), n, bad[0], got[bad[0]], want[bad[0]]))


def test_the_ladder_has_two_words_of_hub_bits():
    S = shared()
    hub = S['dg'].hub_tables()
    assert hub is not None and hub[2] == 2 and hub[1].shape == (D.N_IDS + 1, 2)
    assert int((hub[0] >= 0).sum()) == D.N_HUBS
    assert {v: int(hub[0][v]) for v in S['L'].hub_ids} == S['L'].hub_number
    assert S['dg'].simple_rows and S['dg'].node_records().shape == (D.N_IDS + 1, 4)
    assert not S['multi'].simple_rows and S['multi'].hub_tables() is None


@pytest.mark.parametrize('group', ['wave', 'block', 'many'])
@pytest.mark.parametrize('form', list(FORMS))
def test_every_form_against_the_oracle(form, group):
    ops = _ops()
    S = shared()
    _, r, _ = S[group]
    assert S['dg'].hub_tables()[2] == 2
    assert (r.n > D.FEW) == (group == 'many')
    for srt in (True, False):
        for ext in (True, False):
            for use_dict in (True, False):
                gi, ge = ops.degree_sequence(S['dg'], r, sort=srt, use_degree_dict=use_dict, want_external=ext, **FORMS[form])
                ci, ce = oracle(group, False, use_dict, srt)
                what = '%s %s sort=%s external=%s dict=%s' % (form, group, srt, ext, use_dict)
                _same(gi, ci, what + ' internal')
                assert (ge is None) == (not ext)
                if ext:
                    _same(ge, ce, what + ' external')


def test_which_case_differs_unsorted():
    """The wave cases one launch, unsorted, default form: a difference is reported with the name of its case."""
    ops = _ops()
    S = shared()
    sets, r, (ptr, _) = S['wave']
    for form in FORMS:
        gi, ge = ops.degree_sequence(S['dg'], r, sort=False, use_degree_dict=False, **FORMS[form])
        ci, ce = oracle('wave', False, False, False)
        gi, ge = gi.cpu().numpy(), ge.cpu().numpy()
        bad = [c['name'] for s, c in enumerate(D.wave_cases())
               if not (np.array_equal(gi[ptr[s]:ptr[s + 1]], ci[ptr[s]:ptr[s + 1]]) and np.array_equal(ge[ptr[s]:ptr[s + 1]], ce[ptr[s]:ptr[s + 1]]))]
        assert bad == [], (form, bad)


@pytest.mark.parametrize('group', ['wave', 'many'])
def test_dispatch_order_changes_nothing(group):
    ops = _ops()
    S = shared()
    sets, r, _ = S[group]
    hf = ops.heaviest_first(S['dg'], r)
    order = hf.cpu().numpy()
    assert sorted(order.tolist()) == list(range(len(sets)))
    work = np.array([int(S['L'].deg[s].sum()) if len(s) else 0 for s in sets])
    assert np.all(np.diff(work[order]) <= 0)                               # heaviest first: non-increasing host-computed work
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(sets)).astype(np.int32)).to(DEV)
    for form in ('streamed', 'bitmaps_records'):
        for srt in (True, False):
            a, b = ops.degree_sequence(S['dg'], r, sort=srt, **FORMS[form])
            for o in (hf, hf.flip(0).contiguous(), perm):
                c, d = ops.degree_sequence(S['dg'], r, sort=srt, order=o, **FORMS[form])
                assert torch.equal(a, c) and torch.equal(b, d), (form, srt)
            _same(a, oracle(group, False, True, srt)[0], form)


def _raw_hub_bitmaps(ops, dg, r, col_sorted, hub_index, bits, W, rec, fd, sl, info_degree, srt, out_i, out_e):
    from subgnn_amd import _lib
    _lib.check(_lib.load().sgnn_degree_sequence_hub_bitmaps(
        ops._ptr(dg.rowptr), ops._ptr(dg.col), ops._ptr(col_sorted), dg.nnz, ops._ptr(fd), ops._ptr(sl), ops._ptr(hub_index),
        ops._ptr(bits), W, ops._ptr(rec), info_degree, ops._ptr(r.ptr), ops._ptr(r.nodes), r.n, max(r.max_len, 1), 1 if srt else 0,
        ops._ptr(out_i), ops._ptr(out_e), None, ops._stream()), 'sgnn_degree_sequence_hub_bitmaps')


@pytest.mark.parametrize('parity', [0, 1])
@pytest.mark.parametrize('sorted_rows', [True, False], ids=['search_the_rest', 'stream_the_rest'])
def test_partial_bitmaps_through_the_c_abi(sorted_rows, parity):
    """A bitmap for every other long list: the others are searched next to them in one round of phase A0 (col_sorted given) or
    streamed by the SEARCH instantiation's 8-loads-in-flight loop (col_sorted NULL)."""
    ops = _ops()
    S = shared()
    L, dg = S['L'], S['dg']
    hub_index, bits, W, H, n_numbered = D.partial_hub_tables(L.rowptr, L.col, parity)
    assert n_numbered == H // 2 and W == 1
    t_index = torch.from_numpy(hub_index).to(DEV)
    t_bits = torch.from_numpy(bits.view(np.int32)).to(DEV).contiguous()
    col_sorted = dg.col_sorted if sorted_rows else None
    for group in ('wave', 'many'):
        _, r, _ = S[group]
        n_tot = r.nodes.numel()
        for use_dict in (True, False):
            fd = dg.full_degree if use_dict else None
            rec = torch.from_numpy(D.node_records(L.rowptr, L.col, hub_index, L.full_degree if use_dict else None)).to(DEV).contiguous()
            # node records | rowptr + hub_index + self-loop table | rowptr + hub_index, self loops counted in flight
            for how, (rec_, sl_) in {'records': (rec, None), 'tables': (None, dg.self_loops), 'in_flight': (None, None)}.items():
                for srt in (True, False):
                    out_i = torch.empty(n_tot, dtype=torch.int32, device=DEV)
                    out_e = torch.empty(n_tot, dtype=torch.int32, device=DEV)
                    _raw_hub_bitmaps(ops, dg, r, col_sorted, t_index, t_bits, W, rec_, fd, sl_, 1 if use_dict else 0, srt, out_i, out_e)
                    ci, ce = oracle(group, False, use_dict, srt)
                    what = 'parity %d %s %s dict=%s sort=%s' % (parity, group, how, use_dict, srt)
                    _same(out_i, ci, what + ' internal')
                    _same(out_e, ce, what + ' external')


@pytest.mark.parametrize('group', ['wave', 'block', 'many'])
def test_multigraph_rows_are_streamed(group):
    """Rows with a repeated id: no hub tables, nothing is searched -- the lists of 2048 entries and more go through the full-block
    loop, and a repeated entry counts as often as it is listed."""
    ops = _ops()
    S = shared()
    _, r, _ = S[group]
    assert S['multi'].hub_tables() is None
    for srt in (True, False):
        for use_dict in (True, False):
            for table in (True, False):
                gi, ge = ops.degree_sequence(S['multi'], r, sort=srt, use_degree_dict=use_dict, use_self_loop_table=table)
                ci, ce = oracle(group, True, use_dict, srt)
                _same(gi, ci, 'multigraph %s internal sort=%s dict=%s table=%s' % (group, srt, use_dict, table))
                _same(ge, ce, 'multigraph %s external sort=%s dict=%s table=%s' % (group, srt, use_dict, table))
    # the repeated entries are seen: the multigraph's answers differ from the simple graph's
    assert not np.array_equal(oracle(group, True, False, False)[0], oracle(group, False, False, False)[0])


@pytest.mark.parametrize('sentinel', [7, -7])
def test_poisoned_outputs(sentinel):
    """Every entry inside ptr[-1] is written, nothing behind it is.  Two sentinels: 7 is a degree that occurs, so an entry left
    at 7 could pass for written -- it cannot in both runs; -7 is no degree at all."""
    from subgnn_amd import _lib
    ops = _ops()
    S = shared()
    dg = S['dg']
    lib = _lib.load()
    for group in ('wave', 'block'):
        sets, r, _ = S[group]
        if group == 'block':                                           # (the workspace tier is sgnn_degree_sequence_huge's: not this call)
            sets = [s for s in sets if len(s) <= D.LDS_MAX]
            r = ops.Ragged.from_lists(sets, DEV)
        n = int(r.ptr[-1].item())
        pad = 300
        ptr, flat = cbind.ragged(sets)
        for srt in (True, False):
            ci, ce = cbind.degree_sequence(S['L'].rowptr, S['L'].col, None, ptr, flat, srt)
            for entry in ('plain', 'sorted_rows'):
                out_i = torch.full((n + pad,), sentinel, dtype=torch.int32, device=DEV)
                out_e = torch.full((n + pad,), sentinel, dtype=torch.int32, device=DEV)
                tail = (ops._ptr(r.ptr), ops._ptr(r.nodes), r.n, max(r.max_len, 1), 1 if srt else 0, ops._ptr(out_i), ops._ptr(out_e),
                        None, ops._stream())
                if entry == 'plain':
                    _lib.check(lib.sgnn_degree_sequence(ops._ptr(dg.rowptr), ops._ptr(dg.col), dg.nnz, None, ops._ptr(dg.self_loops),
                                                        *tail), entry)
                else:
                    _lib.check(lib.sgnn_degree_sequence_sorted_rows(ops._ptr(dg.rowptr), ops._ptr(dg.col), ops._ptr(dg.col_sorted), dg.nnz,
                                                                    None, ops._ptr(dg.self_loops), *tail), entry)
                gi, ge = out_i.cpu().numpy(), out_e.cpu().numpy()
                assert np.all(gi[n:] == sentinel) and np.all(ge[n:] == sentinel), (group, entry, srt)
                assert np.array_equal(gi[:n], ci) and np.array_equal(ge[:n], ce), (group, entry, srt)
                if sentinel < 0:
                    assert not np.any(gi[:n] == sentinel) and not np.any(ge[:n] == sentinel)


def test_ids_beyond_two_to_the_24():
    """The slot of an id comes from its low 24 bits; only the compare of the whole id keeps v and v + 2^24 apart."""
    ops = _ops()
    t0 = time.perf_counter()
    rp, col, sets, names = D.big_id_graph()
    g = ops.DeviceGraph.from_device_csr(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV))
    assert g.max_id == D.BIG + D.N_IDS and g.simple_rows
    r = ops.Ragged.from_lists(sets, DEV)
    ptr, flat = cbind.ragged(sets)
    for srt in (True, False):
        ci, ce = cbind.degree_sequence(rp, col, None, ptr, flat, srt)
        for form in ('streamed', 'searched', 'bitmaps_records'):
            for table in (True, False):
                kw = dict(FORMS[form], use_self_loop_table=table)
                gi, ge = ops.degree_sequence(g, r, sort=srt, use_degree_dict=False, **kw)
                _same(gi, ci, 'big ids %s internal sort=%s' % (form, srt))
                _same(ge, ce, 'big ids %s external sort=%s' % (form, srt))
    torch.cuda.synchronize()
    print('ids beyond 2^24: %.2f s' % (time.perf_counter() - t0))

"""The degree-sequence test cases reach the kernel paths their names say, according to the host model of degseq_cases.py, and
together they cover its coverage table; the C oracle the GPU tests compare with agrees with a plain Python restatement on
every one of them.  No GPU."""
import numpy as np
import pytest

import degseq_cases as D
from oracle import cbind


def test_constants_are_parsed_integers():
    for k, v in D.CONST.items():
        if k == 'MULT':
            assert len(v) == D.DS_TRIES and all(isinstance(x, int) and 0 < x < (1 << 24) for x in v)
            assert len(set(v)) == len(v)
        else:
            assert isinstance(v, int) and v > 0, k
    assert D.DS_BIG == 64                                   # one 64-entry load: what list_class counts in
    assert D.DS_SEARCH == 64 * D.TAIL_LOADS == 64 * D.INFL_SEARCH


def test_slot_restatement():
    a, b, c = D.WRAP_IDS
    k = D.MULT[-1]
    assert (D.slot(a, k), D.slot(b, k), D.slot(c, k)) == (D.HASH - 2, D.HASH - 1, D.HASH - 1)
    assert len({a, b, c}) == 3 and max(a, b, c) <= 3000
    for v in (1, 77, 5999):
        for k in D.MULT:
            assert D.slot(v, k) == D.slot(v + D.BIG, k) and 0 <= D.slot(v, k) < D.HASH
    assert D.first_clean_try([5, 5 + D.BIG]) == D.DS_TRIES and D.first_clean_try([5, 5]) == 0


def test_the_ladder_has_a_node_of_every_degree():
    L = D.ladder()
    deg = L.deg
    assert L.max_id == D.N_IDS and 5900 <= len(L.G.node_order) <= D.N_IDS
    have = set(deg.tolist())
    for d in D.EDGE_DEGREES + D.STREAM_DEGREES_MORE + (0,):
        assert d in have, d
    assert all(deg[z] == 0 for z in D.ZERO_IDS) and len(D.ZERO_IDS) >= 3
    hubs = np.nonzero(deg >= D.DS_SEARCH)[0].tolist()
    assert hubs == L.hub_ids and len(hubs) >= 40 and (len(hubs) + 31) // 32 == 2
    assert deg.max() > 4096
    # symmetric and simple
    rows = [set(L.row(v).tolist()) for v in range(L.max_id + 1)]
    assert all(len(rows[v]) == deg[v] for v in range(L.max_id + 1))
    assert all(v in rows[u] for v in range(L.max_id + 1) for u in rows[v])
    assert [v for v in range(L.max_id + 1) if v in rows[v]] == sorted([D.SELF_LOOP_SHORT, L.self_loop_hub])
    assert deg[L.self_loop_hub] >= D.DS_SEARCH and deg[D.SELF_LOOP_SHORT] < D.DS_BIG
    u, v = L.adjacent_hubs
    assert v in rows[u] and deg[u] >= D.DS_SEARCH and deg[v] >= D.DS_SEARCH
    assert L.hub_number[L.late_hub] >= 32 and all(h in rows[L.late_hub] for h in L.hub_ids[:4])
    # the rows are NOT ascending: the streamed forms read another order than the searched ones
    assert any(np.any(np.diff(L.row(h)) < 0) for h in L.hub_ids)
    assert (L.full_degree != deg + (np.arange(L.max_id + 1) == L.self_loop_hub) + (np.arange(L.max_id + 1) == D.SELF_LOOP_SHORT)).sum() > 1000


def test_the_multigraph_variant_repeats_an_id_and_a_self_loop():
    L = D.ladder()
    rp, col = D.ladder().multigraph_csr()
    h = L.self_loop_hub
    row = col[rp[h]:rp[h + 1]].tolist()
    assert row.count(h) == 2 and len(row) == L.deg[h] + 2 and len(row) >= 64 * D.DS_INFLIGHT
    twice = [u for u in set(row) if u != h and row.count(u) == 2]
    assert len(twice) == 1 and col[rp[twice[0]]:rp[twice[0] + 1]].tolist().count(h) == 2
    assert rp[-1] == L.rowptr[-1] + 3


@pytest.mark.parametrize('case', D.wave_cases() + D.block_cases(), ids=lambda c: c['name'])
def test_a_case_reaches_what_its_name_says(case):
    f = D.case_facts(case) if len(case['nodes']) <= D.WAVE_MAX else {'n': len(case['nodes'])}
    for k, want in case['expect'].items():
        assert f[k] == want, (case['name'], k, f[k], want)
    assert all(1 <= v <= D.N_IDS for v in case['nodes'])


def test_edge_cases_hold_the_neighbours_at_the_load_borders():
    L = D.ladder()
    by_name = {c['name']: c for c in D.wave_cases()}
    for d in D.EDGE_DEGREES:
        s = by_name['deg_%d_edges' % d]['nodes']
        row = L.row(s[0])
        assert len(row) == d
        for p in (0, d - 1, 63, 64, 511, 512, 2047, 2048):
            if 0 <= p < d:
                assert int(row[p]) in s, (d, p)
        assert any(int(u) not in s for u in row) or d <= 2


def test_the_wrap_case_and_the_table_forms():
    L = D.ladder()
    by_name = {c['name']: c for c in D.wave_cases()}
    s = by_name['table_probed_wrap_past_the_last_slot']['nodes']
    assert set(D.WRAP_IDS) <= set(s) and D.wraps(s)
    for v in D.WRAP_IDS:
        row = set(L.row(v).tolist())
        assert row & set(s) and row - set(s), v                # neighbours inside and outside the set
    probed = [c for c in D.wave_cases() if D.first_clean_try(c['nodes']) == D.DS_TRIES]
    assert sum(len(c['nodes']) == 48 for c in probed) >= 3 and sum(len(c['nodes']) == 64 for c in probed) >= 3


def test_block_cases():
    L = D.ladder()
    sizes = [len(c['nodes']) for c in D.block_cases()]
    assert sizes == [65, 128, 129, 256, 257, 1024, 2048, 2050]
    for c in D.block_cases():
        s = c['nodes']
        assert len(set(s)) == len(s) - 1
        assert any(L.deg[v] >= 2048 for v in s) and set(D.ZERO_IDS) <= set(s)
        assert L.self_loop_hub in s and D.SELF_LOOP_SHORT in s


def test_many_sets_pick_the_other_kernel_objects():
    sets = D.many_sets()
    assert D.FEW < len(sets) <= D.FEW + 300 and sum(len(s) == 0 for s in sets) == 1
    assert len(D.wave_cases()) <= D.FEW and max(len(s) for s in sets) == D.WAVE_MAX
    assert {tuple(s) for s in sets if s} == {tuple(c['nodes']) for c in D.wave_cases()}


def test_the_cases_cover_the_coverage_table():
    assert D.uncovered(D.wave_cases()) == []


def test_the_coverage_check_bites():
    """Without the cases made for an entry, the entry is reported."""
    cases = D.wave_cases()

    def without(*prefixes):
        return [c for c in cases if not c['name'].startswith(prefixes)]
    assert 'table: probe wraps past the last slot' in D.uncovered(without('table_probed_wrap'))
    assert 'flat total 128' in D.uncovered(without('flat_128'))
    assert 'a long list listed twice' in D.uncovered(without('dup_'))
    lost = D.uncovered(without('n21_', 'n22_', 'n32_'))
    assert 'A0: several rounds with G >= 2' in lost and 'n = 22' in lost
    assert 'INFL %d: full blocks and no tail' % D.DS_INFLIGHT in D.uncovered(without('deg_2048_', 'n', 'block', 'table', 'dup'))
    assert D.uncovered([]) == list(D.COVERAGE)


def test_partial_hub_tables_number_every_other_long_list():
    L = D.ladder()
    for parity in (0, 1):
        hub_index, bits, W, H, n_numbered = D.partial_hub_tables(L.rowptr, L.col, parity)
        assert H == D.N_HUBS and n_numbered == H // 2 and W == 1
        numbered = [v for v in L.hub_ids if hub_index[v] >= 0]
        assert numbered == L.hub_ids[parity::2] and sorted(hub_index[numbered].tolist()) == list(range(n_numbered))
        for v in numbered[:3] + numbered[-1:]:
            h = int(hub_index[v])
            assert np.nonzero((bits[:, h >> 5] >> np.uint32(h & 31)) & 1)[0].tolist() == sorted(L.row(v).tolist())
        rec = D.node_records(L.rowptr, L.col, hub_index, None)
        v = L.self_loop_hub
        assert rec.shape == (L.max_id + 1, 4) and rec[v, 0] == L.rowptr[v] and rec[v, 1] == L.deg[v] and rec[v, 3] == L.deg[v] + 1
        assert (int(rec[v, 2]) >> 24) & 0xff == 1 and (int(rec[D.ZERO_IDS[0], 2]) & 0xffffff) == 0xffffff


def _sets_of(group):
    return {'wave': [c['nodes'] for c in D.wave_cases()], 'block': [c['nodes'] for c in D.block_cases()]}[group]


@pytest.mark.parametrize('multi', [False, True], ids=['simple', 'multigraph'])
@pytest.mark.parametrize('group', ['wave', 'block'])
def test_the_c_oracle_agrees_with_the_plain_restatement(group, multi):
    L = D.ladder()
    rp, col = L.multigraph_csr() if multi else (L.rowptr, L.col)
    sets = _sets_of(group)
    ptr, flat = cbind.ragged(sets)
    for fd in (None, L.full_degree):
        for srt in (True, False):
            ci, ce = cbind.degree_sequence(rp, col, fd, ptr, flat, srt)
            pi, pe = D.degree_sequence_plain(rp, col, fd, sets, srt)
            assert np.array_equal(ci, pi) and np.array_equal(ce, pe), (srt, fd is None)
    ci, _ = cbind.degree_sequence(rp, col, None, ptr, flat, False)
    assert ci.max() > 0 and (ci == 0).any()


def test_big_id_sets():
    rp, col, sets, names = D.big_id_graph()
    assert len(rp) == D.BIG + D.N_IDS + 2 and rp[-1] == len(col)
    deg = np.diff(rp)
    assert deg[D.N_IDS + 1:D.BIG + 1].sum() == 0 and deg.max() >= D.DS_SEARCH      # (the 511 list and its cross edges: one is searched)
    for s, name in zip(sets, names):
        assert len(s) <= D.WAVE_MAX and len(set(s)) == len(s)
        if name.startswith('both'):
            assert D.first_clean_try(s) == D.DS_TRIES and any(v + D.BIG in s for v in s)
        if name.startswith('low_only'):
            row = col[rp[s[0]]:rp[s[0] + 1]].tolist()
            assert any(u - D.BIG in s for u in row if u > D.BIG)           # v + 2^24 is a neighbour, v a member
            assert all(v < D.BIG for v in s)
    ptr, flat = cbind.ragged(sets)
    for srt in (True, False):
        ci, ce = cbind.degree_sequence(rp, col, None, ptr, flat, srt)
        pi, pe = D.degree_sequence_plain(rp, col, None, sets, srt)
        assert np.array_equal(ci, pi) and np.array_equal(ce, pe)

"""The connected-component test cases of cc_cases.py reach what they are named after, according to the kernels' arithmetic
restated in Python integers; their reference agrees with two independent routes (the oracle's traversal, networkx on the
induced subgraph); no call asks for more than 2^23 entries of component tensor; and the five entry points refuse bad arguments
on the host, before anything touches a device.  No GPU."""
import ctypes

import numpy as np
import pytest

import cc_cases as K
from oracle import integer_half as IH

ORACLE_MAX = 2305                       # single sets up to here are compared with the oracle, the larger ones with networkx


# ---- the graph ---------------------------------------------------------------------------------------------------------------------

def test_constants_are_the_kernels():
    assert (K.WAVE_MAX, K.LDS_MAX, K.LDS_HASH, K.CCH_THREADS) == (64, 2048, 4096, 256)
    assert K.LDS_HASH >= 2 * K.LDS_MAX                               # load <= 1/2 in LDS
    assert K.CAPS == {'labels_wave': 8192, 'labels_lds': 2048, 'compact_wave': 16384, 'compact_lds': 2048,
                      'labels_huge': 1024, 'compact_huge': 1024}
    assert all(cap % 1024 == 0 for cap in K.CAPS.values())           # what _family_index relies on


def test_the_graph_is_what_the_cases_assume():
    P = K.parts()
    rp, col = P.rowptr, P.col
    deg = np.diff(rp)
    assert P.max_id == K.MAX_ID and len(rp) == K.MAX_ID + 2 and 14000 <= K.MAX_ID <= 17000
    rows = np.repeat(np.arange(K.MAX_ID + 1), deg)
    assert np.all((np.diff(col) > 0) | (np.diff(rows) > 0))           # rows ascending, no id twice
    fwd = set(zip(rows.tolist(), col.tolist()))
    assert all((v, u) in fwd for u, v in fwd)                        # symmetric
    loops = sorted(u for u, v in fwd if u == v)
    assert loops == sorted(K.LOOPS) and len(loops) == 9
    plain = np.ones(K.MAX_ID + 1, dtype=bool)
    plain[list(K.LOOPS)] = False

    def degs(a, n):
        return deg[a:a + n][plain[a:a + n]]
    for a, n in ((K.PATH_A0, K.N_PATH_A), (K.PATH_B0, K.N_PATH_B)):
        assert degs(a + 1, n - 2).tolist() == [2] * len(degs(a + 1, n - 2)) and deg[a] == 1 and deg[a + n - 1] == 1
        assert all((v, v + 1) in fwd for v in range(a, a + n - 1))
    assert (K.PATH_B0 - 1, K.PATH_B0) not in fwd                     # the two paths are disjoint
    assert np.all(deg[K.CLIQUE0:K.CLIQUE0 + K.N_CLIQUE] == K.N_CLIQUE - 1)
    assert deg[K.HUB] == K.N_LEAVES and np.all(deg[K.LEAF0:K.LEAF0 + K.N_LEAVES] == 1)
    assert deg[K.COMMON] == K.N_LONELY and np.all(degs(K.LONELY0, K.N_LONELY) == 1)
    assert all((v, K.COMMON) in fwd for v in range(K.LONELY0, K.LONELY0 + K.N_LONELY))
    assert all(abs(a - b) > 1 for a in K.LOOPS_PATH for b in K.LOOPS_PATH if a != b)
    assert deg[0] == 0


def _all_cases():
    return [(name, c) for name, cs in K.calls().items() for c in cs]


def test_every_id_is_a_node_and_none_is_the_common_neighbour():
    """What keeps every GPU call inside rowptr: ids in [1, max_id]."""
    for name in K.calls():
        _, flat = K.ragged(K.sets_of(name))
        assert flat.dtype == np.int32 and flat.min() >= 1 and flat.max() <= K.MAX_ID, name
        assert not np.any(flat == K.COMMON), name


# ---- the restated arithmetic -------------------------------------------------------------------------------------------------------

def test_tiers_and_chunks():
    assert [K.tier(n) for n in (0, 1, 64, 65, 2048, 2049, 5000)] == ['empty', 'wave', 'wave', 'lds', 'lds', 'workspace', 'workspace']
    assert [K.chunk(n) for n in (64, 65, 2048, 2049)] == [64, 64, 64, 256]
    have = {c['n'] for c in K.single_cases() if c['builder'] == 'path_reversed'}
    assert have == set(K.N_EDGES)
    for edge in (K.WAVE_MAX, K.LDS_MAX):
        assert {edge, edge + 1} <= have
    for seam in (64, 128, 2048, 2304, 4096):                         # 64-seams; 2304 = 9 x 256 and 4096 are 256-seams too
        assert {seam - 1, seam, seam + 1} <= have


def test_pair_numbers_decode_at_both_ends():
    for n in K.N_EDGES:
        if n < 2:
            continue
        npairs = n * (n - 1) // 2
        for p in {0, 1, 2, npairs // 2, npairs - 65, npairs - 64, npairs - 2, npairs - 1}:
            if not 0 <= p < npairs:
                continue
            i, j = K.decode_pair(p)
            assert 0 <= i < j < n and K.pair_index(i, j) == p
        assert K.decode_pair(npairs - 1) == (n - 2, n - 1)


def test_the_workspace_table_of_every_huge_size():
    for n in sorted({c['n'] for _, c in _all_cases() if c.get('tier') == 'workspace'} | {len(c['nodes']) for c in K.many_huge()}):
        slots = K.workspace_slots(n)
        assert slots & (slots - 1) == 0 and slots <= 4 * n           # inside the region of 4 slots per entry
        assert 4 * n < 4 * slots and 2 * n <= slots                   # load in (1/4, 1/2]
        assert (2 * n == slots) == (n == 4096)                       # load exactly 1/2 only there
    assert K.workspace_slots(4096) == 8192 and K.workspace_slots(4095) == 8192 and K.workspace_slots(4097) == 16384
    assert K.workspace_slots(2049) == 8192 and K.workspace_slots(5000) == 16384


# ---- the single sets ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def single_ref():
    cases = K.single_cases()
    return cases, K.reference(K.parts(), [c['nodes'] for c in cases])


def test_every_builder_runs_at_the_sizes_it_allows():
    by = {}
    for c in K.single_cases():
        by.setdefault(c['builder'], []).append(c['n'])
        assert len(c['nodes']) == c['n'] and c['tier'] == K.tier(c['n']) and c['nodes'].dtype == np.int32
    assert set(by) == set(K.BUILDERS) and len(by) == 10
    for b in ('path_reversed', 'path_shuffled', 'all_lonely', 'two_interleaved', 'one_id', 'doubled', 'self_loops'):
        assert tuple(by[b]) == K.N_EDGES, b
    assert tuple(by['last_pair_only']) == K.N_EDGES[1:]              # needs two entries
    assert tuple(by['star_hub_last']) == tuple(n for n in K.N_EDGES if n <= K.N_LEAVES + 1) and 2305 in by['star_hub_last']
    assert set(by['clique']) == {1, 2, 63, 64, 65, 66, 70}
    for b, sizes in by.items():                                      # every builder in every tier it can reach
        assert {K.tier(n) for n in sizes} >= ({'wave', 'lds'} if b == 'clique' else {'wave', 'lds', 'workspace'}), b


def test_claimed_components_and_lengths(single_ref):
    cases, ref = single_ref
    for s, c in enumerate(cases):
        assert (int(ref.n_components[s]), int(ref.longest[s])) == (c['C'], c['L']), c['name']
        lab = ref.labels_of(s)
        assert np.all(lab <= np.arange(c['n'])) and np.all(lab[lab] == lab), c['name']


def test_what_the_names_say(single_ref):
    cases, ref = single_ref
    loops = set(K.LOOPS)
    for s, c in enumerate(cases):
        n, nodes, lab = c['n'], c['nodes'], ref.labels_of(s)
        b = c['builder']
        if b == 'path_reversed':
            assert nodes[-1] == nodes.min() and np.all(np.diff(nodes) == -1) and np.all(lab == 0)
        elif b == 'path_shuffled':
            assert sorted(nodes.tolist()) == list(range(K.PATH_A0, K.PATH_A0 + n)) and np.all(lab == 0)
            assert n < 3 or np.any(np.diff(nodes) != np.diff(nodes)[0])
        elif b == 'all_lonely':
            assert ref.n_components[s] == n and np.array_equal(lab, np.arange(n)) and len(set(nodes.tolist())) == n
        elif b == 'two_interleaved':
            assert np.array_equal(lab, np.arange(n) % 2)
            w = K.chunk(n)
            for seam in range(w, n, w):                              # each side of a seam that has two positions has both labels
                assert set(lab[:seam].tolist()) == {0, 1}
                assert set(lab[seam:].tolist()) == ({0, 1} if n - seam >= 2 else {0})
        elif b == 'one_id':
            assert len(set(nodes.tolist())) == 1 and np.all(lab == 0) and ref.lists(s) == [[int(nodes[0])]]
        elif b == 'doubled':
            h = (n + 1) // 2
            assert np.array_equal(nodes[h:], nodes[:n - h]) and len(set(nodes.tolist())) == h
            assert ref.lists(s) == [nodes[:h].tolist()]              # the first position of every id is the kept one
        elif b == 'last_pair_only':
            i, j = K.last_pair_first(n), n - 1
            npairs = n * (n - 1) // 2
            assert K.pair_index(i, j) >= npairs - 64 and K.decode_pair(K.pair_index(i, j)) == (i, j)
            assert i == 0 or n > K.WAVE_MAX + 1
            want = np.arange(n)
            want[j] = i
            assert np.array_equal(lab, want) and nodes[j] == nodes[i] + 1
            assert ref.n_components[s] == n - 1 > n - 2               # no early exit: n - 2 components short of one
        elif b == 'star_hub_last':
            assert nodes[-1] == K.HUB and np.all(lab == 0) and (n == 1 or np.all(nodes[:-1] >= K.LEAF0))
        elif b == 'clique':
            assert np.all(lab == 0) and len(set(nodes.tolist())) == n
            if n >= 63:
                # every pair is linked; position n - 1 is joined by pair (0, n - 1), and the round of 64 pairs that holds it is
                # not the last one: the loop ends on its union count with linked pairs still untested
                npairs = n * (n - 1) // 2
                assert K.pair_index(0, n - 1) // 64 < (npairs - 1) // 64
        elif b == 'self_loops':
            inside = {v for v in nodes.tolist() if v in loops}
            assert len(inside) == min(len(K.LOOPS), n) - (1 if n >= 3 else 0) and int(nodes[0]) in inside
            assert n < 3 or (nodes[-1] == nodes[0] and lab[-1] == 0)  # a member with a self loop, listed twice
            assert n < 64 or (inside & set(K.LOOPS_PATH) and inside & set(K.LOOPS_LONELY))
            assert ref.n_components[s] == len(set(nodes.tolist())) and ref.longest[s] == 1


def _networkx_route(Gx, nodes):
    """labels, n_components, longest, canonical lists -- through nx.connected_components of the induced subgraph."""
    import networkx as nx
    nodes = [int(v) for v in nodes]
    comp = {}
    for k, cc in enumerate(nx.connected_components(Gx.subgraph(set(nodes)))):
        for v in cc:
            comp[v] = k
    first, lists, seen = {}, {}, set()
    for i, v in enumerate(nodes):
        first.setdefault(comp[v], i)
        if v not in seen:
            seen.add(v)
            lists.setdefault(comp[v], []).append(v)
    labels = np.array([first[comp[v]] for v in nodes], dtype=np.int32)
    out = [lists[k] for k in sorted(lists, key=lambda k: first[k])]
    return labels, len(out), max((len(l) for l in out), default=0), out


def _oracle_route(G, nodes):
    nodes = [int(v) for v in nodes]
    lists = IH.connected_components(G, nodes)
    where = {}
    for l in lists:
        f = nodes.index(l[0])                                        # (lists are in set order: their first node is the first position)
        for v in l:
            where[v] = f
    return np.array([where[v] for v in nodes], dtype=np.int32), len(lists), max((len(l) for l in lists), default=0), lists


@pytest.fixture(scope='module')
def nx_graph():
    import networkx as nx
    Gx = nx.Graph()
    Gx.add_nodes_from(range(1, K.MAX_ID + 1))
    Gx.add_edges_from(K.parts().pairs)
    return Gx


def _same(ref, s, route, what):
    labels, ncc, longest, lists = route
    assert np.array_equal(ref.labels_of(s), labels), what
    assert (int(ref.n_components[s]), int(ref.longest[s])) == (ncc, longest), what
    assert ref.lists(s) == lists, what


def test_the_reference_equals_the_oracle_and_networkx_on_every_single_set(single_ref, nx_graph):
    cases, ref = single_ref
    G = K.parts().G
    small = large = 0
    for s, c in enumerate(cases):
        if c['n'] <= ORACLE_MAX:
            _same(ref, s, _oracle_route(G, c['nodes']), c['name'])
            small += 1
        else:
            _same(ref, s, _networkx_route(nx_graph, c['nodes']), c['name'])
            large += 1
    assert small > 100 and large >= 24


def test_the_reference_equals_both_routes_on_the_mixed_call(nx_graph):
    ref = K.reference_of('mixed')
    for s, c in enumerate(K.mixed()):
        if c['n'] == 0:
            assert ref.n_components[s] == 0 and ref.longest[s] == 0 and ref.lists(s) == [] and len(ref.labels_of(s)) == 0
        else:
            _same(ref, s, _networkx_route(nx_graph, c['nodes']), c['name'])
            if c['n'] <= ORACLE_MAX:
                _same(ref, s, _oracle_route(K.parts().G, c['nodes']), c['name'])


@pytest.mark.parametrize('family', list(K.FAMILIES))
def test_the_reference_equals_networkx_on_a_sample_of_every_family(family, nx_graph):
    cases = K.calls()[family]
    ref = K.reference_of(family)
    sample = np.random.default_rng(77).choice(len(cases), 200, replace=False)
    for s in sorted(sample.tolist()):
        _same(ref, s, _networkx_route(nx_graph, cases[s]['nodes']), cases[s]['name'])


def test_the_reference_is_not_written_by_padded():
    ref = K.reference_of('mixed')
    before = [a.copy() for a in (ref.labels, ref.n_components, ref.longest, ref.k_rank, ref.k_within, ref.k_node)]
    C, L = ref.dims()
    out = K.padded(ref, C, L)
    loose = K.padded(ref, C + 3, L + 5)
    assert np.array_equal(loose[:, :C, :L], out) and loose[:, C:].sum() == 0 and loose[:, :, L:].sum() == 0
    assert (out != 0).sum() == len(ref.k_node)
    for s, c in enumerate(K.mixed()):
        assert [[v for v in row if v] for row in out[s].tolist() if row[0]] == ref.lists(s), c['name']
    for a, b in zip(before, (ref.labels, ref.n_components, ref.longest, ref.k_rank, ref.k_within, ref.k_node)):
        assert np.array_equal(a, b)


# ---- the families and the mixed call -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', list(K.FAMILIES))
def test_a_family_exceeds_its_grid_caps_with_another_shape_at_every_revisit(family):
    fn, caps = K.FAMILIES[family]
    cases = fn()
    lens = [len(c['nodes']) for c in cases]
    want = {'many_wave': (16500, 1, 4, 'wave'), 'many_block': (2100, 65, 72, 'lds'), 'many_huge': (1030, 2049, 2060, 'workspace')}[family]
    assert (len(cases), min(lens), max(lens)) == want[:3] and {K.tier(n) for n in lens} == {want[3]}
    assert set(lens) == set(range(want[1], want[2] + 1))
    for cap in caps:
        cap = K.CAPS[cap]
        assert len(cases) > cap                                       # some workgroup does a second subgraph
        for s in range(len(cases) - cap):                             # and finds another shape and another length than it left
            a, b = cases[s], cases[s + cap]
            assert a['shape'] != b['shape'] and len(a['nodes']) != len(b['nodes']), (family, cap, s)
    for a, b in zip(cases, cases[1:1024]):                            # neighbours differ too
        assert a['shape'] != b['shape'] or len(a['nodes']) != len(b['nodes'])
    ref = K.reference_of(family)
    if family == 'many_huge':
        assert ref.n_components.max() == 2 and {c['shape'] for c in cases} == {'path_reversed', 'two_interleaved', 'doubled'}
        assert 2_000_000 < ref.ptr[-1] < 2_200_000 and 92e6 < K.workspace_bytes(int(ref.ptr[-1])) < 94e6
    if family == 'many_block':
        assert ref.n_components.max() == 72 and ref.n_components.min() == 1 and len({c['shape'] for c in cases}) == 5
    if family == 'many_wave':
        assert {int(v) for v in ref.n_components} == {1, 2, 3, 4} and any(len(set(c['nodes'].tolist())) < len(c['nodes']) for c in cases)


def test_the_mixed_call_has_every_tier_between_empty_sets():
    cases = K.mixed()
    lens = [c['n'] for c in cases]
    assert {1, 64, 65, 2048, 2049, 4096} <= set(lens) and lens[0] == 0 and lens[-1] == 0 and lens.count(0) >= 6
    assert any(a == 0 and b == 0 for a, b in zip(lens, lens[1:]))     # two empty sets in a row
    tiers = [K.tier(n) for n in lens]
    for t in ('wave', 'lds', 'workspace'):
        own = [i for i, x in enumerate(tiers) if x == t]
        assert len(own) >= 3 and any(tiers[i + 1] not in (t, 'empty') for i in own)      # followed by another kernel's set


def test_no_call_asks_for_more_than_the_entry_limit():
    for name in K.calls():
        ref = K.reference_of(name)
        C, L = ref.dims()
        assert ref.n_sets * C * L <= K.MAX_ENTRIES, name
        if name in K.LOOSE_DIMS:
            assert ref.n_sets * (C + 3) * (L + 5) <= K.MAX_ENTRIES, name
    assert set(K.LOOSE_DIMS) | {'many_huge'} == set(K.calls())
    for name in K.DIRECT_LABELS:
        assert K.reference_of(name).ptr[-1] > 0 and max(len(s) for s in K.sets_of(name)) > K.LDS_MAX
    for name, other in K.WORKSPACE_CALLS:
        a, b = K.reference_of(name), K.reference_of(other)
        assert max(len(s) for s in K.sets_of(name)) > K.LDS_MAX and max(len(s) for s in K.sets_of(other)) > K.LDS_MAX
        assert a.ptr[-1] != b.ptr[-1]                                 # another layout: every array of the workspace starts elsewhere
    byname = {c['name']: name for name, cs in K.calls().items() for c in cs if name in ('long', 'wide')}
    assert byname['all_lonely_5000'] != byname['path_reversed_5000']


# ---- argument rules: every one returns before a launch -----------------------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    from subgnn_amd import _lib
    return _lib.load()


def _buf(n=64):
    b = (ctypes.c_int64 * n)()
    return b, ctypes.cast(b, ctypes.c_void_p)


BAD_ARG, SET_TOO_LARGE, NNZ_TOO_LARGE = -1, -2, -3


def test_error_codes_are_the_header_s():
    from subgnn_amd import _lib
    assert _lib.ERRORS[BAD_ARG] == 'SGNN_ERR_BAD_ARG' and _lib.ERRORS[SET_TOO_LARGE] == 'SGNN_ERR_SET_TOO_LARGE'
    assert _lib.ERRORS[NNZ_TOO_LARGE] == 'SGNN_ERR_NNZ_TOO_LARGE'


def test_workspace_bytes(lib):
    for total in (0, 1, 2049, 2116086, (1 << 28) - 1):
        assert lib.sgnn_cc_huge_workspace_bytes(total) == 44 * total + 64 == K.workspace_bytes(total)
    assert lib.sgnn_cc_huge_workspace_bytes(-1) == 64 and lib.sgnn_cc_huge_workspace_bytes(-(1 << 40)) == 64


def test_cc_labels_refuses_bad_arguments(lib):
    keep, p = _buf()
    good = dict(rowptr=p, col_sorted=p, nnz=8, sub_ptr=p, sub_nodes=p, n_subgraphs=0, max_sub_len=0, out_label=p, stream=None)

    def call(**over):
        return lib.sgnn_cc_labels(*{**good, **over}.values())
    for name in ('rowptr', 'col_sorted', 'sub_ptr', 'sub_nodes', 'out_label'):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(n_subgraphs=-1) == BAD_ARG
    assert call(nnz=1 << 31) == NNZ_TOO_LARGE and call(nnz=(1 << 31) - 1) == 0
    assert call() == 0                                                # no subgraph: nothing to do, nothing launched
    del keep


def test_cc_compact_and_stats_refuse_bad_arguments(lib):
    keep, p = _buf()
    good = dict(sub_ptr=p, sub_nodes=p, labels=p, n_subgraphs=0, max_sub_len=0, out_n_components=p, out_longest=p, stream=None)

    def stats(**over):
        return lib.sgnn_cc_compact_stats(*{**good, **over}.values())
    for name in ('sub_ptr', 'sub_nodes', 'labels', 'out_n_components', 'out_longest'):
        assert stats(**{name: None}) == BAD_ARG, name
    assert stats(n_subgraphs=-1) == BAD_ARG and stats() == 0
    good = dict(sub_ptr=p, sub_nodes=p, labels=p, n_subgraphs=0, max_sub_len=0, C=1, L=1, out=p, stream=None)

    def write(**over):
        return lib.sgnn_cc_compact(*{**good, **over}.values())
    for name in ('sub_ptr', 'sub_nodes', 'labels', 'out'):
        assert write(**{name: None}) == BAD_ARG, name
    for over in (dict(C=0), dict(L=0), dict(C=-1), dict(L=-5), dict(C=0, n_subgraphs=3), dict(L=0, n_subgraphs=3)):
        assert write(**over) == BAD_ARG, over
    assert write(n_subgraphs=-1) == BAD_ARG and write() == 0
    del keep


def test_cc_labels_huge_refuses_bad_arguments(lib):
    keep, p = _buf()
    total = 5000
    wsb = lib.sgnn_cc_huge_workspace_bytes(total)
    good = dict(rowptr=p, col=p, nnz=8, sub_ptr=p, sub_nodes=p, n_subgraphs=0, total_nodes=total, out_label=p, workspace=p,
                workspace_bytes=wsb, stream=None)

    def call(**over):
        return lib.sgnn_cc_labels_huge(*{**good, **over}.values())
    for name in ('rowptr', 'col', 'sub_ptr', 'sub_nodes', 'out_label', 'workspace'):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(n_subgraphs=-1) == BAD_ARG and call(total_nodes=-1) == BAD_ARG
    assert call(nnz=1 << 31) == NNZ_TOO_LARGE
    big = 1 << 28
    assert call(total_nodes=big, workspace_bytes=lib.sgnn_cc_huge_workspace_bytes(big)) == SET_TOO_LARGE
    assert call(total_nodes=big - 1, workspace_bytes=lib.sgnn_cc_huge_workspace_bytes(big - 1)) == 0
    assert call(workspace_bytes=wsb - 1) == BAD_ARG and call(workspace_bytes=wsb - 1, n_subgraphs=4) == BAD_ARG
    assert call(workspace_bytes=0) == BAD_ARG
    assert call() == 0 and call(workspace_bytes=wsb + 1) == 0
    del keep


@pytest.mark.parametrize('write', [0, 1])
def test_cc_compact_huge_refuses_bad_arguments(lib, write):
    keep, p = _buf()
    total = 5000
    wsb = lib.sgnn_cc_huge_workspace_bytes(total)
    good = dict(sub_ptr=p, sub_nodes=p, labels=p, n_subgraphs=0, total_nodes=total, write=write, C=1, L=1, out_n_components=p,
                out_longest=p, out=p, workspace=p, workspace_bytes=wsb, stream=None)

    def call(**over):
        return lib.sgnn_cc_compact_huge(*{**good, **over}.values())
    for name in ('sub_ptr', 'sub_nodes', 'labels', 'workspace'):
        assert call(**{name: None}) == BAD_ARG, name
    if write:
        assert call(out=None) == BAD_ARG
        for over in (dict(C=0), dict(L=0), dict(C=-1), dict(C=0, n_subgraphs=2)):
            assert call(**over) == BAD_ARG, over
        assert call(out_n_components=None, out_longest=None) == 0    # the write form needs no statistics arrays
    else:
        assert call(out_n_components=None) == BAD_ARG and call(out_longest=None) == BAD_ARG
        assert call(out=None, C=0, L=0) == 0                         # the statistics form needs no tensor and no shape
    assert call(n_subgraphs=-1) == BAD_ARG and call(total_nodes=-1) == BAD_ARG
    big = 1 << 28
    assert call(total_nodes=big, workspace_bytes=lib.sgnn_cc_huge_workspace_bytes(big)) == SET_TOO_LARGE
    assert call(workspace_bytes=wsb - 1) == BAD_ARG and call(workspace_bytes=wsb - 1, n_subgraphs=4) == BAD_ARG
    assert call() == 0
    del keep

"""-m gpu: the kept sorted one-hop borders (ops.khop1_borders_sorted: khop1_border_write_kernel) are the materialised borders in
ascending order, the draw from them (ops.draw_border_anchors: sgnn_sample_border_anchors) is the fused border + draw call's bit
for bit, and a pass that draws from kept borders (hotpath.prepare_pass) prepares what the fused call prepares.  Integers, and
floats that are 0 or 1: every comparison is torch.equal."""
import numpy as np
import pytest
import torch

from oracle import tape as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ops():
    from subgnn_amd import ops
    return ops


def _assert_sorted_borders(ops, dg, r, kept):
    ref = ops.sort_ragged(ops.khop_border(dg, r, 1))
    total = int(ref.ptr[-1])
    assert torch.equal(kept.ptr, ref.ptr)
    assert torch.equal(kept.counts, ref.lengths)
    assert torch.equal(kept.ids[:total], ref.nodes[:total])
    return ref


@pytest.mark.parametrize('lds', [None, 32])          # 32: an LDS bitmap of 32 bytes = 256 ids per slice (the sliced form)
def test_sorted_borders_small_graph(lds):
    from test_gpu_integer import _rand_graph, _dev_graph
    ops = _ops()
    G = _rand_graph(600, 2, 11)
    dg = _dev_graph(G)
    rng = np.random.default_rng(4)
    sets = [list({int(v) for v in rng.integers(1, G.max_id() + 1, int(rng.integers(1, 5)))}) for _ in range(700)]
    sets[3] = []
    sets[5] = list(range(1, 151))                   # more members than one 64-lane tile
    sets[6] = list(range(1, G.max_id() + 1))        # everything: empty border
    r = ops.Ragged.from_lists(sets, DEV)
    kept = ops.khop1_borders_sorted(dg, r, bitmap_in_lds=lds)
    _assert_sorted_borders(ops, dg, r, kept)
    assert int(kept.counts[3]) == 0 and int(kept.counts[6]) == 0 and int(kept.counts[5]) > 0
    # above max_bytes: nothing is kept
    assert ops.khop1_borders_sorted(dg, r, bitmap_in_lds=lds, max_bytes=4 * int(kept.ptr[-1]) - 1) is None
    assert ops.khop1_borders_sorted(dg, r, bitmap_in_lds=lds, max_bytes=4 * int(kept.ptr[-1])) is not None


@pytest.mark.parametrize('lds', [None, 1024])         # 1024 bytes of bitmap: 8192 ids per slice, 5 slices
def test_hub_borders_and_the_draw_from_them(lds):
    from subgnn_amd import synthetic
    ops = _ops()
    n = 40000
    rowptr, col = synthetic.sorted_csr(synthetic.barabasi_albert_edges(n, 8, seed=3), n)
    dg = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV)
    sets = synthetic.bfs_subgraphs(rowptr, col, 300, 12, seed=5)
    r = ops.Ragged.from_lists(sets, DEV)
    kept = ops.khop1_borders_sorted(dg, r, bitmap_in_lds=lds)
    _assert_sorted_borders(ops, dg, r, kept)
    A, seed, st = 300, 7, T.stream_id(T.STREAM_N_BOR, 'train', 0)          # more than 64 slots
    anchors, sims, counts = ops.khop_border_sample(dg, r, 1, A, seed, st, bitmap_in_lds=lds)
    a, w, c = ops.draw_border_anchors(kept, A, seed, st)
    assert a.dtype == anchors.dtype and w.dtype == sims.dtype and c.dtype == counts.dtype
    assert a.shape == anchors.shape and w.shape == sims.shape and c.shape == counts.shape
    assert torch.equal(a, anchors) and torch.equal(w, sims) and torch.equal(c, counts)
    # a shard of the rows with item_base and the full call's width reproduces those rows
    width = counts.max().view(1)
    a2, w2, c2 = ops.draw_border_anchors(kept.rows(100, 200), A, seed, st, item_base=100, width=width)
    assert torch.equal(a2, anchors[100:200]) and torch.equal(w2, sims[100:200]) and torch.equal(c2, counts[100:200])


def test_pad_rule_edges_on_stars():
    """Stars whose centres have 31, 32, 33 and 1 leaves, each centre a one-node set: border sizes around the PAD rule's
    32-bit edge (cnt < 32, cnt == 32, cnt > 32); the widest border has no PAD column."""
    ops = _ops()
    leaves = (31, 32, 33, 1)
    n = sum(leaves) + len(leaves)
    adj = [[] for _ in range(n + 1)]
    centres, nxt = [], 1
    for k in leaves:
        c = nxt
        centres.append(c)
        for v in range(c + 1, c + 1 + k):
            adj[c].append(v)
            adj[v].append(c)
        nxt = c + 1 + k
    rowptr = np.zeros(n + 2, dtype=np.int64)
    for v in range(n + 1):
        rowptr[v + 1] = rowptr[v] + len(adj[v])
    col = np.asarray([u for v in range(n + 1) for u in sorted(adj[v])], dtype=np.int32)
    dg = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV)
    r = ops.Ragged.from_lists([[c] for c in centres], DEV)
    A, seed, st = 64, 21, T.stream_id(T.STREAM_N_BOR, 'train', 1)
    kept = ops.khop1_borders_sorted(dg, r)
    assert kept.counts.tolist() == list(leaves)
    anchors, sims, counts = ops.khop_border_sample(dg, r, 1, A, seed, st)
    a, w, c = ops.draw_border_anchors(kept, A, seed, st)
    assert torch.equal(a, anchors) and torch.equal(w, sims) and torch.equal(c, counts)
    an, sm, mx = a.cpu().numpy(), w.cpu().numpy(), max(leaves)
    for i, (cen, k) in enumerate(zip(centres, leaves)):
        real = list(range(cen + 1, cen + 1 + k))                          # the sorted leaves
        for s in range(A):
            kk = T.nanchor_pick(seed, st, i * A + s, k, k < mx)
            assert an[i, s] == (0 if kk < 0 else real[kk])
            assert sm[i, s] == (0.0 if kk < 0 else 1.0)
    assert (an[3] == 0).any()                                              # one leaf: PAD wins half the slots


_LONG_LEAVES = (511, 512, 513, 4200)
_long_cache = []


def _long_list_case():
    """Host CSR (rows ascending), the sets and their numpy borders for test_long_lists_set_sizes_and_order; built once."""
    if _long_cache:
        return _long_cache[0]
    n = 8000
    adj = [[] for _ in range(n + 1)]

    def edge(u, v):
        adj[u].append(v)
        adj[v].append(u)

    centres, nxt = [], 1
    for k in _LONG_LEAVES:                              # stars on consecutive ids: centre, then its leaves
        centres.append(nxt)
        for v in range(nxt + 1, nxt + 1 + k):
            edge(nxt, v)
        nxt += 1 + k
    ring0 = nxt                                         # the other ids: a ring with a chord from every seventh node
    for v in range(ring0, n + 1):
        edge(v, v + 1 if v < n else ring0)
    for v in range(ring0, n - 400, 7):
        edge(v, v + 400)
    rowptr = np.zeros(n + 2, dtype=np.int64)
    for v in range(n + 1):
        rowptr[v + 1] = rowptr[v] + len(adj[v])
    col = np.asarray([u for v in range(n + 1) for u in sorted(adj[v])], dtype=np.int32)
    sets = [list(range(ring0, ring0 + 60)) + [c + 1 for c in centres],       # 64 members: one tile exactly; four leaves
            list(range(ring0 + 100, ring0 + 230, 2)),                        # 65 members: a second tile of one
            []]
    sets += [[c] for c in centres]
    sets += [[centres[2], centres[3]]]                                       # two long lists in one tile
    sets += [[v] for v in range(ring0 + 300, ring0 + 313)]                   # one-node sets
    borders = []
    for m in sets:
        members = np.asarray(m, dtype=np.int32)
        nb = np.concatenate([col[rowptr[v]:rowptr[v + 1]] for v in m]) if m else np.zeros(0, np.int32)
        borders.append(np.setdiff1d(np.unique(nb), members))
    _long_cache.append((rowptr, col, centres, sets, borders))
    return _long_cache[0]


@pytest.mark.parametrize('lds', [None, 256])          # 256 bytes of bitmap: 2048 ids per slice, so the 4200 leaves are a list of
def test_long_lists_set_sizes_and_order(lds):         # at least K1_LONG entries inside a slice too
    """List lengths at the edge of K1_LONG = 512 (511, 512, 513: the first belongs to one wavefront, the others are shared by
    all) and one of 4200 entries, more than one round of the long-list loop covers (K1_INFLIGHT * 16 * 64 = 4096); sets of 64
    and 65 members (one tile exactly, a second tile of one), an empty set, two long lists in one set; a set count that is
    no multiple of the K1_TAKE = 8 sets a workgroup takes per trip; the order= argument.  The borders are checked against
    numpy on the host CSR, the anchors against the tape's law on those borders."""
    ops = _ops()
    rowptr, col, centres, sets, borders = _long_list_case()
    # the case is what it is meant to be
    assert [int(rowptr[c + 1] - rowptr[c]) for c in centres] == list(_LONG_LEAVES)
    assert all(np.all(np.diff(col[rowptr[v]:rowptr[v + 1]]) > 0) for v in range(len(rowptr) - 1))
    assert [len(m) for m in sets[:3]] == [64, 65, 0] and sets[3:7] == [[c] for c in centres] and len(sets[7]) == 2
    assert len(sets) % 8 != 0 and all(len(m) == 1 for m in sets[8:])
    assert [len(b) for b in borders[3:8]] == list(_LONG_LEAVES) + [513 + 4200]
    assert len(rowptr) - 2 == 8000

    n = len(rowptr) - 2
    dg = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), DEV)
    r = ops.Ragged.from_lists(sets, DEV)
    kept = ops.khop1_borders_sorted(dg, r, bitmap_in_lds=lds)
    ptr, ids = kept.ptr.cpu().numpy(), kept.ids.cpu().numpy()
    assert kept.counts.tolist() == [len(b) for b in borders]
    for i, b in enumerate(borders):
        assert ptr[i + 1] - ptr[i] == len(b) and np.array_equal(ids[ptr[i]:ptr[i + 1]], b), i

    A, seed, st = 70, 13, T.stream_id(T.STREAM_N_BOR, 'train', 0)            # more than 64 slots
    anchors, sims, counts = ops.khop_border_sample(dg, r, 1, A, seed, st, bitmap_in_lds=lds)
    assert counts.tolist() == [len(b) for b in borders]
    an, mx = anchors.cpu().numpy(), max(len(b) for b in borders)
    for i, b in enumerate(borders):
        for s in range(A):
            kk = T.nanchor_pick(seed, st, i * A + s, len(b), len(b) < mx)
            assert an[i, s] == (0 if kk < 0 else b[kk]), (i, s)
    a, w, c = ops.draw_border_anchors(kept, A, seed, st)
    assert torch.equal(a, anchors) and torch.equal(w, sims) and torch.equal(c, counts)
    perm = torch.from_numpy(np.random.default_rng(8).permutation(len(sets)).astype(np.int32)).to(DEV)
    a, w, c = ops.khop_border_sample(dg, r, 1, A, seed, st, bitmap_in_lds=lds, order=perm)
    assert torch.equal(a, anchors) and torch.equal(w, sims) and torch.equal(c, counts)


# ---- pass level ---------------------------------------------------------------------------

def _same(x, y, where=''):
    if isinstance(x, torch.Tensor):
        assert torch.equal(x, y), where
    elif isinstance(x, dict):
        assert set(x) == set(y), where
        for k in x:
            _same(x[k], y[k], '%s/%s' % (where, k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), where
        for i, (p, q) in enumerate(zip(x, y)):
            _same(p, q, '%s/%d' % (where, i))
    elif hasattr(x, 'dense'):
        _same(x.dense(), y.dense(), where)
    else:
        assert x == y, where


def _border_half(st, L):
    """What a prepared pass holds of the neighbourhood-border stage."""
    torch.cuda.synchronize()
    sims = st.attrs['train_neigh_pos_similarities']
    return {'anchors': {l: st.per_split['anchors_neigh_border'][l] for l in range(L)},
            'sims': {l: sims[('N', 'out', l)] for l in range(L)},
            'plans': dict(st.per_split['_mpn_edge_plans'])}


def _pass_models(tmp_path, budgets):
    from conftest import load_golden
    from test_gpu_hotpath import _models
    golden = load_golden('density')
    out = []
    while len(out) < len(budgets):
        d = tmp_path / ('m%d' % len(out))
        d.mkdir()
        out += _models(golden, d, {'n_layers': 2, 'neigh_sample_border_size': 1})
    out = out[:len(budgets)]
    for m, b in zip(out, budgets):
        if b is not None:
            m.hparams['kept_border_bytes'] = b
        m._deterministic = True                          # (the border layer's edge plans are part of the comparison)
    return out


def test_a_pass_draws_from_kept_borders_like_the_fused_call(tmp_path):
    from subgnn_amd import hotpath, ops
    kept_m, fused_m, tiny_m = _pass_models(tmp_path, (None, 0, 1))
    L = 2
    firsts = {}
    for name, kw in (('pass 1', {}), ('pass 2', {}), ('epoch 1', {'epoch': 1})):
        got = _border_half(hotpath.prepare_pass(kept_m, 'train', **kw), L)
        want = _border_half(hotpath.prepare_pass(fused_m, 'train', **kw), L)
        small = _border_half(hotpath.prepare_pass(tiny_m, 'train', **kw), L)
        _same(got, want, name)
        _same(small, want, name + ' (budget of one byte)')
        firsts[name] = got
    _same(firsts['pass 2']['anchors'], firsts['pass 1']['anchors'], 'same epoch, same draws')
    assert any(not torch.equal(firsts['epoch 1']['anchors'][l], firsts['pass 1']['anchors'][l]) for l in range(L))
    # what is kept: one object for the split under the default budget, a remembered "no" otherwise
    def borders(m):
        return list(m.__dict__['_split_facts']['train'].borders.values())
    (rec,) = borders(kept_m)
    assert isinstance(rec, ops.KeptBorders) and rec.n == firsts['pass 1']['anchors'][0].shape[0] * firsts['pass 1']['anchors'][0].shape[1]
    assert borders(fused_m) == []
    assert borders(tiny_m) == [None]
    # the split's subgraph list replaced by a different one: the kept object is rebuilt (another list object is another
    # record: nothing has to be forgotten by hand)
    for m in (kept_m, fused_m):
        m.train_sub_G = list(m.train_sub_G)[::-1]
    got = _border_half(hotpath.prepare_pass(kept_m, 'train'), L)
    want = _border_half(hotpath.prepare_pass(fused_m, 'train'), L)
    _same(got, want, 'replaced subgraph list')
    assert len(borders(kept_m)) == 1 and isinstance(borders(kept_m)[0], ops.KeptBorders) and borders(kept_m)[0] is not rec
    assert any(not torch.equal(got['anchors'][l], firsts['pass 1']['anchors'][l]) for l in range(L))
    # a pass prepared on a second stream after one prepared on the first
    second = torch.cuda.Stream()
    second.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(second):
        got2 = _border_half(hotpath.prepare_pass(kept_m, 'train'), L)
    _same(got2, want, 'second stream')
    # ... and one whose first pass (the build) ran on a stream other than the consumer's
    kept_m.__dict__['_split_facts']['train'].borders.clear()
    with torch.cuda.stream(second):
        st3 = hotpath.prepare_pass(kept_m, 'train')
    st4 = hotpath.prepare_pass(kept_m, 'train')          # (no synchronisation in between: the kept border's event orders it)
    _same(_border_half(st3, L), want, 'built on the second stream')
    _same(_border_half(st4, L), want, 'drawn on the first stream from a border built on the second')

"""-m gpu: the node-overlap kernels (sgnn_overlap_topk / sgnn_overlap_diverse, ops.overlap_topk / overlap_diverse) against the
definitions of tests/overlap_cases.py.  Everything is an integer, so every comparison is exact: rows, shared nodes and rows
met for every case and measure, the scores as the float32 of the float64 quotient, the same bits in forced small chunks and on
guarded outputs of the raw entry; the greedy selection; ``SubgraphIndex.overlaps`` / ``self_overlaps`` (also from a saved
file), the CLI in a child process with its ``-summary`` against brute force, and ``discover(max_overlap=...)``."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import overlap_cases as OC
from test_gpu_predict import run                                   # noqa: F401  (the module's fixture: the tiny two-epoch run)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def _ragged(sets):
    from subgnn_amd import ops
    return ops.Ragged.from_lists([np.asarray(s, dtype=np.int32) for s in sets], DEV)


def _case(name):
    """(queries, bank, brute-force intersections, SetBank, query Ragged), computed once."""
    if name not in _REF:
        from subgnn_amd import ops
        queries, bank = OC.SEARCH_CASES[name]() if name in OC.SEARCH_CASES else getattr(OC, name + '_case')()[:2]
        _REF[name] = (queries, bank, OC.intersections(queries, bank), ops.SetBank(_ragged(bank)), _ragged(queries))
    return _REF[name]


def _want(name, measure, exclude=None):
    key = (name, measure, None if exclude is None else tuple(exclude.tolist()))
    if key not in _REF:
        queries, bank, I, _, _ = _case(name)
        _REF[key] = OC.topk(queries, bank, OC.MAX_K, measure, exclude, inter=I)
    return _REF[key]


def _same(got, want, k, what):
    rows, inter, touched, scores = (t.cpu().numpy() for t in got)
    assert rows.dtype == np.int64 and inter.dtype == np.int32 and touched.dtype == np.int32 and scores.dtype == np.float32
    assert np.array_equal(rows, want[0][:, :k]), what
    assert np.array_equal(inter, want[1][:, :k]), what
    assert np.array_equal(touched, want[2]), what
    assert np.array_equal(scores, want[3][:, :k]), what


@pytest.mark.parametrize('measure', OC.MEASURES)
@pytest.mark.parametrize('name', sorted(OC.SEARCH_CASES))
def test_topk_equals_the_definition(name, measure):
    from subgnn_amd import ops
    _, _, _, bank, q = _case(name)
    want = _want(name, measure)
    for k in OC.KS:
        _same(ops.overlap_topk(q, bank, k, measure), want, k, (name, measure, k))
    # the same in forced small chunks, and with a workspace budget that one posting table already exceeds
    _same(ops.overlap_topk(q, bank, 2, measure, chunk_queries=1), want, 2, (name, measure, 'one query per chunk'))
    _same(ops.overlap_topk(q, bank, 64, measure, chunk_queries=2, ws_budget=48), want, 64, (name, measure, 'chunks of two'))


def test_tiers_are_the_ones_restated():
    from subgnn_amd import ops
    assert ops.overlap_lds_max() == OC.LDS_MAX and ops.OVERLAP_MAX_K == OC.MAX_K
    queries, bank, _, sb, q = _case('tiers')
    P = ops.set_postings(q, sb).tolist()
    assert P == [OC.postings_walked(x, bank) for x in queries] == [OC.LDS_MAX - 1, OC.LDS_MAX, OC.LDS_MAX + 1]
    queries, bank, _, sb, q = _case('lengths')
    assert ops.set_postings(q, sb).tolist() == [OC.postings_walked(x, bank) for x in queries]
    held = {}
    for r, b in enumerate(bank):
        for v in b.tolist():
            held.setdefault(v, []).append(r)
    pp, pr = sb.post_ptr.cpu().numpy(), sb.post_rows.cpu().numpy()
    assert sb.max_id == max(held) and len(pp) == sb.max_id + 2 and sb.sizes.tolist() == [len(b) for b in bank]
    assert all(pr[pp[v]:pp[v + 1]].tolist() == held.get(v, []) for v in range(sb.max_id + 1))


@pytest.mark.parametrize('measure', ('jaccard', 'coverage'))
def test_exclude_and_k_around_the_rows_met(measure):
    from subgnn_amd import ops
    queries, bank, exclude = OC.touched_case()
    _, _, _, sb, q = _case('touched')
    want = _want('touched', measure, exclude)
    assert want[2].tolist() == [2, 2, 2] and (want[0][:, :3] >= 0).sum(1).tolist() == [1, 2, 2]
    ex = torch.from_numpy(exclude).to(DEV)
    for k in (1, 2, 3, 64):
        _same(ops.overlap_topk(q, sb, k, measure, exclude=ex), want, k, (measure, k))
    _same(ops.overlap_topk(q, sb, 3, measure, exclude=ex, chunk_queries=2), want, 3, (measure, 'chunks'))
    _same(ops.overlap_topk(q, sb, 3, measure), _want('touched', measure), 3, (measure, 'no exclude'))


def test_more_queries_than_the_grid():
    from subgnn_amd import ops
    _, _, _, sb, q = _case('many')
    assert q.n == OC.MANY > OC.GRID_CAP
    want = _want('many', 'jaccard')
    assert 0 < int((want[2] == 0).sum()) < OC.MANY
    _same(ops.overlap_topk(q, sb, 2, 'jaccard'), want, 2, 'many')


class Guarded:
    """A device buffer of ``n`` elements with GUARD sentinel words on either side."""

    def __init__(self, n, dtype, fill=-7):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _raw_topk(name, k, measure, **over):
    """The entry called as ops.overlap_topk calls it, on guarded outputs and a guarded workspace -> (rc, buffers)."""
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    _, _, _, sb, q = _case(name)
    P = ops.set_postings(q, sb)
    big = torch.where(P > OC.LDS_MAX, P, torch.zeros_like(P))
    off = (torch.cumsum(big, 0) - big).contiguous()
    entries = int(big.sum())
    nbytes = int(lib.sgnn_overlap_workspace_bytes(entries))
    assert nbytes == 48 * entries
    bufs = {'rows': Guarded(q.n * k, torch.int64), 'inter': Guarded(q.n * k, torch.int32), 'touched': Guarded(q.n, torch.int32),
            'ws': Guarded(nbytes // 4, torch.int32)}
    a = dict(q_ptr=ops._ptr(q.ptr), q_nodes=ops._ptr(q.nodes), n=q.n, P=ops._ptr(P), off=ops._ptr(off), b_ptr=ops._ptr(sb.sets.ptr),
             B=sb.n, pp=ops._ptr(sb.post_ptr), pr=ops._ptr(sb.post_rows), max_id=sb.max_id, exclude=None, K=k,
             M=ops.OVERLAP_MEASURES[measure], ws=bufs['ws'].ptr, entries=entries, nbytes=nbytes, rows=bufs['rows'].ptr,
             inter=bufs['inter'].ptr, touched=bufs['touched'].ptr)
    a.update(over)
    rc = lib.sgnn_overlap_topk(*a.values(), ops._stream())
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize('name', ('tiers', 'collision', 'lengths'))
def test_guard_words_around_every_output(name):
    for k, measure in ((1, 'jaccard'), (64, 'coverage')):
        rc, bufs = _raw_topk(name, k, measure)
        assert rc == 0
        for key, b in bufs.items():
            assert b.intact(), 'guard words of ' + key
        want = _want(name, measure)
        n = want[2].shape[0]
        assert np.array_equal(bufs['rows'].t.view(n, k).cpu().numpy(), want[0][:, :k])
        assert np.array_equal(bufs['inter'].t.view(n, k).cpu().numpy(), want[1][:, :k])
        assert np.array_equal(bufs['touched'].t.cpu().numpy(), want[2])


def test_refused_calls_write_nothing():
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    refused = []
    for over in (dict(n=-1), dict(n=2 ** 31), dict(B=-1), dict(max_id=-1), dict(K=0), dict(K=65), dict(M=4), dict(M=-1),
                 dict(entries=-1), dict(nbytes=47), dict(ws=None), dict(off=None), dict(q_ptr=None), dict(q_nodes=None), dict(P=None),
                 dict(b_ptr=None), dict(pp=None), dict(pr=None), dict(rows=None), dict(inter=None), dict(touched=None)):
        rc, bufs = _raw_topk('tiers', 2, 'jaccard', **over)
        refused.append(rc)
        assert all(b.untouched() for b in bufs.values()), over
    assert refused == [-1] * len(refused), refused
    assert lib.sgnn_overlap_workspace_bytes(-1) < 0 and lib.sgnn_overlap_workspace_bytes((1 << 28) + 1) < 0
    sets = _ragged(OC.chain_sets())
    sb = ops.SetBank(sets)
    P = ops.set_postings(sets, sb)
    acc, n, by = Guarded(4, torch.int64), Guarded(1, torch.int32), Guarded(3, torch.int32)

    def call(**over):
        a = dict(ptr=ops._ptr(sets.ptr), nodes=ops._ptr(sets.nodes), N=3, P=ops._ptr(P), pp=ops._ptr(sb.post_ptr), pr=ops._ptr(sb.post_rows),
                 max_id=sb.max_id, num=1, den=2, top=4, ws=None, entries=0, nbytes=0, acc=acc.ptr, n=n.ptr, by=by.ptr)
        a.update(over)
        rc = lib.sgnn_overlap_diverse(*a.values(), ops._stream())
        torch.cuda.synchronize()
        return rc
    for over in (dict(N=-1), dict(top=0), dict(top=2 ** 31), dict(den=0), dict(num=3), dict(num=-1), dict(den=(1 << 20) + 1),
                 dict(max_id=-2), dict(entries=5), dict(entries=-1), dict(ptr=None), dict(nodes=None), dict(P=None), dict(pp=None),
                 dict(pr=None), dict(acc=None), dict(n=None), dict(by=None)):
        assert call(**over) == -1, over
    assert acc.untouched() and n.untouched() and by.untouched()
    assert call() == 0 and acc.intact() and n.intact() and by.intact()
    assert acc.t.tolist() == [0, 2, -1, -1] and n.t.tolist() == [2] and by.t.tolist() == [-1, 0, -1]
    for bad in (dict(k=0), dict(k=65), dict(k=2.0), dict(measure='cosine'), dict(chunk_queries=0), dict(ws_budget=10)):
        with pytest.raises(ValueError):
            ops.overlap_topk(sets, sb, **dict(dict(k=2), **bad))
    with pytest.raises(TypeError):
        ops.overlap_topk(sets, sets, 2)
    for unsorted in ([[2, 1]], [[1, 1]], [[1, 2], [-1, 3]]):
        with pytest.raises(ValueError):
            ops.SetBank(_ragged(unsorted))
        with pytest.raises(ValueError):
            ops.overlap_topk(_ragged(unsorted), sb, 1)


@pytest.mark.parametrize('name', sorted(OC.DIVERSE_CASES))
def test_diverse_equals_the_greedy_loop(name):
    from subgnn_amd import ops
    make, taus, tops = OC.DIVERSE_CASES[name]
    sets = make()
    r = _ragged(sets)
    for tau in taus:
        for top in tops:
            want_acc, want_n, want_by = OC.greedy(sets, OC.threshold(tau), top)
            acc, n, by = ops.overlap_diverse(r, tau, top)
            assert acc.dtype == torch.int64 and n.dtype == by.dtype == torch.int32 and acc.shape == (top,) and n.shape == (1,)
            assert n.tolist() == [want_n], (name, tau, top)
            assert np.array_equal(acc.cpu().numpy(), want_acc), (name, tau, top)
            assert np.array_equal(by.cpu().numpy(), want_by), (name, tau, top)
    if name == 'past_lds':
        assert ops.set_postings(r, ops.SetBank(r))[0].item() > OC.LDS_MAX
    with pytest.raises(ValueError):
        ops.overlap_diverse(r, 1.5, 3)
    with pytest.raises(ValueError):
        ops.overlap_diverse(r, 0.5, 0)


# ---------------------------------------------------------------------------------------------------------- index, CLI, discover
TINY = [[4, 1, 2], [2, 3], [9], [1, 2, 4], [2, 2, 3, 7], [], [11, 12]]
TINY_SPLITS = ['train', 'train', 'train', 'val', 'val', 'test', 'test']


def _tiny_index():
    from subgnn_amd.neighbors import SubgraphIndex
    E = torch.arange(len(TINY) * 3, dtype=torch.float32).view(len(TINY), 3)
    return SubgraphIndex(E, TINY, [['a']] * len(TINY), TINY_SPLITS, [0, 1, 2, 0, 1, 0, 1])


def test_index_overlaps_and_self_overlaps(tmp_path):
    from subgnn_amd.neighbors import SubgraphIndex
    idx = _tiny_index()
    bank = [OC.arr(set(s)) for s in TINY]
    requests = [[3, 2, 2], [], [100], [4, 2, 1, 50]]
    queries = [OC.arr(set(s)) for s in requests]
    path = tmp_path / 'tiny.npz'
    idx.save(str(path))
    for index in (idx, SubgraphIndex.load(str(path)), idx.__class__(idx.embeddings.to(DEV), TINY)):
        for measure in OC.MEASURES:
            got = index.overlaps(requests, k=3, measure=measure)
            _same((got['rows'], got['inter'], got['touched'], got['scores']), OC.topk(queries, bank, 3, measure), 3, measure)
            me = np.arange(len(TINY), dtype=np.int64)
            own = index.self_overlaps(k=2, measure=measure)
            _same((own['rows'], own['inter'], own['touched'], own['scores']), OC.topk(bank, bank, 2, measure, me), 2, measure)
        assert index._overlap_bank() is index._overlap_bank()
    assert got['rows'][1].tolist() == [-1, -1, -1] and got['touched'].tolist()[1:3] == [0, 0]      # an empty request, an unknown id
    with pytest.raises(ValueError):
        idx.overlaps([[1, -2]])
    with np.load(str(path)) as z:                                      # the file's format did not change
        assert sorted(z.files) == sorted(['embeddings', 'sub_ptr', 'sub_ids', 'lab_ptr', 'lab_names', 'splits', 'rows', 'metric',
                                          'checkpoint'])


def _brute_summary(subs, splits, order):
    out = []
    for a in order:
        for b in order:
            if a == b:
                continue
            A = [set(s) for s, sp in zip(subs, splits) if sp == a]
            B = [set(s) for s, sp in zip(subs, splits) if sp == b]
            best = [max([OC.Fraction(len(x & y), len(x | y)) for y in B if x & y] + [OC.Fraction(0)]) for x in A]
            out.append({'first': a, 'second': b, 'rows': len(A), 'identical': sum(f == 1 for f in best),
                        'jaccard_ge_half': sum(f >= OC.Fraction(1, 2) for f in best),
                        'mean_best_jaccard': float(np.mean([float(f) for f in best]))})
    return out


def test_cli_in_a_child_process(tmp_path):
    from subgnn_amd import overlap
    rng = np.random.default_rng(5)
    subs = [sorted(rng.choice(30, size=int(rng.integers(1, 7)), replace=False).tolist()) for _ in range(40)]
    subs[21], subs[36] = subs[2], sorted(set(subs[3] + [29]))          # a copy and a near-copy across splits
    splits = ['train'] * 20 + ['val'] * 10 + ['test'] * 10             # (val is not the smaller split: no swap)
    data = tmp_path / 'data'
    data.mkdir()
    (data / 'subgraphs.pth').write_text(''.join('%s\t%s\t%s\t\n' % ('-'.join(map(str, s)), 'xy'[i % 2], sp)
                                                for i, (s, sp) in enumerate(zip(subs, splits))))
    req = tmp_path / 'req.txt'
    req.write_text('3-1-2\n\n29\n5-5-6\tignored\n')
    out, summary, own = tmp_path / 'out.txt', tmp_path / 'sum.json', tmp_path / 'own.txt'
    env = dict(os.environ, PYTHONPATH=REPO)
    base = [sys.executable, '-m', 'subgnn_amd.overlap', str(data)]
    r = subprocess.run(base + ['-out', str(out), '-subgraphs', str(req), '-k', '3', '-measure', 'containment', '-summary', str(summary)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    index = overlap.index_of_dataset(data)
    assert index.subgraphs == subs and index.splits == splits
    res = index.overlaps([[3, 1, 2], [29], [5, 5, 6]], 3, 'containment')
    got = out.read_text().splitlines()
    assert got[0] == overlap.HEADER and got[1:] == overlap.lines_of(index, res) and len(got) == 1 + 3 * 3
    bank = [OC.arr(set(s)) for s in subs]
    want = OC.topk([OC.arr([1, 2, 3]), OC.arr([29]), OC.arr([5, 6])], bank, 3, 'containment')
    cols = [l.split('\t') for l in got[1:]]
    assert [int(c[5]) if c[4] else -1 for c in cols] == [(index.rows[j] if j >= 0 else -1) for j in want[0].reshape(-1)]
    assert [c[2] for c in cols] == ['%.9g' % s for s in want[3].reshape(-1)] and [int(c[3]) for c in cols] == want[1].reshape(-1).tolist()
    s = json.loads(summary.read_text())
    brute = _brute_summary(subs, splits, ('train', 'val', 'test'))
    assert s['splits'] == ['train', 'val', 'test'] and len(s['pairs']) == 6
    for g, w in zip(s['pairs'], brute):
        assert {k: g[k] for k in ('first', 'second', 'rows', 'identical', 'jaccard_ge_half')} == {k: w[k] for k in w if k != 'mean_best_jaccard'}
        assert abs(g['mean_best_jaccard'] - w['mean_best_jaccard']) <= 1e-12
    assert [p['identical'] for p in s['pairs'] if (p['first'], p['second']) == ('val', 'train')] == [brute[2]['identical']] and brute[2]['identical'] >= 1
    # every row's best other rows, of two splits only (in process: the same code path without the start of a child)
    overlap.main([str(data), '-out', str(own), '-k', '2', '-splits', 'val,test'])
    sub = overlap.index_of_dataset(data, ('val', 'test'))
    lines = own.read_text().splitlines()
    assert lines[0] == overlap.HEADER and lines[1:] == overlap.lines_of(sub, sub.self_overlaps(2)) and len(lines) == 1 + 20 * 2
    me = np.arange(20, dtype=np.int64)
    want = OC.topk(bank[20:], bank[20:], 2, 'jaccard', me)
    assert [int(l.split('\t')[3]) for l in lines[1:]] == want[1].reshape(-1).tolist()


def test_discover_with_max_overlap(run):
    from subgnn_amd.predict import Predictor
    m = run['model']
    g = m.networkx_graph
    P = Predictor(m)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).cpu().numpy()
    seeds = [int(v) - 1 for v in np.nonzero(deg > 0)[0][3:43:4]]
    kw = dict(sizes=(3, 6), per_seed=4)
    plain = P.discover(seeds, top=None, **kw)
    none = P.discover(seeds, top=None, max_overlap=None, **kw)
    assert plain.keys() == none.keys() and 'n_suppressed' not in plain
    for key, v in plain.items():
        assert torch.equal(v, none[key]) if isinstance(v, torch.Tensor) else v == none[key], key
    sets = [OC.arr(s) for s in plain['subgraphs']]
    n = len(sets)
    assert n > len(seeds)                                              # two candidates of one seed: they share the seed
    dev = plain['item'].device
    for tau, top, pool in ((0.5, 6, 4096), (0.5, None, 4096), (0.0, 4, 4096), (0.25, 5, 7), (0.0, None, 4096), (1.0, 6, 4096)):
        got = P.discover(seeds, top=top, max_overlap=tau, overlap_pool=pool, **kw)
        size = min(pool, n)
        acc, cnt, by = OC.greedy(sets[:size], OC.threshold(tau), size if top is None else top)
        pick = torch.from_numpy(acc[:cnt].copy()).to(dev)
        print('max_overlap %s, top %s, pool %d: %d kept, %d suppressed' % (tau, top, pool, cnt, int((by >= 0).sum())))
        assert got['item'].tolist() == plain['item'][pick].tolist(), (tau, top, pool)
        assert got['subgraphs'] == [plain['subgraphs'][i] for i in acc[:cnt]] and got['n_suppressed'] == int((by >= 0).sum())
        assert torch.equal(got['score'], plain['score'][pick]) and torch.equal(got['keys'], plain['keys'][pick])
        assert tau != 0.0 or top is not None or got['n_suppressed'] >= 1
        kept = [set(s) for s in got['subgraphs']]
        assert all(len(a & b) * OC.threshold(tau).denominator <= OC.threshold(tau).numerator * len(a | b)
                   for i, a in enumerate(kept) for b in kept[:i])                 # every returned pair: Jaccard <= tau
    assert got['item'].tolist() == plain['item'][:6].tolist() and got['n_suppressed'] == 0      # tau = 1: the plain top list
    for bad in (dict(max_overlap=1.5), dict(max_overlap=-0.5), dict(max_overlap=0.5, overlap_pool=0)):
        with pytest.raises(ValueError):
            P.discover(seeds, **dict(kw, **bad))

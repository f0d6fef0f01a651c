"""-m gpu: add-one-candidate scoring (subgnn_amd/suggest.py, Predictor.suggest / grow, ops.insertion_sets) end to end.

  * variants: what is prepared for the variants built on the device is exactly what ``Predictor.prepare`` computes for the node
    lists ``S + [v]`` sent as an ordinary request (anchors, similarities, component ids), with border candidates and with a
    pool; their logits are those of that request (within helpers.assert_close, and bit for bit: the padded shapes are equal);
  * gains: ``gain_logit``, ``gain_prob`` and the CLI's ``label_with`` follow from the base and variant logits;
  * draws: draw 0 is ``predict``; mean and standard deviation are those of the per-draw values recomputed with
    ``prepare_sets(..., epoch_offset=d)``;
  * untouched components: a component of the parent without an edge to the added node keeps its neighbourhood anchors, border
    anchors with their hop similarities and structure similarities, bit for bit, at every draw;
  * candidates: the one-hop border through the kept-border kernels is the k-hop border search's, without members; two hops hold
    one hop; a pool loses unknown ids and members, and a request that is left without a candidate is no error;
  * chunking (``max_variants=3``), ``grow``, no leak into the model's own splits, the CLI in a fresh child process.

Inputs: the two-epoch ``cc`` run of tests/test_gpu_predict.py and its six requests (tests/test_gpu_explain.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close
from test_gpu_predict import run, _requests, _snapshot, _split_objects          # noqa: F401  (run: the module's fixture)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT = ('anchors_neigh_int/', 'anchors_neigh_border/', 'sim/N/out/', 'S_sim/')


def _ball(nbr, s, hops):
    seen, front = set(s), set(s)
    for _ in range(hops):
        front = {w for v in front for w in nbr[v]} - seen
        seen |= front
    return sorted(seen - set(s))


@pytest.fixture(scope='module')
def ctx(run):
    """The predictor of the run, the requests, their mapped sets (model ids), the graph's neighbour lists, every request's
    one-hop border from them, and a pool (dataset numbering) of known ids -- members of request 0 and border nodes among them --
    unknown ids and a repeat, with the known ones in model ids."""
    from subgnn_amd.predict import Predictor
    m = run['model']
    g = m.networkx_graph
    P = Predictor(m)
    A, B = _requests(g)
    req = A + B
    subgraphs = P.request_sets(req).to_lists()
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    nbr = {v: sorted({int(w) for w in col[rp[v]:rp[v + 1]]} - {v}) for v in range(1, g.max_id + 1)}
    border = [_ball(nbr, s, 1) for s in subgraphs]
    known = sorted(set(subgraphs[0]) | set(border[1][:6]) | set(border[5][:4]) | set(subgraphs[4][:2]))
    assert all(nbr[v] for v in known)
    pool = [v - 1 for v in known[::-1]] + [10 ** 6, -3, g.max_id, known[0] - 1]
    return dict(P=P, m=m, g=g, hp=m.hparams, req=req, subgraphs=subgraphs, nbr=nbr, border=border, pool=pool, known=known)


def _expected(ctx, mode):
    if mode == 'border':
        return ctx['border']
    return [[v for v in ctx['known'] if v not in s] for s in ctx['subgraphs']]


@pytest.mark.parametrize('mode', ['border', 'pool'])
def test_variants_are_ordinary_requests(ctx, mode):
    from subgnn_amd import ops, suggest
    P, hp, req = ctx['P'], ctx['hp'], ctx['req']
    cands = 'border' if mode == 'border' else ctx['pool']
    expected = _expected(ctx, mode)
    assert all(len(e) > 0 for e in expected) and (mode == 'border' or any(len(e) < len(ctx['known']) for e in expected))
    res = P.suggest(req, candidates=cands)
    ptr, cn = res['ptr'].tolist(), res['candidate_nodes'].tolist()
    assert res['candidate_nodes'].dtype == torch.int64 and res['subgraphs'] == ctx['subgraphs']
    assert [cn[ptr[r]:ptr[r + 1]] for r in range(len(req))] == expected          # ascending, members and unknown ids gone
    explicit = [[v - 1 for v in s] + [c - 1] for s, e in zip(ctx['subgraphs'], expected) for c in e]
    sets = P.request_sets(req)
    rows, shared = suggest.candidate_rows(P, sets, cands, 1)
    assert shared == (mode == 'pool') and rows.n == (1 if shared else sets.n)
    ins = ops.insertion_sets(sets, rows, shared)
    assert ins.parent.tolist() == [r for r, e in enumerate(expected) for _c in e] and ins.cand.tolist() == cn
    assert torch.equal(ins.keys, ops.set_keys(ins.sets))
    st_v = P.prepare_sets(ins.sets, sub_keys=ins.keys)
    got = _snapshot(st_v, hp)
    st_e = P.prepare(explicit)
    want = _snapshot(st_e, hp)
    assert st_v.subgraphs == st_e.subgraphs == [sorted(v + 1 for v in l) for l in explicit]
    assert torch.equal(st_v.keys['subgraphs'], st_e.keys['subgraphs']) and torch.equal(st_v.keys['components'], st_e.keys['components'])
    assert got.keys() == want.keys() and len(got) == 1 + 4 * hp['n_layers'] + 3 * hp['n_layers'] + 2
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    want_logits = P.forward_prepared(st_e)[0].float().cpu()
    through_predict = P.predict(explicit)['logits'].cpu()
    vl = res['variant_logits'].cpu()
    print('variant logits, %s candidates: %d variants, largest absolute difference %.3e' % (mode, len(cn), float((vl - want_logits).abs().max())))
    assert_close(vl, want_logits, 'variant logits, %s candidates' % mode)
    assert_close(vl, through_predict, 'variant logits against predict, %s candidates' % mode)
    assert torch.equal(vl, want_logits) and torch.equal(vl, through_predict)     # one chunk: the padded shapes are the request's


def test_gains_follow_from_the_logits(ctx):
    from subgnn_amd import suggest
    P, req = ctx['P'], ctx['req']
    res = P.suggest(req)
    assert 'valid' not in res
    base, vl, tgt, ptr = res['logits'].cpu(), res['variant_logits'].cpu(), res['target'].cpu(), res['ptr'].tolist()
    assert tgt.dtype == torch.int64 and torch.equal(tgt, base.argmax(-1))
    assert torch.equal(res['probabilities'], torch.softmax(res['logits'], -1))
    gl, gs, gp = res['gain_logit'].cpu(), res['gain_std'].cpu(), res['gain_prob'].cpu()
    assert gl.shape == gs.shape == gp.shape == (ptr[-1],) and vl.shape == (ptr[-1], base.shape[1])
    b64, v64 = base.double(), vl.double()
    pb, pv = torch.softmax(b64, -1), torch.softmax(v64, -1)

    def check(res_gl, res_gp, targets):
        for r in range(len(req)):
            t = int(targets[r])
            for u in range(ptr[r], ptr[r + 1]):
                g = float(v64[u, t] - b64[r, t])                       # exact in float64; the device rounds it once to float32
                assert abs(float(res_gl[u]) - g) <= 2.0 ** -23 * abs(g), (r, u)
                # two float32 softmax values of the same logits, each within a few units of 2^-24 of the host's
                assert abs(float(res_gp[u]) - float(pv[u, t] - pb[r, t])) <= 1e-6, (r, u)
    check(gl, gp, tgt)
    assert bool((gs == 0).all()) and bool((gl != 0).any())
    # a given target: an int, a sequence; values outside the classes and a wrong length are errors
    K = base.shape[1]
    other = [(int(t) + 1) % K for t in tgt]
    res2 = P.suggest(req, target=other)
    assert res2['target'].tolist() == other and torch.equal(res2['variant_logits'].cpu(), vl)
    check(res2['gain_logit'].cpu(), res2['gain_prob'].cpu(), other)
    assert P.suggest(req, target=K - 1)['target'].tolist() == [K - 1] * len(req)
    for bad in (K, -1, [0] * (len(req) + 1), [0] * (len(req) - 1) + [K]):
        with pytest.raises(ValueError):
            P.suggest(req, target=bad)
    for kw in (dict(candidates='edge'), dict(hops=0), dict(hops=1.5), dict(draws=0), dict(batch_size=0), dict(max_variants=0),
               dict(max_variants=2.5)):
        with pytest.raises(ValueError):
            P.suggest(req, **kw)
    # the lines: label_with is the label of the variant's logits, candidates by descending gain_logit, then ascending id
    lines = [l.split('\t') for l in suggest.lines_of(P, res)]
    assert len(lines) == ptr[-1]
    cn = res['candidate_nodes'].tolist()
    for r in range(len(req)):
        mine = [l for l in lines if int(l[0]) == r]
        order = suggest.candidate_order(gl[ptr[r]:ptr[r + 1]].tolist(), cn[ptr[r]:ptr[r + 1]])
        assert len(mine) == len(order) == ptr[r + 1] - ptr[r]
        for l, k in zip(mine, order):
            u = ptr[r] + k
            assert l[1] == str(cn[u] - 1) and l[5] == P.names_of(vl[u].argmax())[0] and l[2] == '%.9g' % float(gl[u])
        got = [float(l[2]) for l in mine]
        assert got == sorted(got, reverse=True)


def test_draws(ctx):
    from subgnn_amd import ops, suggest
    P, req = ctx['P'], ctx['req']
    plain = P.predict(req)
    res1 = P.suggest(req, draws=1)
    for k in ('logits', 'probabilities', 'labels'):
        assert torch.equal(res1[k], plain[k]), k                       # draw 0 is predict's answer
    assert 'logits_mean' not in res1
    E = 3
    out = P.predict(req, draws=E)
    res = P.suggest(req, draws=E)
    for k in ('logits', 'logits_mean', 'logits_std', 'probabilities_mean'):
        assert torch.equal(res[k], out[k]), k
    assert torch.equal(res['logits'], plain['logits'])
    sets = P.request_sets(req)
    rows, shared = suggest.candidate_rows(P, sets, 'border', 1)
    ins = ops.insertion_sets(sets, rows, shared)
    fwd = lambda s, d, keys: P.forward_prepared(P.prepare_sets(s, epoch_offset=d, want_lists=False, sub_keys=keys))[0].float()
    per_draw = torch.stack([fwd(sets, d, None) for d in range(E)])
    var = torch.stack([fwd(ins.sets, d, ins.keys) for d in range(E)])
    assert torch.equal(per_draw[0], plain['logits']) and torch.equal(res['target'], per_draw.mean(0).argmax(-1))
    assert torch.equal(var[0], res1['variant_logits'])
    parent, tgt = ins.parent.long(), res['target']
    diff = (var.gather(2, tgt[parent].view(1, -1, 1).expand(E, -1, 1)).squeeze(2)
            - per_draw.gather(2, tgt.view(1, -1, 1).expand(E, -1, 1)).squeeze(2)[:, parent])
    print('per-draw gain_logit: mean |.| %.3e, mean sample std %.3e' % (float(diff.mean(0).abs().mean()), float(diff.std(0).mean())))
    assert torch.equal(res['gain_logit'], diff.mean(0)) and torch.equal(res['variant_logits'], var.mean(0))
    assert torch.equal(res['gain_std'], diff.std(0, unbiased=True)) and bool((res['gain_std'] > 0).any())
    # the same in float64 on the host
    d64 = diff.double().cpu().numpy()
    assert np.allclose(res['gain_logit'].cpu().numpy(), d64.mean(0), rtol=1e-5, atol=1e-7)
    assert np.allclose(res['gain_std'].cpu().numpy(), d64.std(0, ddof=1), rtol=1e-4, atol=1e-7)


def test_components_the_new_node_does_not_touch_keep_their_draws(ctx):
    from subgnn_amd import ops
    P, hp, nbr = ctx['P'], ctx['hp'], ctx['nbr']
    members = ctx['subgraphs'][1]                                      # two single nodes and an adjacent pair
    sets = P.request_sets([ctx['req'][1]])
    cc = _snapshot(P.prepare_sets(sets, want_lists=False), hp)['cc_ids'][0]
    comps = [[int(v) for v in row if v != 0] for row in cc if row[0] != 0]
    assert sorted(len(c) for c in comps) == [1, 1, 2] and sorted(v for c in comps for v in c) == members
    touched = lambda v: [i for i, c in enumerate(comps) if any(w in nbr[v] for w in c)]
    v = next(v for v in ctx['border'][1] if len(touched(v)) == 1)      # an edge to one component, none to the other two
    free = [i for i in range(3) if i not in touched(v)]
    assert len(free) == 2 and all(v not in nbr[w] for i in free for w in comps[i])
    row = ops.Ragged(torch.tensor([0, 1], dtype=torch.int64, device=sets.ptr.device),
                     torch.tensor([v], dtype=torch.int32, device=sets.ptr.device), max_len=1)
    ins = ops.insertion_sets(sets, row)
    assert ins.sets.to_lists() == [sorted(members + [v])]
    checked = 0
    for d in range(3):
        base = _snapshot(P.prepare_sets(sets, epoch_offset=d, want_lists=False), hp)
        var = _snapshot(P.prepare_sets(ins.sets, epoch_offset=d, want_lists=False, sub_keys=ins.keys), hp)
        vcomps = [[int(x) for x in r if x != 0] for r in var['cc_ids'][0] if r[0] != 0]
        assert len(vcomps) == 3 and sorted(comps[touched(v)[0]] + [v]) in vcomps
        keys = [k for k in base if k.startswith(KEPT)]
        assert len(keys) == 3 * hp['n_layers'] + 2
        for i in free:
            j = vcomps.index(comps[i])
            for k in keys:
                assert torch.equal(var[k][0, j], base[k][0, i]), (d, i, k)
                checked += 1
    assert checked == 3 * 2 * (3 * hp['n_layers'] + 2)


def test_border_candidates(ctx):
    from subgnn_amd import ops, suggest
    P, g, req, nbr = ctx['P'], ctx['g'], ctx['req'], ctx['nbr']
    sets = P.request_sets(req)
    assert ops.khop1_applies(g, sets.n)                                # hops=1 goes through the kept-border kernels here
    rows, shared = suggest.candidate_rows(P, sets, 'border', 1)
    kept = ops.khop1_borders_sorted(g, sets)
    searched = ops.sort_ragged(ops.khop_border(g, sets, 1)).to_lists()
    without = lambda lists: [[v for v in b if v not in s] for b, s in zip(lists, ctx['subgraphs'])]
    assert not shared and rows.to_lists() == ops.Ragged(kept.ptr, kept.ids).to_lists()
    assert without(rows.to_lists()) == without(searched) == ctx['border']
    one, two = P.suggest(req, hops=1), P.suggest(req, hops=2)
    c1, c2, p1, p2 = one['candidate_nodes'].tolist(), two['candidate_nodes'].tolist(), one['ptr'].tolist(), two['ptr'].tolist()
    for r, s in enumerate(ctx['subgraphs']):
        a, b = c1[p1[r]:p1[r + 1]], c2[p2[r]:p2[r + 1]]
        assert a == ctx['border'][r] and b == _ball(nbr, s, 2) and set(a) <= set(b), r
    assert len(c2) > len(c1)


def test_a_pool_of_nothing_known_is_an_error(ctx):
    P, g, req = ctx['P'], ctx['g'], ctx['req']
    for pool in ([], [10 ** 6, -3, g.max_id]):
        with pytest.raises(ValueError, match='pool holds no node of the graph'):
            P.suggest(req, candidates=pool)
    # a pool of members only: every request skips its own, request 0 all of them
    res = P.suggest(req, candidates=[v - 1 for v in ctx['subgraphs'][0]])
    ptr = res['ptr'].tolist()
    assert ptr[1] == 0 and [ptr[r + 1] - ptr[r] for r in range(len(req))] == \
        [len(set(ctx['subgraphs'][0]) - set(s)) for s in ctx['subgraphs']]
    # a request without a candidate is no error: no variant, empty results of the right shapes
    alone = P.suggest(req[:1], candidates=[v - 1 for v in ctx['subgraphs'][0]], draws=2)
    assert alone['ptr'].tolist() == [0, 0] and alone['variant_logits'].shape == (0, res['logits'].shape[1])
    assert alone['gain_logit'].numel() == alone['gain_std'].numel() == alone['gain_prob'].numel() == 0
    assert torch.equal(alone['logits'], P.predict(req[:1])['logits'])


def test_chunks_of_three_variants(ctx):
    P, req = ctx['P'], ctx['req']
    calls, orig = [], P.prepare_sets

    def wrapped(sets, epoch_offset=0, want_lists=True, sub_keys=None):
        calls.append(sets.n)
        return orig(sets, epoch_offset=epoch_offset, want_lists=want_lists, sub_keys=sub_keys)
    P.prepare_sets = wrapped
    try:
        whole = P.suggest(req)
        n_whole = len(calls)
        parts = P.suggest(req, max_variants=3, batch_size=2)
    finally:
        P.__dict__.pop('prepare_sets')
    V = int(whole['ptr'][-1])
    assert n_whole == 2 and calls[:2] == [len(req), V]                 # the base request, then every variant at once
    assert calls[n_whole + 1:] == [3] * (V // 3) + ([V % 3] if V % 3 else [])
    assert torch.equal(parts['ptr'], whole['ptr']) and torch.equal(parts['candidate_nodes'], whole['candidate_nodes'])
    assert torch.equal(parts['target'], whole['target'])
    assert_close(parts['variant_logits'], whole['variant_logits'].cpu().numpy(), 'variant logits in chunks of 3')
    assert_close(parts['logits'], whole['logits'].cpu().numpy(), 'base logits in batches of 2')


@pytest.mark.parametrize('min_gain', [0.0, -1e9])
def test_grow(ctx, min_gain):
    """Two rounds, replayed with ``suggest`` and ``choose``: with the default bar (a request stops when nothing gains), and with
    a bar below every gain (every request takes a node in both rounds)."""
    from subgnn_amd import suggest
    P, req = ctx['P'], ctx['req']
    R = len(req)
    res = P.grow(req, 2, min_gain=min_gain)
    first = P.suggest(req)
    tgt = first['target'].tolist()
    assert res['target'].tolist() == tgt
    picks = suggest.choose(first['ptr'].tolist(), first['candidate_nodes'].tolist(), first['gain_logit'].tolist(), min_gain)
    active = [r for r in range(R) if picks[r] >= 0]
    assert [len(a) >= 1 for a in res['added']] == [picks[r] >= 0 for r in range(R)]
    assert min_gain == 0.0 or len(active) == R
    current = [[v - 1 for v in s] for s in ctx['subgraphs']]
    for r in active:
        u = picks[r]
        assert res['added'][r][0] == int(first['candidate_nodes'][u]) - 1
        assert res['gain_logit'][r][0] == float(first['gain_logit'][u]) > min_gain and res['gain_std'][r][0] == 0.0
        assert torch.equal(res['step_logits'][r][0], first['variant_logits'][u].cpu())
        current[r] = sorted(current[r] + [res['added'][r][0]])
    if active:
        second = P.suggest([current[r] for r in active], target=[tgt[r] for r in active])  # the targets of round 0
        picks2 = suggest.choose(second['ptr'].tolist(), second['candidate_nodes'].tolist(), second['gain_logit'].tolist(), min_gain)
        assert min_gain == 0.0 or all(u >= 0 for u in picks2)
        for i, r in enumerate(active):
            assert len(res['added'][r]) == (2 if picks2[i] >= 0 else 1)
            if picks2[i] >= 0:
                assert res['added'][r][1] == int(second['candidate_nodes'][picks2[i]]) - 1
                assert res['gain_logit'][r][1] == float(second['gain_logit'][picks2[i]])
                current[r] = sorted(current[r] + [res['added'][r][1]])
    assert res['subgraphs'] == current
    assert all(len(a) == len(g) == len(s) == len(z) for a, g, s, z in zip(res['added'], res['gain_logit'], res['gain_std'], res['step_logits']))
    assert_close(res['logits'], P.predict(current)['logits'].cpu().numpy(), 'the final logits')


def test_grow_stops_below_the_bar(ctx):
    P, req = ctx['P'], ctx['req']
    R = len(req)
    first = P.suggest(req)
    # a bar above every gain: nothing is added
    bar = float(first['gain_logit'].max())
    none = P.grow(req, 2, min_gain=bar)
    assert none['added'] == [[] for _ in range(R)] and none['subgraphs'] == [[v - 1 for v in s] for s in ctx['subgraphs']]
    assert torch.equal(none['logits'], first['logits'])
    just = P.grow(req, 1, min_gain=np.nextafter(np.float32(bar), np.float32(-np.inf)).item())
    assert sum(len(a) for a in just['added']) >= 1
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            P.grow(req, bad)


def test_the_models_own_splits_are_untouched(run, ctx):
    from subgnn_amd.predict import Predictor
    m, trainer = run['model'], run['trainer']
    trainer.test(m)
    before = dict(m.test_results)
    objs = _split_objects(m)
    was_training, sparse_mark = m.training, m.__dict__.get('_sparse_prepared')
    P = Predictor(m)
    A, B = _requests(m.networkx_graph)
    P.suggest(A, draws=2)
    P.suggest(B + A, candidates=ctx['pool'], max_variants=2)
    P.grow(B, 1, hops=2)
    after_objs = _split_objects(m)
    assert after_objs.keys() == objs.keys()
    for k, v in objs.items():
        assert after_objs[k] is v, k
    assert m.training == was_training and m.__dict__.get('_sparse_prepared') == sparse_mark
    trainer.test(m)
    assert set(m.test_results) == set(before)
    for k, v in before.items():
        assert float(m.test_results[k]) == float(v) or (np.isnan(float(v)) and np.isnan(float(m.test_results[k]))), k


def test_cli_in_a_child_process(run, ctx, tmp_path):
    from subgnn_amd import config, suggest
    from subgnn_amd.predict import Predictor
    root, results, req = run['root'], run['results'], ctx['req']
    f, pool, out, grown = (tmp_path / n for n in ('requests.txt', 'pool.txt', 'suggested.txt', 'grown.txt'))
    f.write_text(''.join('-'.join(str(v) for v in s) + '\n' for s in req))
    pool.write_text(' '.join(str(v) for v in ctx['pool'][:7]) + '\n' + '\n'.join(str(v) for v in ctx['pool'][7:]) + '\n')
    config.PROJECT_ROOT = root
    P = Predictor.from_run(run['rc'], results)
    label = P.label_names[-1]
    common = [sys.executable, '-m', 'subgnn_amd.suggest', '-config_path', str(run['cfg']), '-project_root', str(root),
              '-restoreModelPath', str(results), '-subgraphs', str(f)]

    def child(args):
        r = subprocess.run(common + args, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]

    child(['-out', str(out), '-target', label, '-draws', '2', '-top', '2', '-batch_size', '4'])
    got = out.read_text().splitlines()
    res = P.suggest(req, target=P.label_names.index(label), draws=2, batch_size=4)
    assert res['target'].tolist() == [len(P.label_names) - 1] * len(req)
    assert got[0] == suggest.HEADER and got[1:] == suggest.lines_of(P, res, top=2)
    assert [l.split('\t')[0] for l in got[1:]] == [str(r) for r in range(len(req)) for _ in range(min(2, len(ctx['border'][r])))]
    assert len(got) == 1 + 2 * len(req)

    child(['-out', str(grown), '-candidates', str(pool), '-grow', '2', '-min_gain', '-1000'])
    got = grown.read_text().splitlines()
    res = P.grow(req, 2, min_gain=-1000.0, candidates=ctx['pool'])
    assert got[0] == suggest.GROW_HEADER and got[1:] == suggest.grow_lines_of(P, res)
    # every request takes a node of the pool in both rounds: the bar is below every gain, and no request holds all of the pool
    assert [l.split('\t')[:2] for l in got[1:]] == [[str(r), str(k)] for r in range(len(req)) for k in range(2)]
    assert all(int(l.split('\t')[2]) + 1 in ctx['known'] for l in got[1:])

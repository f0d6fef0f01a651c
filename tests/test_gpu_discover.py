"""-m gpu: candidate subgraphs around seeds (subgnn_amd/discover.py, Predictor.discover, ops.seeded_walk_sets) end to end.

  * candidates: every returned subgraph is the regenerated set of its item -- connected walk sets around the seed -- and, sent
    as an ordinary request to ``Predictor.predict``, gives the returned logits (within helpers.assert_close);
  * ``score``, ``prob`` and ``labels`` follow from the logits; with several draws they are the mean and the sample standard
    deviation of per-draw forwards (``prepare_sets(..., epoch_offset=d)``);
  * a node set sampled more than once is scored once, under its smallest item; chunks (``max_variants=3``) change nothing;
  * ``known`` / ``novel``, ``top`` / ``top_per_seed`` and the order; unknown seed ids; no leak into the model's own splits; the
    CLI in a fresh child process.

Inputs: the two-epoch ``cc`` run of tests/test_gpu_predict.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close
from test_gpu_predict import run, _split_objects          # noqa: F401  (run: the module's fixture)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(sizes=(3, 6), per_seed=4)


@pytest.fixture(scope='module')
def ctx(run):
    """The predictor of the run, seeds in the dataset's numbering (ten nodes with an edge, descending, with ids that are no
    nodes and a repeat among them), the known ones ascending in model ids, and one ``discover`` call over them without a cut."""
    from subgnn_amd.predict import Predictor
    m = run['model']
    g = m.networkx_graph
    P = Predictor(m)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).cpu().numpy()
    known = [int(v) for v in np.nonzero(deg > 0)[0][3:43:4]]
    bare = [int(v) for v in range(1, g.max_id + 1) if deg[v] == 0][:1]
    seeds = [v - 1 for v in known[::-1]] + [10 ** 6, -3, g.max_id] + [b - 1 for b in bare] + [known[0] - 1]
    res = P.discover(seeds, top=None, **KW)
    return dict(P=P, m=m, g=g, seeds=seeds, known=known, res=res)


def _whole(ctx, **kw):
    """The walk sets of every item of the call, as discover samples them."""
    from subgnn_amd import ops, tape
    P, g = ctx['P'], ctx['g']
    seeds = torch.tensor(ctx['known'], dtype=torch.int32, device=g.device)
    args = dict(KW)
    args.update(kw)
    return ops.seeded_walk_sets(g, seeds, seed=P.freeze()['seed'], stream_id=tape.stream_id(tape.STREAM_DISCOVER, 'predict'), **args)


def test_candidates_are_ordinary_requests(ctx):
    from subgnn_amd import discover
    P, res, known = ctx['P'], ctx['res'], ctx['known']
    whole = _whole(ctx)
    keys, nodes, lens = whole.keys.cpu().numpy(), whole.nodes.cpu().numpy(), whole.lengths.cpu().numpy()
    n = len(known) * KW['per_seed']
    first = {}
    for q in range(n):
        first.setdefault(int(keys[q]), q)
    assert res['n_sampled'] == n and res['n_distinct'] == len(first) and 1 < len(first) <= n
    item = res['item'].tolist()
    assert sorted(item) == sorted(first.values())                      # every distinct set once, under its smallest item
    assert res['item'].dtype == res['seed'].dtype == res['keys'].dtype == res['target'].dtype == torch.int64
    assert res['keys'].tolist() == [int(keys[q]) for q in item] and res['steps'].tolist() == whole.steps[item].tolist()
    assert res['seed'].tolist() == [known[q // KW['per_seed']] - 1 for q in item]
    assert res['subgraphs'] == [(nodes[q, :lens[q]] - 1).tolist() for q in item]
    for q, s, sub in zip(item, res['seed'].tolist(), res['subgraphs']):
        assert s in sub and sub == sorted(set(sub)) and len(sub) <= KW['sizes'][q % 2]
    plain = P.predict(res['subgraphs'])
    assert plain['subgraphs'] == [[v + 1 for v in s] for s in res['subgraphs']]
    print('logits of %d candidates against predict: largest absolute difference %.3e'
          % (len(item), float((res['logits'] - plain['logits']).abs().max())))
    assert_close(res['logits'], plain['logits'].cpu().numpy(), 'candidate logits against predict')
    # the order: descending score, then ascending item
    score = res['score'].cpu().numpy()
    assert discover.rank_order(score, item).tolist() == list(range(len(item))) and not np.isnan(score).any()
    assert bool((np.diff(score) <= 0).all())


def test_scores_follow_from_the_logits(ctx):
    P, res, m = ctx['P'], ctx['res'], ctx['m']
    assert not m.multilabel
    z = res['logits'].double().cpu()
    K = z.shape[1]
    tgt = res['target'].cpu()
    assert torch.equal(tgt, z.argmax(-1)) and torch.equal(res['labels'].cpu(), tgt)
    p64 = torch.softmax(z, -1)
    rows = torch.arange(z.shape[0])
    assert torch.equal(res['score'].cpu(), res['logits'].cpu()[rows, tgt])             # one draw: the logit itself
    assert float((res['prob'].double().cpu() - p64[rows, tgt]).abs().max()) <= 1e-6     # a float32 softmax of the same logits
    assert bool((res['score_std'] == 0).all())
    # a given target
    other = (int(tgt[0]) + 1) % K
    res2 = P.discover(ctx['seeds'], target=other, top=None, **KW)
    back = {q: i for i, q in enumerate(res['item'].tolist())}
    at = [back[q] for q in res2['item'].tolist()]
    assert sorted(at) == list(range(len(back))) and res2['target'].tolist() == [other] * len(at)
    assert torch.equal(res2['logits'], res['logits'][at]) and torch.equal(res2['score'], res2['logits'][:, other])
    assert float((res2['prob'].double().cpu() - p64[at, other]).abs().max()) <= 1e-6
    assert torch.equal(res2['labels'], res['labels'][at])
    for bad in (K, -1, [0], 1.5, True):
        with pytest.raises(ValueError):
            P.discover(ctx['seeds'], target=bad, **KW)
    for kw in (dict(per_seed=0), dict(draws=0), dict(top=0), dict(top_per_seed=0), dict(batch_size=0), dict(max_variants=2.5),
               dict(sizes=(0,)), dict(sizes=(257,)), dict(restart=1.5), dict(max_steps=-1)):
        with pytest.raises(ValueError):
            P.discover(ctx['seeds'], **kw)
    with pytest.raises(ValueError):
        P.discover('every')


def test_draws(ctx):
    from subgnn_amd import ops
    P, res1 = ctx['P'], ctx['res']
    E = 3
    res = P.discover(ctx['seeds'], target=1, draws=E, top=None, **KW)
    whole = _whole(ctx)
    assert sorted(res['item'].tolist()) == sorted(res1['item'].tolist())
    # the distinct candidates in the order of their items -- the one chunk discover forwards -- at every draw
    by_item = torch.argsort(res['item'])
    item, keys = res['item'][by_item], res['keys'][by_item].contiguous()
    packed = ops.Ragged.from_padded(whole.nodes[item].long())
    sets = ops.Ragged(packed.ptr, packed.nodes, max_len=int(whole.lengths[item].max()))
    assert torch.equal(ops.set_keys(sets), keys)
    fwd = lambda d: P.forward_prepared(P.prepare_sets(sets, epoch_offset=d, want_lists=False, sub_keys=keys))[0].float()
    per_draw = torch.stack([fwd(d) for d in range(E)])
    z = per_draw[:, :, 1].contiguous()
    print('per-draw target logit: mean sample std %.3e' % float(z.std(0).mean()))
    assert torch.equal(res['logits'][by_item], per_draw.mean(0)) and torch.equal(res['score'][by_item], z.mean(0))
    assert torch.equal(res['score_std'][by_item], z.std(0, unbiased=True)) and bool((res['score_std'] > 0).any())
    assert torch.equal(res['prob'][by_item], torch.softmax(per_draw, -1)[:, :, 1].contiguous().mean(0))
    assert res['target'].tolist() == [1] * item.numel() and torch.equal(res['labels'], res['logits'].argmax(-1))
    # the same in float64 on the host
    z64 = z.double().cpu().numpy()
    assert np.allclose(res['score'][by_item].cpu().numpy(), z64.mean(0), rtol=1e-5, atol=1e-7)
    assert np.allclose(res['score_std'][by_item].cpu().numpy(), z64.std(0, ddof=1), rtol=1e-4, atol=1e-7)
    # draw 0 alone is the one-draw answer
    back = {q: i for i, q in enumerate(res1['item'].tolist())}
    assert torch.equal(per_draw[0], res1['logits'][[back[q] for q in item.tolist()]])


def test_a_set_sampled_twice_is_scored_once(ctx):
    P, known = ctx['P'], ctx['known']
    res = P.discover(ctx['seeds'], sizes=(1,), per_seed=5, top=None)
    assert res['n_sampled'] == 5 * len(known) and res['n_distinct'] == len(known)
    assert sorted(res['item'].tolist()) == [5 * i for i in range(len(known))]          # the first item of every seed
    assert sorted(s[0] + 1 for s in res['subgraphs']) == known and res['steps'].tolist() == [0] * len(known)
    assert res['seed'].tolist() == [s[0] for s in res['subgraphs']]


def test_chunks_of_three_items(ctx):
    P, whole = ctx['P'], ctx['res']
    calls, orig = [], P.prepare_sets

    def wrapped(sets, epoch_offset=0, want_lists=True, sub_keys=None):
        calls.append(sets.n)
        return orig(sets, epoch_offset=epoch_offset, want_lists=want_lists, sub_keys=sub_keys)
    P.prepare_sets = wrapped
    try:
        parts = P.discover(ctx['seeds'], top=None, max_variants=3, batch_size=2, **KW)
    finally:
        P.__dict__.pop('prepare_sets')
    assert all(1 <= c <= 3 for c in calls) and sum(calls) == whole['n_distinct'] and len(calls) >= whole['n_distinct'] // 3
    assert parts['n_sampled'] == whole['n_sampled'] and parts['n_distinct'] == whole['n_distinct']
    assert sorted(parts['item'].tolist()) == sorted(whole['item'].tolist())
    back = {q: i for i, q in enumerate(whole['item'].tolist())}
    at = [back[q] for q in parts['item'].tolist()]
    assert_close(parts['logits'], whole['logits'][at].cpu().numpy(), 'logits in chunks of 3')
    assert [whole['subgraphs'][i] for i in at] == parts['subgraphs'] and torch.equal(parts['keys'], whole['keys'][at])
    # the same ranking, unless two scores are within the rounding of another padded shape of each other
    if at != list(range(len(at))):
        s = whole['score'].cpu().numpy()
        moved = [i for i, a in enumerate(at) if a != i]
        assert all(abs(s[at[i]] - s[i]) <= 1e-4 * max(1.0, abs(s[i])) for i in moved), moved


def test_known_and_novel(ctx):
    from subgnn_amd import discover, ops
    P, m, res = ctx['P'], ctx['m'], ctx['res']
    known = discover.known_keys(P)
    assert known is discover.known_keys(P) and known.dtype == torch.int64 and bool((known[1:] > known[:-1]).all())
    own = P.request_sets([[v - 1 for v in m.train_sub_G[0]], [v - 1 for v in m.test_sub_G[-1]]])
    assert bool(torch.isin(ops.set_keys(own), known).all())
    assert known.numel() <= len(m.train_sub_G) + len(m.val_sub_G) + len(m.test_sub_G)
    assert torch.equal(res['known'], torch.isin(res['keys'], known)) and res['known'].dtype == torch.bool
    # two of the candidates declared known: they are flagged, and novel=True leaves exactly them out
    f = P.freeze()
    mine = res['keys'][[0, 5]]
    f['known_keys'] = torch.unique(torch.cat([known, mine]))
    try:
        flagged = P.discover(ctx['seeds'], top=None, **KW)
        fresh = P.discover(ctx['seeds'], top=None, novel=True, **KW)
    finally:
        f['known_keys'] = known
    expect = torch.isin(res['keys'], mine) | res['known']
    assert torch.equal(flagged['item'], res['item']) and torch.equal(flagged['known'], expect) and int(expect.sum()) >= 2
    assert not bool(fresh['known'].any()) and fresh['item'].tolist() == res['item'][~expect].tolist()
    assert fresh['n_distinct'] == res['n_distinct'] and fresh['subgraphs'] == [s for s, k in zip(res['subgraphs'], expect.tolist()) if not k]


def test_top_and_top_per_seed(ctx):
    from subgnn_amd import discover
    P, res = ctx['P'], ctx['res']
    item = res['item'].tolist()
    order = list(range(len(item)))
    seed_index = [q // KW['per_seed'] for q in item]
    for kw in (dict(top=5), dict(top=None, top_per_seed=1), dict(top=4, top_per_seed=2), dict(top=10 ** 6)):
        got = P.discover(ctx['seeds'], **dict(KW, **kw))
        want = discover.select(order, seed_index, kw['top'], kw.get('top_per_seed')).tolist()
        assert got['item'].tolist() == [item[i] for i in want], kw
        assert got['subgraphs'] == [res['subgraphs'][i] for i in want] and torch.equal(got['score'], res['score'][want])
    one = P.discover(ctx['seeds'], top=None, top_per_seed=1, **KW)
    assert sorted(one['seed'].tolist()) == [v - 1 for v in ctx['known']]               # the best candidate of every seed
    default = P.discover(ctx['seeds'], **KW)
    assert default['item'].tolist() == item[:100]


def test_unknown_seeds_are_dropped(ctx):
    P, g, res = ctx['P'], ctx['g'], ctx['res']
    again = P.discover([v - 1 for v in ctx['known']], top=None, **KW)
    assert torch.equal(again['item'], res['item']) and again['subgraphs'] == res['subgraphs'] and torch.equal(again['logits'], res['logits'])
    for seeds in ([], [10 ** 6, -3, g.max_id]):
        with pytest.raises(ValueError, match='no node of the graph'):
            P.discover(seeds)
    every = P.discover('all', sizes=(2,), per_seed=1, top=None)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).cpu().numpy()
    assert every['n_sampled'] == int((deg > 0).sum()) and len(set(every['seed'].tolist())) == every['n_distinct']


def test_the_models_own_splits_are_untouched(run, ctx):
    from subgnn_amd.predict import Predictor
    m, trainer = run['model'], run['trainer']
    trainer.test(m)
    before = dict(m.test_results)
    objs = _split_objects(m)
    was_training, sparse_mark = m.training, m.__dict__.get('_sparse_prepared')
    P = Predictor(m)
    P.discover(ctx['seeds'], draws=2, **KW)
    P.discover(ctx['seeds'][:4], max_variants=2, novel=True, top_per_seed=1, **KW)
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
    from subgnn_amd import config, discover
    from subgnn_amd.predict import Predictor
    root, results = run['root'], run['results']
    f, out = tmp_path / 'seeds.txt', tmp_path / 'found.txt'
    f.write_text(' '.join(str(v) for v in ctx['seeds'][:6]) + '\n' + '\n'.join(str(v) for v in ctx['seeds'][6:]) + '\n')
    config.PROJECT_ROOT = root
    P = Predictor.from_run(run['rc'], results)
    label = P.label_names[-1]
    cmd = [sys.executable, '-m', 'subgnn_amd.discover', '-config_path', str(run['cfg']), '-project_root', str(root),
           '-restoreModelPath', str(results), '-seeds', str(f), '-out', str(out), '-target', label, '-sizes', '3,6', '-per_seed', '4',
           '-draws', '2', '-top', '7', '-top_per_seed', '2', '-batch_size', '4', '-restart', '0.25', '-sample_seed', '11']
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = out.read_text().splitlines()
    res = P.discover(ctx['seeds'], target=P.label_names.index(label), draws=2, top=7, top_per_seed=2, batch_size=4, restart=0.25,
                     sample_seed=11, **KW)
    assert got[0] == discover.HEADER and got[1:] == discover.lines_of(P, res) and len(got) == 8
    cols = [l.split('\t') for l in got[1:]]
    assert [c[0] for c in cols] == [str(r) for r in range(7)] and all(c[1] in c[5].split('-') for c in cols)
    assert max(sum(c[1] == d[1] for d in cols) for c in cols) <= 2 and {c[7] for c in cols} <= {'0', '1'}

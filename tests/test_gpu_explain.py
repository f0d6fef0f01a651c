"""-m gpu: leave-one-out attribution (subgnn_amd/explain.py, Predictor.explain / prepare_sets / predict(draws=)) end to end.

  * variants: what is prepared for the variants built on the device is exactly what ``Predictor.prepare`` computes for the same
    node lists sent as an ordinary request (anchors, similarities, component ids); their logits within helpers.assert_close;
  * deltas: ``delta_logit``, ``delta_prob`` and the CLI's ``label_without`` follow from the base and variant logits; a one-node
    request has one invalid unit with NaN;
  * draws: draw 0 is ``predict``, bit for bit; mean and standard deviation are those of the per-draw values recomputed with
    ``prepare_sets(..., epoch_offset=d)``; the draws do differ;
  * kept components: in component mode the components a variant keeps have the parent's neighbourhood anchors, border anchors
    with their hop similarities and structure similarities, bit for bit, at every draw;
  * chunking (``max_variants=3``), no leak into the model's own splits, the CLI in a fresh child process.

Inputs: the two-epoch ``cc`` run of tests/test_gpu_predict.py (250 nodes, 24 subgraphs, the ``tiny`` hyper-parameters) and its
requests: a connected subgraph, a three-component one, a one-node one, a second connected one, six isolated nodes, twelve
connected nodes."""
import math
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


@pytest.fixture(scope='module')
def ctx(run):
    """The predictor of the run, the requests and, per unit mode, the variants as explicit node lists built from the mapped
    request in Python (dataset numbering) with their (request, unit rank)."""
    from subgnn_amd.predict import Predictor
    m = run['model']
    P = Predictor(m)
    A, B = _requests(m.networkx_graph)
    req = A + B
    st = P.prepare(req)
    cc = st.attrs['predict_cc_ids'].cpu().numpy()
    units = {'node': [[[v] for v in s] for s in st.subgraphs],
             'component': [[[int(v) for v in comp if v != 0] for comp in cc[r] if comp[0] != 0] for r in range(len(req))]}
    assert [len(u) for u in units['component']] == [1, 3, 1, 1, 6, 1] and [len(u) for u in units['node']] == [4, 4, 1, 3, 6, 12]
    lists = {}
    for mode, per_req in units.items():
        out = []
        for r, us in enumerate(per_req):
            for k, gone in enumerate(us):
                if len(us) >= 2:
                    out.append((r, k, [v - 1 for v in st.subgraphs[r] if v not in gone]))
        lists[mode] = out
    return dict(P=P, m=m, hp=m.hparams, req=req, subgraphs=st.subgraphs, units=units, lists=lists)


def _spy(P, hp):
    """Record (number of sets, epoch_offset, snapshot) of every ``prepare_sets`` call of ``P`` -> (calls, undo)."""
    calls, orig = [], P.prepare_sets

    def wrapped(sets, epoch_offset=0, want_lists=True, sub_keys=None):
        st = orig(sets, epoch_offset=epoch_offset, want_lists=want_lists, sub_keys=sub_keys)
        calls.append((sets.n, epoch_offset, _snapshot(st, hp)))
        return st
    P.prepare_sets = wrapped
    return calls, lambda: P.__dict__.pop('prepare_sets')


def _same_row(a, b, what):
    """One set's slice of two snapshots' tensors, equal up to the padding of their requests (PAD ids, zero similarities)."""
    assert a.dtype == b.dtype and a.dim() == b.dim(), what
    cut = tuple(slice(0, min(x, y)) for x, y in zip(a.shape, b.shape))
    if a.dim() == 2 and what.startswith('cc_ids'):
        assert int((a != 0).sum()) == int((a[cut] != 0).sum()) and int((b != 0).sum()) == int((b[cut] != 0).sum()), what
    elif a.dim() == 2:                                                # (C, A): whole components are cut
        cut = (cut[0], slice(None))
        assert a.shape[1] == b.shape[1] and not bool(a[cut[0].stop:].any()) and not bool(b[cut[0].stop:].any()), what
    assert torch.equal(a[cut], b[cut]), what


@pytest.mark.parametrize('mode', ['node', 'component'])
def test_variants_are_ordinary_requests(ctx, mode):
    from subgnn_amd import ops
    P, hp, req = ctx['P'], ctx['hp'], ctx['req']
    explicit = ctx['lists'][mode]
    sets = P.request_sets(req)
    occ = ops.occlusion_sets(sets, mode, ops.cc_labels(ctx['m'].networkx_graph, sets) if mode == 'component' else None)
    assert occ.parent.tolist() == [r for r, _k, _l in explicit] and occ.unit.tolist() == [k for _r, k, _l in explicit]
    assert occ.units.tolist() == [len(u) for u in ctx['units'][mode]]
    st_v = P.prepare_sets(occ.sets, sub_keys=occ.keys)
    got = _snapshot(st_v, hp)
    st_e = P.prepare([l for _r, _k, l in explicit])
    want = _snapshot(st_e, hp)
    assert st_v.subgraphs == st_e.subgraphs == [sorted(v + 1 for v in l) for _r, _k, l in explicit]
    assert torch.equal(st_v.keys['subgraphs'], st_e.keys['subgraphs']) and torch.equal(st_v.keys['components'], st_e.keys['components'])
    assert got.keys() == want.keys() and len(got) == 1 + 4 * hp['n_layers'] + 3 * hp['n_layers'] + 2
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    want_logits = P.forward_prepared(st_e)[0].float().cpu()
    # the same through explain: the units' rows, the invalid ones, the logits
    res = P.explain(req, unit=mode)
    ptr = res['ptr'].tolist()
    assert ptr == np.concatenate([[0], np.cumsum([len(u) for u in ctx['units'][mode]])]).tolist()
    rows = [ptr[r] + k for r, k, _l in explicit]
    valid = res['valid'].cpu()
    assert valid.sum() == len(rows) and bool(valid[rows].all())
    assert res['subgraphs'] == ctx['subgraphs']
    if mode == 'node':
        assert res['unit_nodes'].tolist() == [v for s in ctx['subgraphs'] for v in s]
    else:
        uptr, ids = (t.tolist() for t in res['unit_nodes'])
        assert [ids[uptr[i]:uptr[i + 1]] for i in range(len(uptr) - 1)] == [u for us in ctx['units'][mode] for u in us]
    vl = res['variant_logits'].cpu()
    print('variant logits, %s mode: largest absolute difference %.3e' % (mode, float((vl[rows] - want_logits).abs().max())))
    assert_close(vl[rows], want_logits, 'variant logits, %s mode' % mode)
    assert bool(torch.isnan(vl[~valid]).all()) and not bool(torch.isnan(vl[valid]).any())


@pytest.mark.parametrize('mode', ['node', 'component'])
def test_deltas_follow_from_the_logits(ctx, mode):
    from subgnn_amd import explain
    P, req = ctx['P'], ctx['req']
    res = P.explain(req, unit=mode)
    base, vl, tgt, ptr = res['logits'].cpu(), res['variant_logits'].cpu(), res['target'].cpu(), res['ptr'].tolist()
    valid = res['valid'].cpu()
    assert tgt.dtype == torch.int64 and torch.equal(tgt, base.argmax(-1))
    assert torch.equal(res['probabilities'], torch.softmax(res['logits'], -1))
    dl, ds, dp = res['delta_logit'].cpu(), res['delta_std'].cpu(), res['delta_prob'].cpu()
    pb, pv = torch.softmax(base, -1), torch.softmax(vl, -1)
    for r in range(len(req)):
        for u in range(ptr[r], ptr[r + 1]):
            t = int(tgt[r])
            if valid[u]:
                assert float(dl[u]) == float(base[r, t] - vl[u, t]) and float(ds[u]) == 0.0
                # two float32 softmax values of the same logits, each within a few units of 2^-24 of the host's
                assert abs(float(dp[u]) - float(pb[r, t] - pv[u, t])) <= 1e-6
            else:
                assert math.isnan(dl[u]) and math.isnan(ds[u]) and math.isnan(dp[u])
    # the one-node request: one unit, no variant
    assert ptr[3] - ptr[2] == 1 and not bool(valid[ptr[2]])
    assert bool((dl[valid] != 0).any())
    # a given target: an int, a sequence; values outside the classes and a wrong length are errors
    K = base.shape[1]
    other = [(int(t) + 1) % K for t in tgt]
    res2 = P.explain(req, unit=mode, target=other)
    assert res2['target'].tolist() == other and torch.equal(res2['variant_logits'].cpu()[valid], vl[valid])
    u = int(valid.nonzero()[0])
    r = max(i for i in range(len(req)) if ptr[i] <= u)
    assert float(res2['delta_logit'][u]) == float(base[r, other[r]] - vl[u, other[r]])
    assert P.explain(req, unit=mode, target=K - 1)['target'].tolist() == [K - 1] * len(req)
    for bad in (K, -1, [0] * (len(req) + 1), [0] * (len(req) - 1) + [K]):
        with pytest.raises(ValueError):
            P.explain(req, unit=mode, target=bad)
    with pytest.raises(ValueError):
        P.explain(req, unit='edge')
    # the lines: label_without is the label of the variant's logits, units by descending delta_logit, the invalid one last
    lines = [l.split('\t') for l in explain.lines_of(P, res)]
    assert len(lines) == ptr[-1]
    for r in range(len(req)):
        mine = [l for l in lines if int(l[0]) == r]
        order = explain.unit_order(dl[ptr[r]:ptr[r + 1]].tolist(), valid[ptr[r]:ptr[r + 1]].tolist())
        assert len(mine) == len(order)
        for l, k in zip(mine, order):
            u = ptr[r] + k
            members = [v - 1 for v in ctx['units'][mode][r][k]]
            assert l[1] == '-'.join(str(v) for v in members)
            assert l[5] == (P.names_of(vl[u].argmax())[0] if valid[u] else '')
            assert l[2] == '%.9g' % float(dl[u])
        got = [float(l[2]) for l in mine if l[5] != '']
        assert got == sorted(got, reverse=True)


def test_draws(ctx):
    from subgnn_amd import ops
    P, hp, req = ctx['P'], ctx['hp'], ctx['req']
    plain = P.predict(req)
    assert set(plain) == {'logits', 'probabilities', 'labels', 'subgraphs'} == set(P.predict(req, draws=1))
    res1 = P.explain(req, draws=1)
    for k in ('logits', 'probabilities', 'labels'):
        assert torch.equal(res1[k], plain[k]), k
    assert res1['subgraphs'] == plain['subgraphs'] and 'logits_mean' not in res1
    E = 3
    out = P.predict(req, draws=E)
    assert set(out) == set(plain) | {'logits_mean', 'logits_std', 'probabilities_mean'}
    for k in ('logits', 'probabilities', 'labels'):
        assert torch.equal(out[k], plain[k]), k
    sets = P.request_sets(req)
    snaps, per_draw = [], []
    for d in range(E):
        st = P.prepare_sets(sets, epoch_offset=d, want_lists=False)
        assert st.subgraphs is None
        snaps.append(_snapshot(st, hp))
        per_draw.append(P.forward_prepared(st)[0].float())
    per_draw = torch.stack(per_draw)
    assert torch.equal(per_draw[0], plain['logits'])
    assert torch.equal(out['logits_mean'], per_draw.mean(0)) and torch.equal(out['logits_std'], per_draw.std(0, unbiased=True))
    assert torch.equal(out['probabilities_mean'], torch.softmax(per_draw, -1).mean(0))
    # the draws differ in the request's own anchors and in nothing the model shares
    moved = [k for k in snaps[0] if not torch.equal(snaps[0][k], snaps[1][k])]
    assert any(k.startswith('anchors_') for k in moved), moved
    assert all(k.startswith(('anchors_', 'sim/N/out', 'sim/P/in')) for k in moved), moved
    assert bool((out['logits_std'] > 0).any())
    # explain over draws: the mean and the sample standard deviation of the per-draw difference, both terms at the same draw
    res = P.explain(req, unit='node', draws=E)
    for k in ('logits', 'logits_mean', 'logits_std', 'probabilities_mean'):
        assert torch.equal(res[k], out[k]), k
    assert torch.equal(res['target'], per_draw.mean(0).argmax(-1))
    occ = ops.occlusion_sets(sets, 'node')
    var = torch.stack([P.forward_prepared(P.prepare_sets(occ.sets, epoch_offset=d, want_lists=False))[0].float() for d in range(E)])
    parent, tgt = occ.parent.long(), res['target']
    row = res['ptr'][:-1][parent] + occ.unit.long()
    diff = (per_draw.gather(2, tgt.view(1, -1, 1).expand(E, -1, 1)).squeeze(2)[:, parent]
            - var.gather(2, tgt[parent].view(1, -1, 1).expand(E, -1, 1)).squeeze(2))
    print('per-draw delta_logit: mean |.| %.3e, mean sample std %.3e' % (float(diff.mean(0).abs().mean()), float(diff.std(0).mean())))
    assert torch.equal(res['delta_logit'][row], diff.mean(0)) and torch.equal(res['variant_logits'][row], var.mean(0))
    assert torch.equal(res['delta_std'][row], diff.std(0, unbiased=True))
    assert bool((res['delta_std'][row] > 0).any())


def test_kept_components_keep_their_draws(ctx):
    from subgnn_amd import ops
    P, hp, req = ctx['P'], ctx['hp'], ctx['req']
    sets = P.request_sets(req)
    occ = ops.occlusion_sets(sets, 'component', ops.cc_labels(ctx['m'].networkx_graph, sets))
    parent, gone = occ.parent.tolist(), occ.unit.tolist()
    assert sorted(set(parent)) == [1, 4] and len(parent) == 3 + 6
    checked = 0
    for d in range(3):
        base = _snapshot(P.prepare_sets(sets, epoch_offset=d, want_lists=False), hp)
        var = _snapshot(P.prepare_sets(occ.sets, epoch_offset=d, want_lists=False, sub_keys=occ.keys), hp)
        keys = [k for k in base if k.startswith(KEPT)]
        assert len(keys) == 3 * hp['n_layers'] + 2
        for v, (r, u) in enumerate(zip(parent, gone)):
            n_comp = len(ctx['units']['component'][r])
            kept = [c for c in range(n_comp) if c != u]
            for k in keys:
                assert torch.equal(var[k][v, :n_comp - 1], base[k][r, kept]), (d, v, k)
                checked += 1
            for j, c in enumerate(kept):
                a, b = var['cc_ids'][v, j], base['cc_ids'][r, c]
                assert a[a != 0].tolist() == b[b != 0].tolist() == ctx['units']['component'][r][c]
    assert checked == 3 * 9 * (3 * hp['n_layers'] + 2)


def test_chunks_of_three_variants(ctx):
    P, hp, req = ctx['P'], ctx['hp'], ctx['req']
    calls, undo = _spy(P, hp)
    try:
        whole = P.explain(req, unit='node')
        n_whole = len(calls)
        parts = P.explain(req, unit='node', max_variants=3, batch_size=2)
    finally:
        undo()
    V = int(whole['valid'].sum())
    assert n_whole == 2 and calls[1][0] == V                           # the base request, then every variant at once
    chunks = calls[n_whole + 1:]
    assert [c[0] for c in chunks] == [3] * (V // 3) + ([V % 3] if V % 3 else [])
    full, lo = calls[1][2], 0
    for n, _d, snap in chunks:
        assert snap.keys() == full.keys()
        for k in snap:
            for i in range(n):
                _same_row(snap[k][i], full[k][lo + i], '%s, variant %d' % (k, lo + i))
        lo += n
    assert torch.equal(parts['valid'], whole['valid']) and torch.equal(parts['ptr'], whole['ptr'])
    ok = whole['valid']
    assert_close(parts['variant_logits'][ok], whole['variant_logits'][ok].cpu().numpy(), 'variant logits in chunks of 3')
    assert_close(parts['logits'], whole['logits'].cpu().numpy(), 'base logits in batches of 2')
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            P.explain(req, max_variants=bad)
    with pytest.raises(ValueError):
        P.explain(req, draws=0)


def test_the_models_own_splits_are_untouched(run):
    from subgnn_amd.predict import Predictor
    m, trainer = run['model'], run['trainer']
    trainer.test(m)
    before = dict(m.test_results)
    objs = _split_objects(m)
    was_training, sparse_mark = m.training, m.__dict__.get('_sparse_prepared')
    P = Predictor(m)
    A, B = _requests(m.networkx_graph)
    P.explain(A, unit='node', draws=2)
    P.explain(B + A, unit='component', max_variants=2)
    after_objs = _split_objects(m)
    assert after_objs.keys() == objs.keys()
    for k, v in objs.items():
        assert after_objs[k] is v, k
    assert m.training == was_training and m.__dict__.get('_sparse_prepared') == sparse_mark
    trainer.test(m)
    assert set(m.test_results) == set(before)
    for k, v in before.items():
        assert float(m.test_results[k]) == float(v) or (np.isnan(float(v)) and np.isnan(float(m.test_results[k]))), k


def test_cli_in_a_child_process(run, tmp_path):
    from subgnn_amd import config, explain
    from subgnn_amd.predict import Predictor
    root, results = run['root'], run['results']
    A, B = _requests(run['model'].networkx_graph)
    req = A + B
    f, out = tmp_path / 'requests.txt', tmp_path / 'explained.txt'
    f.write_text(''.join('-'.join(str(v) for v in s) + '\n' for s in req))
    config.PROJECT_ROOT = root
    P = Predictor.from_run(run['rc'], results)
    label = P.label_names[-1]
    r = subprocess.run([sys.executable, '-m', 'subgnn_amd.explain', '-config_path', str(run['cfg']), '-project_root', str(root),
                        '-restoreModelPath', str(results), '-subgraphs', str(f), '-out', str(out), '-unit', 'component',
                        '-target', label, '-draws', '2', '-top', '2', '-batch_size', '4'], cwd=REPO,
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = out.read_text().splitlines()
    assert got[0] == explain.HEADER
    res = P.explain(req, unit='component', target=P.label_names.index(label), draws=2, batch_size=4)
    assert res['target'].tolist() == [len(P.label_names) - 1] * len(req)
    want = explain.lines_of(P, res, top=2)
    assert [l.split('\t')[0] for l in got[1:]] == ['0', '1', '1', '2', '3', '4', '4', '5']
    worst = 0.0
    for a, b in zip(got[1:], want):
        a, b = a.split('\t'), b.split('\t')
        worst = max([worst] + [abs(float(x) - float(y)) for x, y in zip(a[2:5], b[2:5]) if x != 'nan'])
    print('CLI against in-process deltas: largest absolute difference %.3e' % worst)
    assert got[1:] == want
    assert got[1].split('\t')[2:] == ['nan', 'nan', 'nan', '']           # one component: nothing to leave out

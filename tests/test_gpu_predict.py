"""-m gpu: prediction on subgraphs outside the dataset (subgnn_amd/predict.py) end to end.

  * content only: what ``Predictor.prepare`` draws and computes for a subgraph does not depend on where it stands in the request,
    on what else the request holds, or on the order of its node list -- anchors and similarities exactly, logits within the
    element-wise 1e-4 bound of helpers.assert_close (the same forward pass at other padded shapes);
  * values: the similarities are what the graph says for the drawn anchors (ops.bfs_min_hops_to_sets, ops.bfs_hops,
    SubGNN.compute_structure_patch_similarities) and the logits are the oracle forward's (oracle/float_half.py in float64) fed
    the request's anchors and similarities;
  * no leak: the model's own splits are the same objects afterwards and test the same;
  * driver: a run trained with -checkpoint_k 1, the CLI in a fresh child process, Predictor.from_run in this one.

Inputs: the ``tiny`` fixture (prepared, untrained) and a generated multi-component dataset of the size
tests/test_gpu_train_driver.py trains (trained for two epochs, once per module)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close, write_dataset_from_golden

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
SLOTS = ('N_I', 'N_B', 'S_I', 'S_B', 'P_I', 'P_B')

CONFIG = '''{
    "data": {"task": "ds"},
    "tb": {"tb_logging": false, "dir": "tensorboard", "name": "x"},
    "optuna": {"opt_n_trials": 1, "opt_n_cores": 1, "monitor_metric": "val_micro_f1", "opt_direction": "maximize",
               "sampler": "random", "pruning": false},
    "hyperparams_fix": %s,
    "hyperparams_optuna": {}
}'''


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """The generated COMPONENT dataset, trained for two epochs with one kept checkpoint -> dict(root, cfg, results, model,
    trainer, rc)."""
    from conftest import load_golden
    from subgnn_amd import config, train_config, prepare_dataset as pd, precompute_graph_metrics as pgm
    root = tmp_path_factory.mktemp('predict_run')
    out, info = pd.write_dataset(root / 'ds', 'cc', seed=9, embed_dim=16, n=250, n_subgraphs=24, n_subgraph_nodes=6)
    pgm.calculate_stats(out)
    fix = dict(load_golden('tiny').hp)
    fix.update({'max_epochs': 2, 'seed': 1, 'lin_dropout': 0.0, 'compute_similarities': True, 'node_embed_size': 16,
                'batch_size': 8, 'learning_rate': 5e-3, 'grad_clip': 1.0, 'n_layers': 2})
    cfg = root / 'config.json'
    cfg.write_text(CONFIG % json.dumps(fix))
    config.PROJECT_ROOT = root
    rc = train_config.read_json(cfg)
    best, model, trainer = train_config.train_model(rc, results_dir=root / 'results', checkpoint_k=1, log=lambda *a: None)
    yield dict(root=root, cfg=cfg, results=root / 'results', model=model, trainer=trainer, rc=rc)
    torch.cuda.empty_cache()


def _tiny_model(tiny, tmp_path):
    from test_gpu_model import _model
    m = _model(tiny, tmp_path)
    m.prepare_data()
    return m


# ---- requests built from the graph ------------------------------------------------------------------------------------------
def _requests(g):
    """(A, B) in the dataset's numbering (model id - 1).  A: a connected subgraph, one of three components (two single nodes
    and an adjacent pair), a one-node subgraph, a second connected one.  B: a subgraph of six pairwise non-adjacent nodes (more
    components than any of A) and a connected one of twelve nodes (a longer component than any of A)."""
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    nbr = {v: sorted({int(w) for w in col[rp[v]:rp[v + 1]]} - {v}) for v in range(1, g.max_id + 1)}
    nodes = [v for v in range(1, g.max_id + 1) if nbr[v]]

    def ball(v, n):
        seen, q = [v], [v]
        while q and len(seen) < n:
            u = q.pop(0)
            for w in nbr[u]:
                if w not in seen and len(seen) < n:
                    seen.append(w)
                    q.append(w)
        return seen

    def spread(k, start):
        """k nodes from ``start`` on, no two equal or adjacent."""
        got = []
        for v in nodes[start:] + nodes[:start]:
            if all(v != u and v not in nbr[u] for u in got):
                got.append(v)
            if len(got) == k:
                return got
        raise AssertionError('graph too dense for %d spread nodes' % k)

    a, b, c = spread(3, 5)
    pair = [c, next(w for w in nbr[c] if w not in (a, b) and w not in nbr[a] and w not in nbr[b])]
    big = max((ball(v, 12) for v in nodes[:40]), key=len)
    assert len(big) == 12
    A = [ball(nodes[3], 4), [a, b] + pair, [nodes[11]], ball(nodes[20], 3)]
    B = [spread(6, 17), big]
    back = lambda ls: [[v - 1 for v in s] for s in ls]
    return back(A), back(B)


def _dense(t):
    return t.dense() if hasattr(t, 'dense') else t


def _snapshot(st, hp):
    """Everything a prepared request holds, by name, as CPU tensors (anchors, similarities, component ids)."""
    out = {'cc_ids': st.attrs['predict_cc_ids']}
    for k, v in (st.attrs['predict_neigh_pos_similarities'] or {}).items():
        out['sim/%s/%s/%d' % k] = _dense(v)
    for k in ('anchors_neigh_int', 'anchors_neigh_border', 'anchors_pos_int'):
        for l, v in st.per_split.get(k, {}).items():
            out['%s/%d' % (k, l)] = v
    for k in ('int', 'bor'):
        v = st.attrs['predict_%s_struc_similarities' % k]
        if v is not None:
            out['S_sim/' + k] = v
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _rows(snap, rows, like):
    """``snap`` restricted to ``rows`` (in that order) and cut to the padded widths of ``like`` -- with what is cut away
    checked to be padding (PAD ids, zero similarities)."""
    out = {}
    for k, v in snap.items():
        v = v[torch.as_tensor(rows)]
        w = like[k]
        if k == 'cc_ids':
            cut = v[:, :w.shape[1], :w.shape[2]]
            assert int((v != 0).sum()) == int((cut != 0).sum())
        elif v.dim() == 3:                                          # (S, C, A): per component
            cut = v[:, :w.shape[1]]
            assert not bool(v[:, w.shape[1]:].any()), k
        else:
            cut = v
        out[k] = cut
    return out


def _check_content_only(P, hp):
    A, B = _requests(P.model.networkx_graph)
    nA = len(A)
    st = P.prepare(A)
    base = _snapshot(st, hp)
    logits = P.forward_prepared(st)[0].cpu()
    S, C, Lc = base['cc_ids'].shape
    n_comp = (base['cc_ids'][:, :, 0] != 0).sum(1).tolist()
    assert S == nA and n_comp == [1, 3, 1, 1] and base['cc_ids'][2].ne(0).sum() == 1     # single, multi, one node
    assert hp['use_neighborhood'] and hp['use_position'] and hp['use_structure']
    assert len(base) == 1 + 4 * hp['n_layers'] + 3 * hp['n_layers'] + 2

    rng = np.random.default_rng(2)
    shuffled = [[s[i] for i in rng.permutation(len(s))] for s in A]
    assert any(a != b for a, b in zip(A, shuffled))
    cases = {'A + B': (A + B, list(range(nA))), 'B + A': (B + A, list(range(len(B), len(B) + nA))),
             'reversed A': (A[::-1], list(range(nA))[::-1]), 'shuffled node lists': (shuffled, list(range(nA)))}
    worst = 0.0
    for name, (req, rows) in cases.items():
        st2 = P.prepare(req)
        snap = _snapshot(st2, hp)
        if 'B' in name:                                            # B widens both the padded C and the padded length
            assert snap['cc_ids'].shape[1] > C and snap['cc_ids'].shape[2] > Lc
        got = _rows(snap, rows, base)
        assert got.keys() == base.keys()
        for k in base:
            assert got[k].dtype == base[k].dtype and torch.equal(got[k], base[k]), '%s: %s' % (name, k)
        lg = P.forward_prepared(st2)[0].cpu()[torch.as_tensor(rows)]
        worst = max(worst, float((lg - logits).abs().max()))
        assert_close(lg, logits, 'logits, ' + name)
    print('content-only logits: largest absolute difference over the cases %.3e' % worst)
    return A, B


def test_content_only_tiny(tiny, tmp_path):
    from subgnn_amd.predict import Predictor
    m = _tiny_model(tiny, tmp_path)
    _check_content_only(Predictor(m), m.hparams)


def test_content_only_trained_run(run):
    from subgnn_amd.predict import Predictor
    _check_content_only(Predictor(run['model']), run['model'].hparams)


# ---- values -----------------------------------------------------------------------------------------------------------------
def _oracle_logits(m, st):
    """oracle/float_half.forward in float64 on the installed request."""
    from oracle import float_half as FH
    hp, Lr = m.hparams, m.hparams['n_layers']
    cpu = lambda t: t.detach().cpu()
    f64 = lambda t: cpu(t).double() if t.is_floating_point() else cpu(t)
    params = {k: f64(v) for k, v in m.state_dict().items()}
    anchors = {'N_int': {'predict': {l: cpu(m.anchors_neigh_int['predict'][l]) for l in range(Lr)}},
               'N_bor': {'predict': {l: cpu(m.anchors_neigh_border['predict'][l]) for l in range(Lr)}},
               'P_int': {'predict': {l: cpu(m.anchors_pos_int['predict'][l]) for l in range(Lr)}},
               'P_ext': {l: cpu(m.anchors_pos_ext[l]) for l in range(Lr)}, 'S': {}}
    for l in range(Lr):
        p, i, a, b = m.anchors_structure[l]
        anchors['S'][l] = (cpu(p), [int(v) for v in (i.tolist() if torch.is_tensor(i) else i)], cpu(a), cpu(b))
    cc = st.attrs['predict_cc_ids']
    ob = {'cc_ids': cpu(cc), 'subgraph_idx': torch.arange(cc.shape[0]).view(-1, 1),
          'NP_sim': {k: f64(_dense(v)) for k, v in st.attrs['predict_neigh_pos_similarities'].items()},
          'I_S_sim': f64(st.attrs['predict_int_struc_similarities']), 'B_S_sim': f64(st.attrs['predict_bor_struc_similarities'])}
    ccp = {nm: f64(getattr(m, 'predict_%s_cc_embed' % nm)) for nm in SLOTS} if hp['trainable_cc'] else None
    with torch.no_grad():
        return FH.forward(params, hp, 'predict', ob, anchors, ccp)


def test_similarities_and_logits_are_what_the_graph_and_the_oracle_say(run, tmp_path):
    from subgnn_amd import ops
    from subgnn_amd.predict import Predictor
    m = run['model']
    hp, g = m.hparams, m.networkx_graph
    P = Predictor(m)
    A, B = _requests(g)
    st = P.prepare(A + B)
    cc = st.attrs['predict_cc_ids']
    S, C, Lc = cc.shape
    sims = st.attrs['predict_neigh_pos_similarities']
    cc_sets = ops.Ragged.from_padded(cc.reshape(S * C, Lc))
    cap = hp.get('max_bfs_hops', 32)
    # the unique member nodes' hop tables, for the border check
    members = torch.unique(cc[cc != 0]).to(torch.int32).contiguous()
    table = ops.bfs_hops(g, members, max_hops=cap).cpu().numpy().astype(np.int64)            # (n_members, max_id + 1)
    row_of = {int(v): i for i, v in enumerate(members.tolist())}
    ccn = cc.cpu().numpy()
    for l in range(hp['n_layers']):
        # position, external: the frozen hop tables give what a search from the anchors gives
        want = ops.bfs_min_hops_to_sets(g, m.anchors_pos_ext[l].to(torch.int32).contiguous(), cc_sets, max_hops=cap)
        assert torch.equal(sims[('P', 'out', l)].reshape(S * C, -1), want)
        assert bool((want != 0).any())
        # neighbourhood, border: the similarity of a slot is the hop of its anchor from the component; PAD has 0
        an = m.anchors_neigh_border['predict'][l].cpu().numpy()
        w = sims[('N', 'out', l)].cpu().numpy()
        seen = set()
        for s in range(S):
            for c in range(C):
                rows = [row_of[int(v)] for v in ccn[s, c] if v != 0]
                for i, a in enumerate(an[s, c]):
                    if a == 0 or not rows:
                        assert w[s, c, i] == 0.0
                    else:
                        hop = int(table[rows, a].min())
                        assert 1 <= hop <= hp['neigh_sample_border_size'] and w[s, c, i] == float(hop), (l, s, c, i)
                        seen.add(hop)
        assert seen == set(range(1, hp['neigh_sample_border_size'] + 1))
        assert not bool(_dense(sims[('N', 'in', l)]).any())
    # structure: the model's own similarity routine on the request's padded component ids
    for internal, k in ((True, 'int'), (False, 'bor')):
        want = m.compute_structure_patch_similarities(None, tmp_path / (k + '.npy'), internal, cc)
        assert torch.equal(st.attrs['predict_%s_struc_similarities' % k], want)
    # logits and embeddings
    logits, emb = P.forward_prepared(st)
    ref = _oracle_logits(m, st)
    assert logits.shape == (S, m.num_classes) and emb.shape == (S, m.lin.in_features)
    assert_close(logits, ref, 'logits against the float64 oracle')
    # batch_size only chunks the forward pass
    lg3, emb3 = P.forward_prepared(st, batch_size=3)
    assert_close(lg3, logits.cpu().numpy(), 'logits in chunks of 3')
    assert_close(emb3, emb.cpu().numpy(), 'embeddings in chunks of 3')
    out = P.predict(A + B, batch_size=4, return_embeddings=True)
    assert set(out) == {'logits', 'probabilities', 'labels', 'subgraphs', 'embeddings'}
    assert torch.equal(out['labels'], out['logits'].argmax(-1)) and out['labels'].dtype == torch.int64
    assert torch.allclose(out['probabilities'].sum(-1), torch.ones(S, device=out['logits'].device), atol=1e-6)
    assert torch.equal(out['probabilities'], torch.softmax(out['logits'], -1))
    assert_close(out['logits'], logits.cpu().numpy(), 'predict() against forward_prepared()')
    assert 'embeddings' not in P.predict(A)


# ---- no leak ----------------------------------------------------------------------------------------------------------------
def _split_objects(m):
    out = {}
    for sp in ('train', 'val', 'test'):
        for nm in ('_cc_ids', '_N_border', '_neigh_pos_similarities', '_int_struc_similarities', '_bor_struc_similarities',
                   '_sub_G', '_sub_G_label'):
            out[sp + nm] = getattr(m, sp + nm, None)
        for nm in ('anchors_neigh_int', 'anchors_neigh_border', 'anchors_pos_int'):
            for l, t in getattr(m, nm)[sp].items():
                out['%s/%s/%d' % (nm, sp, l)] = t
    for l, t in m.anchors_pos_ext.items():
        out['anchors_pos_ext/%d' % l] = t
    for l, t in m.anchors_structure.items():
        out['anchors_structure/%d' % l] = t
    out['structure_anchors'] = m.structure_anchors
    return out


def test_the_models_own_splits_are_untouched(run):
    from subgnn_amd.predict import Predictor
    m, trainer = run['model'], run['trainer']
    trainer.test(m)
    before = dict(m.test_results)
    objs = _split_objects(m)
    was_training, sparse_mark = m.training, m.__dict__.get('_sparse_prepared')
    P = Predictor(m)
    A, B = _requests(m.networkx_graph)
    P.predict(A)
    P.predict(B + A, batch_size=2)
    after_objs = _split_objects(m)
    assert after_objs.keys() == objs.keys()
    for k, v in objs.items():
        assert after_objs[k] is v, k
    assert m.training == was_training and m.__dict__.get('_sparse_prepared') == sparse_mark
    trainer.test(m)
    assert set(m.test_results) == set(before)
    for k, v in before.items():
        assert float(m.test_results[k]) == float(v) or (np.isnan(float(v)) and np.isnan(float(m.test_results[k]))), k


# ---- driver -----------------------------------------------------------------------------------------------------------------
def test_cli_in_a_child_process_and_from_run(run, tmp_path):
    from subgnn_amd import config
    from subgnn_amd.predict import Predictor, read_requests
    from subgnn_amd.subgraph_utils import label_names
    root, results = run['root'], run['results']
    assert [n for n in os.listdir(results) if n.startswith('epoch') and n.endswith('.ckpt')]
    A, B = _requests(run['model'].networkx_graph)
    req = (A + B)[:5]
    n_graph = run['model'].networkx_graph.max_id
    req[1] = req[1] + [n_graph + 50]                                # an id outside the graph: dropped
    f = tmp_path / 'requests.txt'
    f.write_text(''.join('-'.join(str(v) for v in s) + ('\tignored\tcolumns\n' if i % 2 else '\n') for i, s in enumerate(req)))
    assert read_requests(f) == req
    out, emb = tmp_path / 'pred.txt', tmp_path / 'emb.npy'
    r = subprocess.run([sys.executable, '-m', 'subgnn_amd.predict', '-config_path', str(run['cfg']), '-project_root', str(root),
                        '-restoreModelPath', str(results), '-subgraphs', str(f), '-out', str(out), '-embeddings', str(emb),
                        '-batch_size', '2'], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = out.read_text().splitlines()
    assert len(lines) == 5
    names = label_names(root / 'ds' / 'subgraphs.pth')
    config.PROJECT_ROOT = root
    P = Predictor.from_run(run['rc'], results)
    assert P.restored_from.startswith('epoch') and P.label_names == names
    res = P.predict(req, batch_size=2, return_embeddings=True)
    prob = res['probabilities'].cpu().numpy()
    E = np.load(emb)
    assert E.shape == (5, P.model.lin.in_features) and E.dtype == np.float32
    worst = 0.0
    for i, line in enumerate(lines):
        nodes, label, ps = line.split('\t')
        want_nodes = sorted(v for v in req[i] if v < n_graph)              # the request as a set, without the foreign id
        assert [int(v) for v in nodes.split('-')] == want_nodes
        assert label in names and label == names[int(res['labels'][i])]
        got = np.asarray([float(p) for p in ps.split(',')], dtype=np.float32)
        assert got.shape == (P.model.num_classes,)
        worst = max(worst, float(np.abs(got - prob[i]).max()))
    print('CLI against in-process probabilities: largest absolute difference %.3e' % worst)
    for i, line in enumerate(lines):
        got = np.asarray([float(p) for p in line.split('\t')[2].split(',')], dtype=np.float32)
        assert np.array_equal(got, prob[i]), (i, got, prob[i])
    assert np.array_equal(E, res['embeddings'].cpu().numpy())
    assert res['subgraphs'][1] == sorted(v + 1 for v in req[1][:-1])
    # a list with nothing but ids outside the graph: an error naming its index
    with pytest.raises(ValueError, match='subgraph 2 '):
        P.predict([req[0], req[1], [n_graph + 7, n_graph + 8]])

"""-m gpu: k-means (csrc/kmeans.hip through the raw ABI and ops.kmeans_step / ops.kmeans) and the clustering of an index
(subgnn_amd/cluster.py) end to end.

  * a step on the dyadic grids: assign and score bit for bit ops.topk_rows(k = 1) with the same aux vectors, both metrics; sums,
    counts, inertia, changed, centres and empty bit for bit tests/kmeans_cases.step_ref; at every edge of N, K, D and the slots;
  * the order (duplicate centres, duplicate rows, a centre that wins nothing), prev_assign, fixed point and repeatability;
  * strided X; guard words around every output in every call of ``_step``; refusals write nothing;
  * random inputs: assign again topk_rows' bits, sums within the derived bound of the float64 sums (kmeans_cases.sums_tolerance);
  * whole fits on Gaussian blobs: the labels of the float64 reference run at every iteration, n_iter, centres within the bound;
  * the clustering of a trained run's index, its file and the CLI.

Every call of ``_step`` goes through the raw ABI into guarded buffers AND through ops.kmeans_step, and the two must agree."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kmeans_cases as KC
import neighbors_cases as NC

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
GUARD = 64                                   # words on either side of an output
FILL = {torch.float32: -12345.5, torch.int32: -0x5A5A5A5A, torch.float64: -54321.25}
OUTPUTS = (('assign', torch.int32, 'N'), ('score', torch.float32, 'N'), ('sums', torch.float32, 'KD'), ('counts', torch.int32, 'K'),
           ('inertia', torch.float64, '1'), ('empty', torch.int32, '1'), ('centers', torch.float32, 'KD'),
           ('c_aux', torch.float32, 'K'), ('changed', torch.int32, '1'))


def _t(a):
    return a if isinstance(a, torch.Tensor) or a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(N, K, D):
    n = {'N': N, 'K': K, 'KD': K * D, '1': 1}
    return {name: torch.full((max(n[size], 0) + 2 * GUARD,), FILL[dt], dtype=dt, device=DEV) for name, dt, size in OUTPUTS}


def _untouched(bufs):
    return all(bool((b == FILL[b.dtype]).all()) for b in bufs.values())


def _raw(X, C, metric, x_aux, c_aux, prev, K=None, code=None, ws_short=0, finish=True):
    """sgnn_kmeans_step + sgnn_kmeans_finish into guarded buffers -> (rc of the step, rc of the finish, buffers)."""
    from subgnn_amd import _lib, ops
    lib = _lib.load()
    N, D = X.shape
    K = C.shape[0] if K is None else K
    bufs = _guarded(N, max(K, 0), D)
    nbytes = max(0, int(lib.sgnn_kmeans_workspace_bytes(N, min(max(K, 1), KC.MAX_K), D)))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)
    o = lambda name: p(bufs[name], GUARD * bufs[name].element_size())
    xs, cs = X.stride(0) if N > 1 else max(D, X.stride(0)), C.stride(0) if C.shape[0] > 1 else max(D, C.stride(0))
    code = NC.METRIC_CODE[metric] if code is None else code
    rc1 = lib.sgnn_kmeans_step(p(X), xs, N, p(C), cs, K, D, code, p(x_aux), p(c_aux), p(prev), o('assign'), o('score'), p(ws),
                               nbytes - ws_short, ops._stream())
    rc2 = lib.sgnn_kmeans_finish(p(ws), nbytes - ws_short, N, K, D, code, p(C), cs, o('sums'), o('counts'), o('inertia'),
                                 o('empty'), o('centers'), o('c_aux'), o('changed'), 0, ops._stream()) if finish else None
    torch.cuda.synchronize()
    return rc1, rc2, bufs


def _step(X, C, metric, prev=None, x_aux=None, c_aux=None):
    """dict of numpy arrays through both entries; guards checked; assign and score checked against topk_rows(k = 1)."""
    from subgnn_amd import ops
    X, C, prev = _t(X), _t(C), _t(prev)
    (N, D), K = X.shape, C.shape[0]
    xa = ops.topk_aux(X, metric) if x_aux is None else _t(x_aux)
    ca = ops.topk_aux(C, metric) if c_aux is None else _t(c_aux)
    rc1, rc2, bufs = _raw(X, C, metric, xa, ca, prev)
    assert (rc1, rc2) == (0, 0)
    n = {'N': N, 'K': K, 'KD': K * D, '1': 1}
    out = {}
    for name, dt, size in OUTPUTS:
        b = bufs[name]
        assert bool((b[:GUARD] == FILL[dt]).all()) and bool((b[GUARD + n[size]:] == FILL[dt]).all()), 'guard of %s overwritten' % name
        out[name] = b[GUARD:GUARD + n[size]]
    res = ops.kmeans_step(X, C, metric, x_aux=xa, c_aux=ca, prev_assign=prev)
    assert set(res) == {name for name, _, _ in OUTPUTS}
    for name, dt, size in OUTPUTS:
        assert res[name].dtype == dt, name
        a, b = out[name].view(torch.int32 if dt != torch.float64 else torch.int64), res[name].reshape(-1)
        assert torch.equal(a, b.view(a.dtype)), '%s differs between the ABI and ops' % name
    s, i = ops.topk_rows(X, C, 1, metric, q_aux=xa, b_aux=ca)
    assert torch.equal(out['assign'].long(), i[:, 0]), 'assign is not topk_rows(k = 1)'
    assert torch.equal(out['score'].view(torch.int32), s[:, 0].contiguous().view(torch.int32)), 'score bits are not topk_rows(k = 1)'
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out['sums'], out['centers'] = out['sums'].reshape(K, D), out['centers'].reshape(K, D)
    return out


def _check_against_reference(got, X, C, prev, what):
    N, D = X.shape
    want = KC.step_ref(X, C, got['assign'], got['score'], prev, KC.slot_rows(N, C.shape[0], D))
    for name in ('sums', 'centers'):
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), '%s: %s bits differ at %s' % (
            what, name, np.argwhere(got[name].view(np.uint32) != want[name].view(np.uint32))[:5].tolist())
    assert np.array_equal(got['counts'], want['counts']), what
    assert int(got['empty'][0]) == want['empty'] and int(got['changed'][0]) == want['changed'], what
    return want


# ---- bit for bit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', KC.exact_cases(), ids=KC.case_id)
def test_dyadic_grids_bit_for_bit(case):
    X, C, prev = KC.make_inputs(case)
    for metric in ('l2', 'cosine'):
        got = _step(X, C, metric, prev)
        want = _check_against_reference(got, X, C, prev, '%s %s' % (KC.case_id(case), metric))
        if metric == 'l2':                                           # the scores are exact too: so is their float64 sum
            assert float(got['inertia'][0]) == want['inertia']
            if case['N'] * case['K'] * case['D'] <= 10 ** 7:
                a, s = KC.assign_ref(X, C, 'l2')
                assert np.array_equal(got['assign'], a) and np.array_equal(got['score'].view(np.uint32), s.view(np.uint32))
        else:
            assert abs(float(got['inertia'][0]) - want['inertia']) <= KC.gamma(case['N']) * np.abs(got['score'].astype(np.float64)).sum()
        c64 = got['centers'].astype(np.float64)
        sq = (c64 * c64).sum(1)
        aux = sq if metric == 'l2' else 1.0 / np.sqrt(np.maximum(sq, 1e-30))
        assert np.all(np.abs(got['c_aux'] - aux) <= KC.aux_tolerance(case['D']) * np.abs(aux) + 1e-45), 'c_aux'


# ---- order --------------------------------------------------------------------------------------------------------------------
def test_duplicate_centres_duplicate_rows_and_a_centre_that_wins_nothing():
    rng = np.random.default_rng(21)
    base = NC.dyadic(rng, 5, 9)
    C = np.concatenate([base, base[[2, 0]], np.full((1, 9), 8.0, dtype=np.float32)])     # 5, 6 duplicate 2, 0; 7 is far away
    C[7, 0] = np.float32(1) + np.float32(2.0 ** -23)                                     # bits a recomputation would not give
    rows = NC.dyadic(rng, 40, 9)
    X = np.concatenate([rows, rows[::-1], base])                                         # every row twice; the centres themselves
    for metric in ('l2', 'cosine'):
        got = _step(X, C, metric)
        a = got['assign']
        assert a.max() <= 4 or metric == 'cosine' and set(a.tolist()) <= {0, 1, 2, 3, 4, 7}
        assert not np.isin(a, [5, 6]).any()                                              # the smaller index of a duplicate pair
        assert np.array_equal(a[:40], a[40:80][::-1])                                    # duplicate rows, the same cluster
        if metric == 'l2':
            assert a[80:].tolist() == [0, 1, 2, 3, 4] and np.all(got['score'][80:] == 0)
            assert got['counts'][7] == 0 and got['counts'][5] == got['counts'][6] == 0 and int(got['empty'][0]) == 3
            for k in (5, 6, 7):
                assert np.array_equal(got['centers'][k].view(np.uint32), C[k].view(np.uint32))    # kept bit for bit
                assert np.all(got['sums'][k] == 0)
        _check_against_reference(got, X, C, None, metric)


# ---- prev_assign, fixed point, repeatability ------------------------------------------------------------------------------------
def test_changed_counts_exactly_the_differing_rows():
    X, C, _ = KC.make_inputs(dict(N=1000, K=7, D=9, prev=False))
    first = _step(X, C, 'l2')
    assert int(first['changed'][0]) == 1000                          # null: N
    prev = first['assign'].copy()
    assert int(_step(X, C, 'l2', prev)['changed'][0]) == 0
    flip = [0, 31, 32, 500, 991, 999]                                # across tiles and slots, the ragged last one included
    prev[flip] = (prev[flip] + 1) % 7
    assert int(_step(X, C, 'l2', prev)['changed'][0]) == len(flip)
    assert int(_step(X, C, 'l2', np.full(1000, -1, dtype=np.int32))['changed'][0]) == 1000


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_a_step_fed_its_own_assignment_is_a_fixed_point_and_calls_repeat(metric):
    X = KC.blobs(metric)
    C0 = X[KC.init_rows(X, 6, 'random', 1)].copy()
    a = _step(X, C0, metric)
    b = _step(X, C0, metric)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name      # two calls, identical bits
    # iterate to convergence by hand, then once more: the centres' bits must not move
    C, aux, prev = a['centers'], a['c_aux'], a['assign']
    for _ in range(60):
        r = _step(X, C, metric, prev, c_aux=aux)
        if int(r['changed'][0]) == 0:
            break
        C, aux, prev = r['centers'], r['c_aux'], r['assign']
    assert int(r['changed'][0]) == 0
    assert np.array_equal(r['centers'].view(np.uint32), C.view(np.uint32)) and np.array_equal(r['c_aux'].view(np.uint32), aux.view(np.uint32))
    again = _step(X, r['centers'], metric, r['assign'], c_aux=r['c_aux'])
    for name in again:
        assert np.array_equal(again[name].view(np.uint8), r[name].view(np.uint8)), name


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_kmeans_does_not_depend_on_check_every(metric):
    from subgnn_amd import ops
    X = torch.from_numpy(KC.blobs(metric)).to(DEV)
    a = ops.kmeans(X, 5, metric=metric, check_every=1, seed=3)
    b = ops.kmeans(X, 5, metric=metric, check_every=8, seed=3)
    assert a['converged'] and a['n_iter'] == b['n_iter'] and a['inertia'] == b['inertia'] and a['empty'] == b['empty'] == 0
    for name in ('centers', 'assign', 'score', 'sizes', 'c_aux'):
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name
    assert int(a['sizes'].sum()) == X.shape[0] and a['assign'].dtype == torch.int32
    assert a['n_iter'] >= 2                                          # the first iteration changes every row
    c = ops.kmeans(X, 5, metric=metric, max_iter=a['n_iter'] - 1, seed=3)
    assert not c['converged'] and c['n_iter'] == a['n_iter'] - 1
    best = ops.kmeans(X, 5, metric=metric, n_init=3, seed=3, init='random')
    runs = [ops.kmeans(X, 5, metric=metric, seed=3 + r, init='random')['inertia'] for r in range(3)]
    assert best['inertia'] == (max(runs) if metric == 'cosine' else min(runs))
    given = ops.kmeans(X, 5, metric=metric, init=a['centers'])
    assert torch.equal(given['assign'], a['assign'])


def test_initialisation_is_the_numpy_restatement():
    from subgnn_amd import ops
    X = KC.blobs('l2')
    Xd = torch.from_numpy(X).to(DEV)
    for seed in (0, 4):
        assert ops.kmeans_init_rows(Xd, 6, 'k-means++', seed) == KC.init_rows(X, 6, 'k-means++', seed)
        assert ops.kmeans_init_rows(Xd, 6, 'random', seed) == KC.init_rows(X, 6, 'random', seed)
    ones = torch.ones(5, 2, device=DEV)
    assert ops.kmeans_init_rows(ones, 4, 'k-means++', 3) == KC.init_rows(np.ones((5, 2), dtype=np.float32), 4, 'k-means++', 3)


# ---- strides and safety -------------------------------------------------------------------------------------------------------
def test_a_column_slice_of_a_wider_matrix_is_accepted():
    rng = np.random.default_rng(4)
    wide = torch.from_numpy(NC.dyadic(rng, 70, 40)).to(DEV)
    X = wide[:, 3:12]
    assert X.stride() == (40, 1) and not X.is_contiguous()
    C = NC.dyadic(rng, 5, 9)
    for metric in ('l2', 'cosine'):
        got = _step(X, C, metric)
        _check_against_reference(got, X.cpu().numpy(), C, None, metric)
    wc = torch.from_numpy(NC.dyadic(rng, 5, 33)).to(DEV)
    got = _step(X, wc[:, 20:29], 'l2')
    _check_against_reference(got, X.cpu().numpy(), wc[:, 20:29].cpu().numpy(), None, 'centre slice')


def test_refused_calls_write_nothing():
    from subgnn_amd import ops
    X, C = torch.ones(40, 6, device=DEV), torch.ones(3, 6, device=DEV)
    xa, ca = torch.ones(40, device=DEV), torch.ones(3, device=DEV)
    big = torch.ones(1025, 6, device=DEV)
    for kw in (dict(code=0), dict(code=7), dict(K=0), dict(ws_short=1)):
        rc1, rc2, bufs = _raw(X, C, 'l2', xa, ca, None, **kw)
        assert (rc1, rc2) == (-1, -1) and _untouched(bufs), kw
    rc1, rc2, bufs = _raw(X, big, 'l2', xa, torch.ones(1025, device=DEV), None)           # K above the limit
    assert (rc1, rc2) == (-1, -1) and _untouched(bufs)
    rc1, rc2, bufs = _raw(X, C, 'l2', None, ca, None, finish=False)                      # a missing aux vector
    assert rc1 == -1 and _untouched(bufs)
    with pytest.raises(ValueError):
        ops.kmeans_step(X, C, 'dot')
    with pytest.raises(ValueError, match='1024'):
        ops.kmeans_step(X, big, 'l2')
    with pytest.raises(ValueError):
        ops.kmeans_step(X, C[:, :5], 'l2')
    with pytest.raises(ValueError):
        ops.kmeans_step(X, C[:0], 'l2')
    with pytest.raises(ValueError, match='n_clusters'):
        ops.kmeans(X, 41)                                            # K > N
    with pytest.raises(ValueError):
        ops.kmeans(X, 0)
    bad = X.clone()
    bad[7, 2] = float('nan')
    with pytest.raises(ValueError, match='NaN'):
        ops.kmeans(bad, 2)
    bad[7, 2] = float('inf')
    with pytest.raises(ValueError):
        ops.kmeans(bad, 2, metric='cosine')


# ---- random inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_random_inputs_within_the_derived_bound(metric):
    X, C = KC.random_inputs()
    N, D = X.shape
    K = C.shape[0]
    got = _step(X, C, metric)                                        # (assign and score are topk_rows' bits: checked there)
    S = KC.geometry(N, K, D)[2]
    s64, tol = KC.sums_f64(X, got['assign'], K), KC.sums_tolerance(X, got['assign'], K, S)
    err = np.abs(got['sums'].astype(np.float64) - s64)
    print('%s: largest sums error / bound %.3f' % (metric, float((err / np.maximum(tol, 1e-300)).max())))
    assert np.all(err <= tol)
    assert np.array_equal(got['counts'], np.bincount(got['assign'], minlength=K)) and got['counts'].sum() == N
    want = KC.step_ref(X, C, got['assign'], got['score'], None, KC.slot_rows(N, K, D))
    for name in ('sums', 'centers'):                                 # and the stated order of the additions, literally
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name
    assert abs(float(got['inertia'][0]) - want['inertia']) <= KC.gamma(N) * np.abs(got['score'].astype(np.float64)).sum()
    score64 = NC.scores_f64(X, C, metric)[np.arange(N), got['assign']]
    assert np.all(np.abs(got['score'] - score64) <= NC.tolerance(X, C, metric)[np.arange(N), got['assign']])


# ---- whole fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_whole_fit_equals_the_float64_reference_run(metric):
    from subgnn_amd import ops
    f = KC.FIT
    X0 = torch.from_numpy(KC.blobs(metric)).to(DEV)
    Xd = ops.kmeans_unit_rows(X0) if metric == 'cosine' else X0      # the rows the kernel runs on
    X = Xd.cpu().numpy()
    rows = KC.init_rows(X, f['K'], 'k-means++', 0)
    assert ops.kmeans_init_rows(Xd, f['K'], 'k-means++', 0) == rows
    S = KC.geometry(f['N'], f['K'], f['D'])[2]
    ref = KC.lloyd_f64(X, rows, metric, f['max_iter'], S)
    assert ref['n_iter'] is not None and ref['no_empty'] and ref['min_margin'] >= 1.0    # the host test's condition, on these rows
    C, aux, prev = Xd[rows].contiguous(), None, None
    for it in range(ref['n_iter']):                                  # every iteration's end state
        r = ops.kmeans_step(Xd, C, metric, c_aux=aux, prev_assign=prev)
        assert np.array_equal(r['assign'].cpu().numpy(), ref['labels'][it]), 'labels differ at iteration %d' % (it + 1)
        tolC = KC.centers_tolerance(X, ref['labels'][it], f['K'], S, ref['centers'][it])
        err = np.abs(r['centers'].cpu().numpy().astype(np.float64) - ref['centers'][it])
        assert np.all(err <= tolC), (it, float((err / tolC).max()))
        C, aux, prev = r['centers'], r['c_aux'], r['assign']
    assert int(r['changed'].item()) == 0
    fit = ops.kmeans(X0, f['K'], metric=metric, seed=0, max_iter=f['max_iter'])
    assert fit['n_iter'] == ref['n_iter'] and fit['converged'] and fit['empty'] == 0
    assert np.array_equal(fit['assign'].cpu().numpy(), ref['labels'][-1])
    assert torch.equal(fit['centers'].view(torch.int32), r['centers'].view(torch.int32))
    assert np.array_equal(fit['sizes'].cpu().numpy(), np.bincount(ref['labels'][-1], minlength=f['K']))
    print('%s: %d iterations, largest centre error / bound %.3f' % (metric, fit['n_iter'], float((err / tolC).max())))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
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
    """The recipe of tests/test_gpu_neighbors.py's ``run``: the generated 24-subgraph COMPONENT dataset, two epochs, one kept
    checkpoint; then the predictor of the finished run, the index of its three splits and its clustering into 3."""
    from conftest import load_golden
    from subgnn_amd import config, train_config, prepare_dataset as pd, precompute_graph_metrics as pgm
    from subgnn_amd.neighbors import SubgraphIndex
    from subgnn_amd.predict import Predictor
    root = tmp_path_factory.mktemp('cluster_run')
    out, info = pd.write_dataset(root / 'ds', 'cc', seed=9, embed_dim=16, n=250, n_subgraphs=24, n_subgraph_nodes=6)
    pgm.calculate_stats(out)
    fix = dict(load_golden('tiny').hp)
    fix.update({'max_epochs': 2, 'seed': 1, 'lin_dropout': 0.0, 'compute_similarities': True, 'node_embed_size': 16,
                'batch_size': 8, 'learning_rate': 5e-3, 'grad_clip': 1.0, 'n_layers': 2})
    cfg = root / 'config.json'
    cfg.write_text(CONFIG % json.dumps(fix))
    config.PROJECT_ROOT = root
    rc = train_config.read_json(cfg)
    train_config.train_model(rc, results_dir=root / 'results', checkpoint_k=1, log=lambda *a: None)
    P = Predictor.from_run(rc, root / 'results')
    before = _split_objects(P.model)
    index = SubgraphIndex.from_predictor(P)
    cl = index.cluster(3)
    yield dict(root=root, cfg=cfg, results=root / 'results', rc=rc, P=P, index=index, before=before, cl=cl)
    torch.cuda.empty_cache()


def _split_objects(m):
    out = {}
    for sp in ('train', 'val', 'test'):
        for nm in ('_cc_ids', '_N_border', '_neigh_pos_similarities', '_int_struc_similarities', '_bor_struc_similarities',
                   '_sub_G', '_sub_G_label'):
            out[sp + nm] = getattr(m, sp + nm, None)
        for nm in ('anchors_neigh_int', 'anchors_neigh_border', 'anchors_pos_int'):
            for l, t in getattr(m, nm)[sp].items():
                out['%s/%s/%d' % (nm, sp, l)] = t
    return out


def test_clustering_of_a_run_labels_every_row(run):
    from subgnn_amd.cluster import label_figures, medoid_rows
    index, cl = run['index'], run['cl']
    n = len(index)
    assert n == 24 and cl.metric == index.metric == 'cosine' and cl.n_clusters == 3
    labels = cl.labels.cpu().numpy()
    assert cl.labels.dtype == torch.int64 and labels.shape == (n,) and labels.min() >= 0 and labels.max() < 3
    assert int(cl.sizes.sum()) == n and np.array_equal(cl.sizes.cpu().numpy(), np.bincount(labels, minlength=3))
    assert cl.centers.shape == (3, index.width) and cl.scores.shape == (n,) and cl.n_iter >= 2 and cl.converged
    scores = cl.scores.cpu().numpy()
    for k in range(3):                                               # medoids: members, best score first, then the smaller row
        members = [r for r in range(n) if labels[r] == k]
        want = sorted(members, key=lambda r: (-float(scores[r]), r))[:5]
        assert cl.medoids[k] == want and set(want) <= set(members)
    assert cl.medoids == medoid_rows(labels, scores, 3, 'cosine', 5)
    counts, pur, mi = label_figures(labels, index.labels, 3)
    assert cl.label_counts == counts and cl.purity == pur and cl.nmi == mi and 0 < pur <= 1 and 0 <= mi <= 1 + 1e-12
    assert sum(sum(c.values()) for c in counts) == sum(len(l) for l in index.labels)
    again = index.cluster(3)
    assert torch.equal(again.labels, cl.labels) and torch.equal(again.centers.view(torch.int32), cl.centers.view(torch.int32))
    l2 = index.cluster(2, metric='l2', medoids=1, init='random', seed=2)
    assert l2.metric == 'l2' and int(l2.sizes.sum()) == n and all(len(m) <= 1 for m in l2.medoids)


def test_assigning_the_index_rows_reproduces_the_labels_and_files_round_trip(run, tmp_path):
    from subgnn_amd.cluster import Clustering
    index, cl = run['index'], run['cl']
    k, s = cl.assign(index.embeddings)
    assert torch.equal(k, cl.labels) and torch.equal(s.view(torch.int32), cl.scores.view(torch.int32))
    f = tmp_path / 'clusters.npz'
    cl.save(f)
    assert os.listdir(tmp_path) == ['clusters.npz']
    again = Clustering.load(f, DEV)
    assert torch.equal(again.labels, cl.labels) and torch.equal(again.centers.view(torch.int32), cl.centers.view(torch.int32))
    assert again.medoids == cl.medoids and again.label_counts == cl.label_counts and again.majority == cl.majority
    assert (again.inertia, again.n_iter, again.converged, again.purity, again.nmi) == (cl.inertia, cl.n_iter, cl.converged, cl.purity, cl.nmi)
    k2, s2 = again.assign(index.embeddings[:7])
    assert torch.equal(k2, cl.labels[:7])


def test_clustering_leaves_the_models_splits_untouched(run):
    run['index'].cluster(2)
    after = _split_objects(run['P'].model)
    assert after.keys() == run['before'].keys()
    for k, v in run['before'].items():
        assert after[k] is v, k


def test_cli_in_a_child_process(run, tmp_path):
    index, cl = run['index'], run['cl']
    req = [list(s) for s in index.subgraphs[2:5]]
    f = tmp_path / 'requests.txt'
    f.write_text(''.join('-'.join(str(v) for v in s) + '\n' for s in req))
    out, npz, summ = tmp_path / 'clusters.txt', tmp_path / 'index.npz', tmp_path / 'summary.json'
    r = subprocess.run([sys.executable, '-m', 'subgnn_amd.cluster', '-config_path', str(run['cfg']), '-project_root', str(run['root']),
                        '-restoreModelPath', str(run['results']), '-n_clusters', '3', '-out', str(out), '-summary', str(summ),
                        '-index', str(npz), '-subgraphs', str(f)], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert npz.exists()
    lines = out.read_text().splitlines()
    n = len(index)
    assert lines[0].split('\t') == ['split', 'row', 'cluster', 'score', 'nodes', 'labels'] and len(lines) == 1 + n + len(req)
    labels, scores = cl.labels.cpu().numpy(), cl.scores.cpu().numpy()
    for j, line in enumerate(lines[1:1 + n]):
        cols = line.split('\t')
        sp, row, nodes, ls = index.describe(j)
        assert len(cols) == 6 and cols[0] == sp and int(cols[1]) == row and int(cols[2]) == labels[j]
        assert np.float32(float(cols[3])).view(np.uint32) == scores[j].view(np.uint32)
        assert [int(v) for v in cols[4].split('-')] == nodes and cols[5].split('-') == ls
    for i, line in enumerate(lines[1 + n:]):                         # the requests are dataset subgraphs: their rows' clusters
        cols = line.split('\t')
        assert cols[0] == 'request' and int(cols[1]) == i and int(cols[2]) == labels[2 + i] and cols[5] == ''
        assert [int(v) for v in cols[4].split('-')] == req[i]
    s = json.loads(summ.read_text())
    assert s['n_clusters'] == 3 and [c['size'] for c in s['clusters']] == cl.sizes.tolist() and s['arguments']['n_clusters'] == 3
    assert [c['medoids'] for c in s['clusters']] == cl.medoids and [c['label_counts'] for c in s['clusters']] == cl.label_counts
    assert s['purity'] == cl.purity and s['nmi'] == cl.nmi and s['n_iter'] == cl.n_iter

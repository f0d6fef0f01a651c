"""-m gpu: the nearest-row search (csrc/neighbors.hip through the raw ABI and ops.topk_rows) and the index over it
(subgnn_amd/neighbors.py) end to end.

  * bit for bit against tests/neighbors_cases.topk_ref for dot and l2 on the dyadic grids, at every edge of Q, N, D, k, splits;
  * ties by the smaller row; the same bits for every split count on a random problem;
  * random inputs, all three metrics, against the float64 reference within the derived tolerance (neighbors_cases.tolerance);
  * exclude, fillers, NaN, strided queries; refusals; guard words around both outputs in every call of ``_run``;
  * the index of a trained run: a dataset subgraph finds a row with its own embedding, files, leave-one-out, the CLI.

Every call of ``_run`` goes through the raw ABI into guarded buffers AND through ops.topk_rows, and the two must agree."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbors_cases as NC

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
GUARD = 64                                   # words on either side of an output
GUARD_F, GUARD_I = -12345.5, -0x5A5A5A5A5A5A5A5A


def _guarded(Q, k):
    s = torch.full((Q * k + 2 * GUARD,), GUARD_F, dtype=torch.float32, device=DEV)
    i = torch.full((Q * k + 2 * GUARD,), GUARD_I, dtype=torch.int64, device=DEV)
    return s, i


def _guards_intact(s, i, Q, k):
    for buf, g in ((s, GUARD_F), (i, GUARD_I)):
        assert bool((buf[:GUARD] == g).all()) and bool((buf[GUARD + Q * k:] == g).all()), 'a guard word was overwritten'


def _raw(q, bank, k, metric, exclude, splits, q_aux, b_aux):
    """sgnn_topk_rows into guarded buffers -> (rc, score buffer, index buffer)."""
    from subgnn_amd import _lib, ops
    lib = _lib.load()
    Q, D = q.shape
    N = bank.shape[0]
    s, i = _guarded(Q, k)
    nbytes = max(0, int(lib.sgnn_topk_rows_workspace_bytes(Q, N, min(max(k, 1), 64), splits)))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)
    rc = lib.sgnn_topk_rows(p(q), q.stride(0) if Q > 1 else max(D, q.stride(0)), Q, p(bank) if N else None,
                            bank.stride(0) if N > 1 else D, N, D, k, NC.METRIC_CODE[metric], p(q_aux), p(b_aux) if N else None,
                            p(exclude), splits, p(s, 4 * GUARD), p(i, 8 * GUARD), p(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    return rc, s, i


def _run(q, bank, k, metric, exclude=None, splits=0):
    """(scores, indices) as numpy, through both entries; guards checked."""
    from subgnn_amd import ops
    q = q if isinstance(q, torch.Tensor) else torch.from_numpy(q).to(DEV)
    bank = bank if isinstance(bank, torch.Tensor) else torch.from_numpy(bank).to(DEV)
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int64, device=DEV)
    Q = q.shape[0]
    qa, ba = ops.topk_aux(q, metric), ops.topk_aux(bank, metric)
    rc, s, i = _raw(q, bank, k, metric, ex, splits, qa, ba)
    assert rc == 0
    _guards_intact(s, i, Q, k)
    sc, ix = s[GUARD:GUARD + Q * k].view(Q, k), i[GUARD:GUARD + Q * k].view(Q, k)
    sc2, ix2 = ops.topk_rows(q, bank, k, metric=metric, exclude=ex, splits=splits)
    assert sc2.shape == (Q, k) and sc2.dtype == torch.float32 and ix2.dtype == torch.int64
    assert torch.equal(sc.view(torch.int32), sc2.view(torch.int32)) and torch.equal(ix, ix2)
    return sc.cpu().numpy(), ix.cpu().numpy()


def _same_bits(got, want, what):
    gs, gi = got
    ws, wi = want
    assert np.array_equal(gi, wi), '%s: indices differ at %s' % (what, np.argwhere(gi != wi)[:5].tolist())
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), '%s: score bits differ at %s' % (
        what, np.argwhere(gs.view(np.uint32) != ws.view(np.uint32))[:5].tolist())


# ---- bit for bit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', NC.exact_cases(), ids=NC.case_id)
def test_dyadic_grids_bit_for_bit(case):
    q, bank = NC.make_inputs(case)
    for metric in ('dot', 'l2'):
        got = _run(q, bank, case['k'], metric, splits=case['splits'])
        _same_bits(got, NC.topk_ref(q, bank, case['k'], metric), '%s %s' % (NC.case_id(case), metric))


def test_operands_keep_their_places():
    """Asymmetric data no transposed or permuted tile survives: q = one-hot rows, bank[j][d] = 64 j + d exactly."""
    Q, N, D = 33, 130, 33
    q = np.zeros((Q, D), dtype=np.float32)
    q[np.arange(Q), np.arange(Q) % D] = 1
    bank = (64.0 * np.arange(N)[:, None] + np.arange(D)[None, :]).astype(np.float32)
    sc, ix = _run(q, bank, 3, 'dot', splits=1)
    for i in range(Q):
        assert ix[i].tolist() == [N - 1, N - 2, N - 3]
        assert sc[i].tolist() == [64.0 * j + i % D for j in (N - 1, N - 2, N - 3)]
    sc, ix = _run(q, -bank, 2, 'dot', splits=2)
    assert ix.tolist() == [[0, 1]] * Q and sc[:, 1].tolist() == [-(64.0 + i % D) for i in range(Q)]


# ---- ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('splits', NC.SPLITS)
def test_identical_rows_come_back_in_index_order(splits):
    rng = np.random.default_rng(1)
    row = NC.dyadic(rng, 1, 9)
    bank = np.repeat(row, 200, axis=0)
    q = NC.dyadic(rng, 5, 9)
    for metric in ('dot', 'cosine', 'l2'):
        for k in (1, 7, 64):
            sc, ix = _run(q, bank, k, metric, splits=splits)
            assert np.array_equal(ix, np.tile(np.arange(k), (5, 1))), (metric, k)
            assert np.all(sc.view(np.uint32) == sc[:, :1].view(np.uint32))


@pytest.mark.parametrize('splits', NC.SPLITS)
def test_interleaved_repeats_follow_the_reference_order(splits):
    rng = np.random.default_rng(2)
    rows = NC.dyadic(rng, 5, 6)
    bank = np.tile(rows, (40, 1))                                    # row j is rows[j % 5]
    q = NC.dyadic(rng, 33, 6)
    for metric in ('dot', 'l2'):
        for k in (2, 41, 64):
            _same_bits(_run(q, bank, k, metric, splits=splits), NC.topk_ref(q, bank, k, metric), '%s k=%d' % (metric, k))


# ---- geometry -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def random_problem():
    c = NC.RANDOM_CASE
    q, bank = NC.make_inputs(c)
    return c, q, bank


@pytest.mark.parametrize('metric', ['dot', 'cosine', 'l2'])
def test_result_does_not_depend_on_the_split_count(random_problem, metric):
    c, q, bank = random_problem
    base = _run(q, bank, c['k'], metric, splits=1)
    for s in (2, 7, 0):
        _same_bits(_run(q, bank, c['k'], metric, splits=s), base, 'splits=%d against 1' % s)


# ---- random inputs against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['dot', 'cosine', 'l2'])
def test_random_inputs_within_the_derived_tolerance(random_problem, metric):
    c, q, bank = random_problem
    k = c['k']
    sc, ix = _run(q, bank, k, metric)
    s64, tol = NC.scores_f64(q, bank, metric), NC.tolerance(q, bank, metric)
    sign = 1.0 if metric == 'l2' else -1.0                           # sign * score: smaller is better
    worst = [0.0, 0.0]
    for i in range(c['Q']):
        assert len(set(ix[i].tolist())) == k and ix[i].min() >= 0 and ix[i].max() < c['N']
        err = np.abs(sc[i].astype(np.float64) - s64[i, ix[i]])
        worst[0] = max(worst[0], float((err / tol[i, ix[i]]).max()))
        assert np.all(err <= tol[i, ix[i]]), (i, err.max())
        ref_order = NC.order_rows(s64[i:i + 1], metric)[0]
        kth = ref_order[k - 1]
        bound = sign * s64[i, kth]
        # no returned row is worse than the reference's k-th by more than 2 tol
        excess = sign * s64[i, ix[i]] - bound
        assert np.all(excess <= 2 * np.maximum(tol[i, ix[i]], tol[i, kth])), (i, excess.max())
        # every row better than the reference's k-th by more than 2 tol is returned
        margin = bound - sign * s64[i]
        must = np.nonzero(margin > 2 * np.maximum(tol[i], tol[i, kth]))[0]
        assert set(must.tolist()) <= set(ix[i].tolist()), i
        worst[1] = max(worst[1], len(must) / k)
        # and the returned list is in the order of its own float32 scores
        key = sign * sc[i].astype(np.float64)
        assert np.all((key[1:] > key[:-1]) | ((key[1:] == key[:-1]) & (ix[i][1:] > ix[i][:-1])))
    print('%s: largest error / tolerance %.3f; rows forced by the margin: up to %.0f %% of k' % (metric, worst[0], 100 * worst[1]))


# ---- edges --------------------------------------------------------------------------------------------------------------------
def test_excluded_rows_never_appear_and_leave_a_filler():
    c = NC.EDGE_CASES[2]
    q, bank = NC.make_inputs(c)
    Q, N, k = c['Q'], c['N'], c['k']
    assert N == k
    ex = np.arange(Q, dtype=np.int64) % N
    ex[3], ex[4] = -1, N + 5                                         # none; no row of the bank
    for metric in ('dot', 'cosine', 'l2'):
        for splits in (0, 3):
            sc, ix = _run(q, bank, k, metric, exclude=ex, splits=splits)
            for i in range(Q):
                if 0 <= ex[i] < N:
                    assert ex[i] not in ix[i] and ix[i, -1] == -1 and sc[i, -1] == (np.inf if metric == 'l2' else -np.inf)
                    assert sorted(ix[i, :-1].tolist()) == [j for j in range(N) if j != ex[i]]
                else:
                    assert sorted(ix[i].tolist()) == list(range(N))
            if metric != 'cosine':
                want = NC.topk_ref(q, bank, k, metric, exclude=np.where(ex < N, ex, -1))
                _same_bits((sc, ix), want, metric)


@pytest.mark.parametrize('case', NC.EDGE_CASES[:2], ids=NC.case_id)
def test_fewer_rows_than_k_gives_fillers(case):
    q, bank = NC.make_inputs(case)
    for metric in ('dot', 'cosine', 'l2'):
        for splits in (0, 2):
            sc, ix = _run(q, bank, case['k'], metric, splits=splits)
            N = case['N']
            assert np.all(ix[:, N:] == -1) and np.all(sc[:, N:] == (np.inf if metric == 'l2' else -np.inf))
            assert all(sorted(r[:N].tolist()) == list(range(N)) for r in ix)
            if metric != 'cosine':
                _same_bits((sc, ix), NC.topk_ref(q, bank, case['k'], metric), metric)


def test_a_nan_row_ranks_last():
    rng = np.random.default_rng(3)
    q, bank = NC.dyadic(rng, 4, 5), NC.dyadic(rng, 140, 5)
    bank[7, 2] = np.nan
    bank[133, 0] = np.nan
    for metric in ('dot', 'l2'):
        for splits in (1, 2):
            sc, ix = _run(q, bank, 64, metric, splits=splits)
            assert 7 not in ix and 133 not in ix and not np.isnan(sc).any()
        sc, ix = _run(q, bank[:40], 40, metric)
        assert np.all(ix[:, -1] == 7) and np.isnan(sc[:, -1]).all() and not np.isnan(sc[:, :-1]).any()
        want = NC.topk_ref(q, bank[:40], 40, metric)
        assert np.array_equal(ix, want[1]) and np.array_equal(sc[:, :-1].view(np.uint32), want[0][:, :-1].view(np.uint32))


def test_a_column_slice_of_a_wider_matrix_is_a_query():
    rng = np.random.default_rng(4)
    wide = torch.from_numpy(NC.dyadic(rng, 35, 40)).to(DEV)
    bank = NC.dyadic(rng, 70, 9)
    q = wide[:, 3:12]
    assert q.stride() == (40, 1) and not q.is_contiguous()
    for metric in ('dot', 'l2'):
        _same_bits(_run(q, bank, 5, metric), NC.topk_ref(q.cpu().numpy(), bank, 5, metric), metric)
    wb = torch.from_numpy(NC.dyadic(rng, 70, 33)).to(DEV)
    _same_bits(_run(q, wb[:, 20:29], 5, 'dot', splits=2), NC.topk_ref(q.cpu().numpy(), wb[:, 20:29].cpu().numpy(), 5, 'dot'), 'bank slice')


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_the_op_refuses_what_the_kernel_does_not_serve():
    from subgnn_amd import ops
    q, bank = torch.zeros(4, 6, device=DEV), torch.zeros(9, 6, device=DEV)
    with pytest.raises(ValueError, match='64'):
        ops.topk_rows(q, bank, 65)
    with pytest.raises(ValueError, match='64'):
        ops.topk_rows(q, bank, 0)
    with pytest.raises(ValueError):
        ops.topk_rows(q.cpu(), bank.cpu(), 2)
    with pytest.raises(ValueError):
        ops.topk_rows(q, bank[:, :5], 2)
    with pytest.raises(ValueError):
        ops.topk_rows(q.double(), bank.double(), 2)
    with pytest.raises(ValueError):
        ops.topk_rows(q, bank, 2, metric='manhattan')
    with pytest.raises(ValueError):
        ops.topk_rows(q.t().contiguous().t(), bank, 2)               # column stride 4


def test_the_abi_refuses_and_writes_nothing():
    q, bank = torch.ones(4, 6, device=DEV), torch.ones(9, 6, device=DEV)
    qa, ba = torch.ones(4, device=DEV), torch.ones(9, device=DEV)
    for k, metric, a, b in ((65, 'dot', None, None), (0, 'dot', None, None), (2, 'cosine', None, ba), (2, 'l2', qa, None)):
        rc, s, i = _raw(q, bank, k, metric, None, 0, a, b)
        assert rc == -1, (k, metric)
        assert bool((s == GUARD_F).all()) and bool((i == GUARD_I).all())
    from subgnn_amd import _lib, ops
    lib = _lib.load()
    s, i = _guarded(4, 2)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.sgnn_topk_rows(p(q), 6, 4, p(bank), 6, 9, 6, 2, 7, None, None, None, 0, p(s), p(i), None, 0, ops._stream()) == -1
    assert lib.sgnn_topk_rows(p(q), 5, 4, p(bank), 6, 9, 6, 2, 0, None, None, None, 0, p(s), p(i), None, 0, ops._stream()) == -1
    assert lib.sgnn_topk_rows(p(q), 6, 4, p(bank), 6, 9, 0, 2, 0, None, None, None, 0, p(s), p(i), None, 0, ops._stream()) == -1
    assert lib.sgnn_topk_rows(p(q), 6, 4, p(bank), 6, 9, 6, 2, 0, None, None, None, 0, None, p(i), None, 0, ops._stream()) == -1
    torch.cuda.synchronize()
    assert bool((s == GUARD_F).all()) and bool((i == GUARD_I).all())


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
    """The recipe of tests/test_gpu_predict.py's ``run``: the generated 24-subgraph COMPONENT dataset, two epochs, one kept
    checkpoint; then the predictor of the finished run and the index of its three splits."""
    from conftest import load_golden
    from subgnn_amd import config, train_config, prepare_dataset as pd, precompute_graph_metrics as pgm
    from subgnn_amd.neighbors import SubgraphIndex
    from subgnn_amd.predict import Predictor
    root = tmp_path_factory.mktemp('neighbors_run')
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
    yield dict(root=root, cfg=cfg, results=root / 'results', rc=rc, P=P, index=index, before=before)
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


def _dataset_requests(index):
    return [list(s) for s in index.subgraphs]


def test_index_of_a_run_describes_the_dataset(run):
    index, P = run['index'], run['P']
    m = P.model
    n = sum(len(getattr(m, sp + '_sub_G')) for sp in ('train', 'val', 'test'))
    assert len(index) == n and index.width == m.lin.in_features and index.embeddings.is_cuda
    assert index.checkpoint == P.restored_from and index.metric == 'cosine'
    lines = [l.split('\t') for l in open(run['root'] / 'ds' / 'subgraphs.pth').read().splitlines() if l.strip()]
    by_nodes = {tuple(int(v) for v in c[0].split('-')): c[1].split('-') for c in lines}
    for j in range(n):
        sp, row, nodes, labels = index.describe(j)
        assert [v + 1 for v in nodes] == getattr(m, sp + '_sub_G')[row]
        assert labels == by_nodes[tuple(nodes)]


def test_a_dataset_subgraph_finds_its_own_embedding(run):
    index, P = run['index'], run['P']
    res = P.nearest(index, _dataset_requests(index), k=3)
    sc, ix, E = res['scores'].cpu().numpy(), res['indices'].cpu().numpy(), res['embeddings']
    bank = index.embeddings
    assert torch.equal(E.view(torch.int32), bank.view(torch.int32))                 # keyed draws: the same rows, bit for bit
    assert torch.equal(bank[torch.from_numpy(ix[:, 0]).to(bank.device)].view(torch.int32), E.view(torch.int32))
    e = E.cpu().numpy()
    tol = np.diag(NC.tolerance(e, e, 'cosine'))
    print('rank-0 cosine: largest |score - 1| / tolerance %.3f' % float((np.abs(sc[:, 0].astype(np.float64) - 1) / tol).max()))
    assert np.all(np.abs(sc[:, 0].astype(np.float64) - 1) <= tol)


def test_self_neighbors_leave_the_row_out(run):
    index = run['index']
    sc, ix = index.self_neighbors(3)
    ix = ix.cpu().numpy()
    assert ix.shape == (len(index), 3) and ix.min() >= 0
    assert not np.any(ix == np.arange(len(index))[:, None])
    e = index.embeddings.cpu().numpy()
    s64, tol = NC.scores_f64(e, e, 'cosine'), NC.tolerance(e, e, 'cosine')
    rows = np.arange(len(index))[:, None]
    assert np.all(np.abs(sc.cpu().numpy() - s64[rows, ix]) <= tol[rows, ix])


def test_index_file_round_trip_queries_identically(run, tmp_path):
    from subgnn_amd.neighbors import SubgraphIndex
    index, P = run['index'], run['P']
    f = tmp_path / 'index.npz'
    index.save(f)
    again = SubgraphIndex.load(f, DEV, predictor=P)
    assert torch.equal(again.embeddings.view(torch.int32), index.embeddings.view(torch.int32))
    assert again.subgraphs == index.subgraphs and again.labels == index.labels and again.checkpoint == index.checkpoint
    req = _dataset_requests(index)[:7]
    a, b = index.query(P, req, 4), again.query(P, req, 4)
    assert torch.equal(a['indices'], b['indices']) and torch.equal(a['scores'].view(torch.int32), b['scores'].view(torch.int32))


def test_building_and_querying_leave_the_models_splits_untouched(run):
    P, index = run['P'], run['index']
    P.nearest(index, _dataset_requests(index)[:3], k=2)
    after = _split_objects(P.model)
    assert after.keys() == run['before'].keys()
    for k, v in run['before'].items():
        assert after[k] is v, k


def test_cli_in_a_child_process(run, tmp_path):
    index, P = run['index'], run['P']
    req = _dataset_requests(index)[2:6]
    f = tmp_path / 'requests.txt'
    f.write_text(''.join('-'.join(str(v) for v in s) + '\n' for s in req))
    out, npz = tmp_path / 'near.txt', tmp_path / 'index.npz'
    k = 3
    r = subprocess.run([sys.executable, '-m', 'subgnn_amd.neighbors', '-config_path', str(run['cfg']), '-project_root', str(run['root']),
                        '-restoreModelPath', str(run['results']), '-subgraphs', str(f), '-out', str(out), '-k', str(k),
                        '-index', str(npz)], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert npz.exists()
    lines = out.read_text().splitlines()
    assert len(lines) == len(req) * k
    here = index.query(P, req, k)
    sc, ix = here['scores'].cpu().numpy(), here['indices'].cpu().numpy()
    for n, line in enumerate(lines):
        cols = line.split('\t')
        assert len(cols) == 7
        i, rank = divmod(n, k)
        assert (int(cols[0]), int(cols[1])) == (i, rank)
        assert np.float32(float(cols[2])).view(np.uint32) == sc[i, rank].view(np.uint32)
        sp, row, nodes, labels = index.describe(int(ix[i, rank]))
        assert cols[3] == sp and int(cols[4]) == row and [int(v) for v in cols[5].split('-')] == nodes and cols[6].split('-') == labels

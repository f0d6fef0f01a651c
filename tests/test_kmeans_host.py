"""CPU: k-means' reference, cases, initialisation, figures, files and command line (tests/kmeans_cases.py, subgnn_amd/cluster.py,
the host side of csrc/kmeans.hip).  No GPU: the kernels themselves are tests/test_gpu_kmeans.py's."""
import json
import os
import re

import numpy as np
import pytest
import torch

import kmeans_cases as KC
import neighbors_cases as NC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope='module')
def feature():
    """The cases, references and restatements below describe ops.kmeans_step: without it they describe nothing."""
    from subgnn_amd import ops, cluster                              # noqa: F401
    assert hasattr(ops, 'kmeans_step') and hasattr(ops, 'kmeans')


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
NAMES = ('sgnn_kmeans_max_k', 'sgnn_kmeans_slots', 'sgnn_kmeans_workspace_bytes', 'sgnn_kmeans_step', 'sgnn_kmeans_finish')


def test_the_header_and_the_signatures_carry_the_new_entries_and_agree_on_the_abi():
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    from subgnn_amd import build, _lib, ops
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, txt), name
        assert name in _lib.SIGNATURES
    assert 'Replaces no reference function' in txt[txt.index('n2   k-means'):txt.index('sgnn_kmeans_max_k(void)')]
    assert re.search(r'#define SGNN_ABI_VERSION 14\b', txt) and _lib.load().sgnn_abi_version() == 14
    assert 'kmeans.hip' in build.SOURCES
    assert callable(ops.kmeans_step) and callable(ops.kmeans)


def test_the_queries_answer_on_the_host_and_bad_arguments_are_refused():
    """No GPU is touched: the checks precede any launch (NULL pointers never reach one)."""
    from subgnn_amd import _lib
    lib = _lib.load()
    assert lib.sgnn_kmeans_max_k() == KC.MAX_K == 1024
    for c in KC.exact_cases() + [KC.RANDOM_CASE, dict(N=50000, K=64, D=516), dict(N=10 ** 6, K=256, D=128),
                                 dict(N=2 ** 31 - 257, K=1024, D=2 ** 23 - 1)]:
        nt, per, S, W = KC.geometry(c['N'], c['K'], c['D'])
        assert lib.sgnn_kmeans_slots(c['N'], c['K'], c['D']) == S, c
        assert lib.sgnn_kmeans_workspace_bytes(c['N'], c['K'], c['D']) == KC.workspace_bytes(c['N'], c['K'], c['D']), c
        assert 1 <= S <= KC.MAX_SLOTS and (S - 1) * per < nt <= S * per                  # the bound; no slot is empty
        assert S == 1 or S * c['K'] * c['D'] * 4 <= KC.PART_CAP
    for N, K, D in ((0, 1, 1), (4, 0, 1), (4, 1025, 1), (4, 1, 0), (2 ** 31, 1, 1), (4, 1, 2 ** 23), (-1, 1, 1)):
        assert lib.sgnn_kmeans_workspace_bytes(N, K, D) == -1 and lib.sgnn_kmeans_slots(N, K, D) == -1, (N, K, D)
    assert lib.sgnn_kmeans_step(None, 4, 1, None, 4, 1, 4, 2, None, None, None, None, None, None, 0, None) == -1
    assert lib.sgnn_kmeans_finish(None, 0, 1, 1, 4, 2, None, 4, None, None, None, None, None, None, None, 0, None) == -1


def test_the_ops_refuse_on_the_host():
    from subgnn_amd import ops
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        ops.kmeans_step(x, x[:2])                                    # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        ops.kmeans_step(x, x[:2], metric='dot')
    with pytest.raises(ValueError):
        ops.kmeans(x, 2)
    with pytest.raises(ValueError):
        ops.kmeans(x, 2, metric='dot')


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def test_every_branch_of_the_dispatch_is_reached_by_some_case():
    reached = set()
    for c in KC.exact_cases() + [KC.RANDOM_CASE]:
        b = KC.branches(**c)
        assert b <= KC.ALL_BRANCHES, b - KC.ALL_BRANCHES
        reached |= b
    assert reached == KC.ALL_BRANCHES, KC.ALL_BRANCHES - reached


def test_the_cases_cover_every_listed_size():
    cs = KC.exact_cases()
    for name, values in (('N', KC.NS), ('K', KC.KS), ('D', KC.DS)):
        assert set(values) <= {c[name] for c in cs}, name
    assert {1, 31, 32, 33} <= set(KC.NS) and {1, 2, 33} <= set(KC.KS) and any(k > KC.TC for k in KC.KS)
    assert set(KC.DS) == {1, 31, 32, 33, 130}
    assert KC.geometry(31, 7, 9)[2] == KC.geometry(32, 7, 9)[2] == 1 and KC.geometry(33, 7, 9)[2] == 2   # a slot's row range
    nt, per, S, _ = KC.geometry(65605, 7, 9)
    assert per == 3 and nt - (S - 1) * per == 2                                          # several ranges, a ragged last one
    cap = KC.PART_CAP // (KC.BIG['K'] * KC.BIG['D'] * 4)
    assert KC.geometry(**{k: KC.BIG[k] for k in 'NKD'})[1:3] == (2, 65) and 65 <= cap == 126 < -(-KC.BIG['N'] // KC.TR)
    assert 2 * len(cs) <= 40                                          # a few dozen launches, both metrics


def test_the_dyadic_cases_are_order_free():
    for c in KC.exact_cases():
        X, C, prev = KC.make_inputs(c)
        for x in (X, C):
            m = x * 8
            assert x.dtype == np.float32 and np.array_equal(m, np.round(m)) and np.abs(m).max() <= 8
        assert c['N'] * 8 < 2 ** 23 and c['D'] <= 130                                    # every subset sum is exact in float32
        K = c['K']
        if c['N'] * K * c['D'] <= 10 ** 7:
            assign, score = KC.assign_ref(X, C, 'l2')
            assert np.array_equal(score.astype(np.float64), NC.scores_f64(X, C, 'l2')[np.arange(c['N']), assign])
        else:                                                        # any assignment serves: the sums' exactness is the grid's
            assign = np.random.default_rng(1).integers(0, K, size=c['N']).astype(np.int32)
        slots = KC.slot_rows(c['N'], K, c['D'])
        fwd, rev = KC.sums_f32(X, assign, K, slots), KC.sums_f32(X, assign, K, slots, reverse=True)
        assert np.array_equal(fwd.view(np.uint32), rev.view(np.uint32)), c
        assert np.array_equal(fwd.astype(np.float64), KC.sums_f64(X, assign, K)), c
        one = KC.sums_f32(X, assign, K, [(0, c['N'])])
        assert np.array_equal(fwd.view(np.uint32), one.view(np.uint32)), c               # whatever the slots


def test_step_reference_on_a_hand_made_input():
    X = np.array([[1, 0], [3, 0], [0, 2], [0, 4], [9, 9]], dtype=np.float32)
    C = np.array([[2, 0], [0, 3], [50, 50], [0, 3]], dtype=np.float32)
    assign, score = KC.assign_ref(X, C, 'l2')
    assert assign.tolist() == [0, 0, 1, 1, 1] and score.tolist() == [1, 1, 1, 1, 117]     # centre 3 duplicates 1: the smaller wins
    r = KC.step_ref(X, C, assign, score, np.array([0, 1, 1, 1, 2], dtype=np.int32), [(0, 5)])
    assert r['counts'].tolist() == [2, 3, 0, 0] and r['empty'] == 2 and r['changed'] == 2 and r['inertia'] == 121.0
    assert r['sums'].tolist() == [[4, 0], [9, 15], [0, 0], [0, 0]]
    assert r['centers'].tolist() == [[2, 0], [3, 5], [50, 50], [0, 3]]                    # empty clusters keep their centre
    assert KC.step_ref(X, C, assign, score, None, [(0, 5)])['changed'] == 5


def test_the_sums_tolerance_is_the_stated_bound():
    X = np.array([[1.0, -2.0], [0.5, 4.0], [3.0, 1.0]], dtype=np.float32)
    a = np.array([1, 1, 0], dtype=np.int32)
    t = KC.sums_tolerance(X, a, 3, 5)
    g = lambda n: n * KC.U / (1 - n * KC.U)
    assert np.allclose(t, [[g(6) * 3, g(6) * 1], [g(7) * 1.5, g(7) * 6], [0, 0]], rtol=1e-12, atol=0)
    ct = KC.centers_tolerance(X, a, 3, 5, np.array([[3.0, 1.0], [0.75, 1.0], [7.0, 7.0]]))
    assert np.allclose(ct[1], [g(7) * 1.5 / 2 + 2 * KC.U * 0.75, g(7) * 6 / 2 + 2 * KC.U], rtol=1e-12) and ct[2].tolist() == [0, 0]


# ---- initialisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 5])
def test_kmeans_plus_plus_restatement_picks_the_rows_of_a_plain_second_implementation(seed):
    rng = np.random.default_rng(100 + seed)
    X = rng.integers(-6, 7, size=(60, 3)).astype(np.float32)         # integer grid: every distance and cumulative sum exact
    X[7] = X[3]
    assert KC.init_rows(X, 9, 'k-means++', seed) == KC.init_rows_plain(X.tolist(), 9, seed)
    exact = lambda X, r: ((X.astype(np.float64) - X[r].astype(np.float64)) ** 2).sum(1)
    assert KC.init_rows(X, 9, 'k-means++', seed, dist=exact) == KC.init_rows(X, 9, 'k-means++', seed)


def test_initialisation_of_coincident_rows_takes_the_smallest_unchosen_row():
    X = np.ones((5, 2), dtype=np.float32)
    first = min(int(np.random.default_rng(3).random(4)[0] * 5), 4)
    want = [first] + [r for r in range(5) if r != first][:3]
    assert KC.init_rows(X, 4, 'k-means++', 3) == want == KC.init_rows_plain(X.tolist(), 4, 3)
    r = KC.init_rows(X, 4, 'random', 3)
    assert r == [int(v) for v in np.random.default_rng(3).choice(5, 4, replace=False)] and len(set(r)) == 4


# ---- the figures --------------------------------------------------------------------------------------------------------------
def test_nmi_equals_scikit_learns():
    from sklearn.metrics import normalized_mutual_info_score
    from subgnn_amd.cluster import nmi
    rng = np.random.default_rng(8)
    for n, ka, kb in ((50, 3, 4), (500, 7, 2), (24, 3, 3), (10, 1, 3), (10, 4, 1), (6, 1, 1)):
        a, b = rng.integers(0, ka, size=n), rng.integers(0, kb, size=n)
        assert abs(nmi(a, b) - normalized_mutual_info_score(b, a)) <= 1e-12, (n, ka, kb)
    a = rng.integers(0, 5, size=200)
    assert abs(nmi(a, (a * 3 + 1) % 5) - 1.0) <= 1e-12
    assert abs(nmi(a, a // 2) - normalized_mutual_info_score(a // 2, a)) <= 1e-12


def test_purity_and_label_counts_on_hand_made_inputs():
    from subgnn_amd.cluster import purity, label_figures, Clustering
    assert purity([0, 0, 0, 1, 1, 2], [5, 5, 7, 7, 7, 9]) == 5 / 6
    assert purity([0, 0, 1, 1], [1, 2, 1, 2]) == 0.5
    counts, pur, mi = label_figures([0, 0, 1, 1, 1, 2], [['a'], ['a', 'z'], ['b'], ['b'], ['a'], []], 4)
    assert counts == [{'a': 2, 'z': 1}, {'b': 2, 'a': 1}, {}, {}] and pur == 5 / 6
    cl = Clustering([0, 0, 1, 1, 1, 2], np.zeros((4, 2), dtype=np.float32), [2, 3, 1, 0], np.zeros(6, dtype=np.float32), 0.0, 2,
                    True, 'l2', label_counts=counts + [])
    assert cl.majority == ['a', 'b', None, None] and cl.cluster_purity == [2 / 3, 2 / 3, 0.0, 0.0]
    tie = Clustering([0, 0], np.zeros((1, 2), dtype=np.float32), [2], np.zeros(2, dtype=np.float32), 0.0, 1, True, 'l2',
                     label_counts=[{'y': 1, 'x': 1}])
    assert tie.majority == ['x']


def test_medoid_order_is_best_score_then_smaller_row():
    from subgnn_amd.cluster import medoid_rows
    labels = [0, 1, 0, 0, 1, 0, 2]
    scores = [0.5, 0.1, 0.25, 0.5, 0.1, 0.25, 0.0]
    assert medoid_rows(labels, scores, 4, 'l2', 3) == [[2, 5, 0], [1, 4], [6], []]
    assert medoid_rows(labels, scores, 4, 'cosine', 3) == [[0, 3, 2], [1, 4], [6], []]
    assert medoid_rows(labels, scores, 4, 'l2', 0) == [[], [], [], []]
    assert medoid_rows(labels, scores, 4, 'l2', 9)[0] == [2, 5, 0, 3]


# ---- files --------------------------------------------------------------------------------------------------------------------
def _clustering():
    from subgnn_amd.cluster import Clustering
    return Clustering([0, 2, 2, 1], torch.arange(6, dtype=torch.float32).view(3, 2) / 7, [1, 1, 2],
                      torch.tensor([0.5, 0.25, 1.5, 0.0]), 2.25, 4, True, 'cosine', torch.tensor([1.0, 0.5, 0.25]),
                      [[0], [3], [1, 2]], [{'a': 1}, {}, {'b': 1, 'c d': 2}], 0.75, 0.5)


def test_clustering_round_trips_through_a_file(tmp_path):
    from subgnn_amd.cluster import Clustering
    a = _clustering()
    f = tmp_path / 'cl.npz'
    a.save(f)
    assert os.listdir(tmp_path) == ['cl.npz']                        # the temporary name is gone
    b = Clustering.load(f)
    for name in ('labels', 'centers', 'sizes', 'scores', 'center_aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)) and getattr(a, name).dtype == getattr(b, name).dtype, name
    for name in ('inertia', 'n_iter', 'converged', 'metric', 'medoids', 'label_counts', 'purity', 'nmi'):
        assert getattr(a, name) == getattr(b, name), name
    assert b.labels.dtype == torch.int64 and b.n_clusters == 3
    a.save(f)                                                        # over an existing file
    assert Clustering.load(f).medoids == a.medoids
    with pytest.raises(ValueError):
        a.save(tmp_path / 'cl.txt')
    with np.load(f, allow_pickle=False) as z:                        # no pickles inside
        assert all(z[k].dtype != object for k in z.files)
    s = json.loads(json.dumps(a.summary({'seed': 1})))
    assert s['clusters'][2] == {'cluster': 2, 'size': 2, 'label_counts': {'b': 1, 'c d': 2}, 'majority': 'c d', 'purity': 2 / 3,
                                'medoids': [1, 2]}
    assert s['purity'] == 0.75 and s['nmi'] == 0.5 and s['arguments'] == {'seed': 1} and s['n_clusters'] == 3


def test_cluster_refuses_dot_and_unknown_metrics():
    from subgnn_amd.neighbors import SubgraphIndex
    from subgnn_amd.cluster import Clustering
    idx = SubgraphIndex.from_embeddings(torch.zeros(3, 2), metric='dot')
    with pytest.raises(ValueError, match='dot'):
        idx.cluster(2)
    with pytest.raises(ValueError):
        idx.cluster(2, metric='manhattan')
    with pytest.raises(ValueError):
        Clustering([0], np.zeros((1, 2), dtype=np.float32), [1], np.zeros(1, dtype=np.float32), 0.0, 1, True, 'dot')


# ---- command line -------------------------------------------------------------------------------------------------------------
BASE = ['-config_path', 'c.json', '-restoreModelPath', 'run', '-n_clusters', '4', '-out', 'out.txt']


def test_cli_parser_defaults():
    from subgnn_amd import cluster
    a = cluster.parse_args(BASE)
    assert (a.n_clusters, a.metric, a.splits, a.index, a.init, a.n_init, a.max_iter, a.seed, a.medoids, a.subgraphs, a.summary) == (
        4, 'cosine', ('train', 'val', 'test'), None, 'k-means++', 1, 100, 0, 5, None, None)
    a = cluster.parse_args(BASE + ['-metric', 'l2', '-splits', 'val,train', '-index', 'i.npz', '-init', 'random', '-n_init', '3',
                                   '-max_iter', '7', '-seed', '2', '-medoids', '0', '-subgraphs', 'r.txt', '-summary', 's.json'])
    assert (a.metric, a.splits, a.index, a.init, a.n_init, a.max_iter, a.seed, a.medoids, a.subgraphs, a.summary) == (
        'l2', ('val', 'train'), 'i.npz', 'random', 3, 7, 2, 0, 'r.txt', 's.json')


@pytest.mark.parametrize('extra', [['-n_clusters', '0'], ['-metric', 'dot'], ['-metric', 'manhattan'], ['-splits', 'train,dev'],
                                   ['-index', 'out.txt'], ['-index', 'i.npy'], ['-init', 'furthest'], ['-n_init', '0'],
                                   ['-max_iter', '0'], ['-medoids', '-1'], ['-subgraphs', 'out.txt'], ['-summary', 's.txt'],
                                   ['-batch_size', '0']])
def test_cli_parser_refuses(extra, capsys):
    from subgnn_amd import cluster
    with pytest.raises(SystemExit):
        cluster.parse_args(BASE + extra)
    capsys.readouterr()


def test_output_line_round_trips_a_float32():
    from subgnn_amd.cluster import format_line, HEADER
    assert HEADER.split('\t') == ['split', 'row', 'cluster', 'score', 'nodes', 'labels']
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.standard_normal(200).astype(np.float32), (rng.standard_normal(200) * 1e-20).astype(np.float32),
                           np.array([np.float32(1) - np.float32(2.0 ** -24), 1.0, 0.0, 3.4028235e38], dtype=np.float32)])
    for i, v in enumerate(vals):
        cols = format_line('val', i, 3, v, [4, 0, 11], ['x', 'y']).split('\t')
        assert len(cols) == 6 and cols[:3] == ['val', str(i), '3'] and cols[4:] == ['4-0-11', 'x-y']
        assert np.float32(float(cols[3])).view(np.uint32) == v.view(np.uint32), (v, cols[3])
    assert format_line('request', 0, 1, np.float32(0.5), [7], []).split('\t') == ['request', '0', '1', '0.5', '7', '']


# ---- the whole fit's margin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_the_whole_fit_case_keeps_every_row_clear_of_a_decision_boundary(metric):
    """What makes tests/test_gpu_kmeans.py's demand (the float32 kernel's labels EQUAL the float64 run's) a fair one: at every
    iteration of the reference run every row's gap between best and second-best score exceeds twice the allowance of
    kmeans_cases.lloyd_f64 (both score tolerances plus the effect of the centres' own rounding bound); no cluster empties;
    the run converges inside max_iter."""
    f = KC.FIT
    X = KC.blobs(metric)
    rows = KC.init_rows(X, f['K'], 'k-means++', 0)
    assert len(set(rows)) == f['K']
    r = KC.lloyd_f64(X, rows, metric, f['max_iter'], KC.geometry(f['N'], f['K'], f['D'])[2])
    print('%s: converged at iteration %s, smallest gap %.1f x twice the allowance' % (metric, r['n_iter'], r['min_margin']))
    assert r['n_iter'] is not None and 2 <= r['n_iter'] < f['max_iter']
    assert r['no_empty']
    assert r['min_margin'] >= 1.0                                    # gap >= 2 x allowance

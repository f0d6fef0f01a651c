"""CPU: the nearest-row search's reference, cases, files and command line (tests/neighbors_cases.py, subgnn_amd/neighbors.py).
No GPU: the kernel itself is tests/test_gpu_neighbors.py's."""
import os
import re

import numpy as np
import pytest
import torch

import neighbors_cases as NC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def test_every_branch_of_the_dispatch_is_reached_by_some_case():
    reached = set()
    for c in NC.exact_cases() + NC.EDGE_CASES + [NC.RANDOM_CASE]:
        b = NC.branches(c['Q'], c['N'], c['D'], c['k'], c['splits'], c.get('exclude', False))
        assert b <= NC.ALL_BRANCHES, b - NC.ALL_BRANCHES
        reached |= b
    assert reached == NC.ALL_BRANCHES, NC.ALL_BRANCHES - reached


def test_the_cases_cover_every_listed_size():
    cs = NC.exact_cases()
    for name, values in (('Q', NC.QS), ('N', NC.NS), ('D', NC.DS), ('k', NC.KS), ('splits', NC.SPLITS)):
        assert set(values) <= {c[name] for c in cs}, name
    assert 30 <= 2 * len(cs) <= 80                                   # a few dozen launches, both metrics


def test_the_restated_geometry_agrees_with_the_librarys_workspace_query():
    from subgnn_amd import _lib
    lib = _lib.load()
    for c in NC.exact_cases() + NC.EDGE_CASES + [dict(Q=50000, N=50000, D=1, k=10, splits=0), dict(Q=1024, N=10 ** 6, D=1, k=10, splits=0),
                                                 dict(Q=1, N=50000, D=1, k=10, splits=0)]:
        nt, per, s = NC.geometry(c['Q'], c['N'], c['splits'])
        want = 0 if s == 1 else c['Q'] * s * c['k'] * 8
        assert lib.sgnn_topk_rows_workspace_bytes(c['Q'], c['N'], c['k'], c['splits']) == want, c
    assert lib.sgnn_topk_rows_workspace_bytes(4, 4, 65, 0) < 0 and lib.sgnn_topk_rows_workspace_bytes(4, 4, 0, 0) < 0
    assert lib.sgnn_topk_rows_workspace_bytes(0, 4, 1, 0) < 0 and lib.sgnn_topk_rows_workspace_bytes(4, 4, 1, 1025) < 0


def test_the_dyadic_cases_are_order_free():
    for c in NC.exact_cases():
        q, bank = NC.make_inputs(c)
        for x in (q, bank):
            m = x * 8
            assert x.dtype == np.float32 and np.array_equal(m, np.round(m)) and np.abs(m).max() <= 8
        fwd, rev = NC.dot_chain_f32(q, bank), NC.dot_chain_f32(q, bank, reverse=True)
        assert np.array_equal(fwd.view(np.uint32), rev.view(np.uint32)), c
        assert np.array_equal(fwd.astype(np.float64), q.astype(np.float64) @ bank.astype(np.float64).T), c     # every sum exact
        for x in (q, bank):
            assert np.array_equal(NC.aux_f32(x, 'l2').astype(np.float64), (x.astype(np.float64) ** 2).sum(1))
        s64 = NC.scores_f64(q, bank, 'l2')
        assert np.array_equal(NC.scores_f32(q, bank, 'l2').astype(np.float64), s64), c


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_reference_orders_ties_by_index_nan_last_and_fills():
    s = np.array([[1.0, 3.0, np.nan, 3.0, -np.inf, 1.0, -0.0, 0.0]], dtype=np.float32)
    sc, ix = NC.select(s, 8, 'dot')
    assert ix.tolist() == [[1, 3, 0, 5, 6, 7, 4, 2]]
    assert np.isnan(sc[0, 7]) and sc[0, 6] == -np.inf
    sc, ix = NC.select(s, 8, 'l2')
    assert ix.tolist() == [[4, 6, 7, 0, 5, 1, 3, 2]]
    sc, ix = NC.select(s, 10, 'dot', exclude=np.array([1]))
    assert ix.tolist() == [[3, 0, 5, 6, 7, 4, 2, -1, -1, -1]]
    assert np.all(sc[0, 7:] == -np.inf) and sc.dtype == np.float32
    sc, ix = NC.select(s[:, :0], 2, 'l2')
    assert ix.tolist() == [[-1, -1]] and np.all(sc == np.inf)
    sc, ix = NC.select(s, 3, 'dot', exclude=np.array([-1]))
    assert ix.tolist() == [[1, 3, 0]] and sc.tolist() == [[3.0, 3.0, 1.0]]


def test_reference_chain_is_the_float32_fma_chain():
    # 2^24 + 1 * 1 rounds back to 2^24 at every step of a float32 chain; float64 would keep the ones
    q = np.array([[2.0 ** 12, 1, 1, 1]], dtype=np.float32)
    b = np.array([[2.0 ** 12, 1, 1, 1]], dtype=np.float32)
    assert NC.dot_chain_f32(q, b)[0, 0] == np.float32(2.0 ** 24)
    assert NC.dot_chain_f32(q, b, reverse=True)[0, 0] == np.float32(2.0 ** 24 + 4)         # 3, then + 2^24 -> ties to even
    a = NC.topk_ref(q, b, 1, 'cosine')
    qa = NC.aux_f32(q, 'cosine')
    assert a[0][0, 0] == np.float32(np.float32(np.float32(2.0 ** 24) * qa[0]) * qa[0])


def test_tolerance_is_the_stated_bound():
    q = np.array([[1.0, -2.0, 0.5]], dtype=np.float32)
    b = np.array([[3.0, 1.0, -4.0]], dtype=np.float32)
    u = 2.0 ** -24
    g = 5 * u / (1 - 5 * u)
    assert NC.tolerance(q, b, 'dot')[0, 0] == g * 7.0
    assert np.isclose(NC.tolerance(q, b, 'cosine')[0, 0], g * 7.0 / np.sqrt(5.25 * 26.0), rtol=1e-12)
    assert np.isclose(NC.tolerance(q, b, 'l2')[0, 0], 2 * g * 7.0 + g * 2 * (5.25 + 26.0), rtol=1e-12)


# ---- the index and its files ---------------------------------------------------------------------------------------------------
def _index():
    from subgnn_amd.neighbors import SubgraphIndex
    E = torch.arange(12, dtype=torch.float32).view(4, 3) / 7
    return SubgraphIndex(E, [[5, 2, 9], [], [7], [1, 2]], [['a'], ['b', 'c d'], [], 'e'], ['train', 'train', 'val', 'test'],
                         [0, 1, 0, 0], 'l2', 'epoch=1.ckpt')


def test_index_round_trips_through_a_file(tmp_path):
    from subgnn_amd.neighbors import SubgraphIndex
    a = _index()
    assert a.labels == [['a'], ['b', 'c d'], [], ['e']] and len(a) == 4 and a.width == 3
    f = tmp_path / 'index.npz'
    a.save(f)
    assert os.listdir(tmp_path) == ['index.npz']                     # the temporary name is gone
    b = SubgraphIndex.load(f, 'cpu')
    assert torch.equal(a.embeddings, b.embeddings) and b.embeddings.dtype == torch.float32
    for name in ('subgraphs', 'labels', 'splits', 'rows', 'metric', 'checkpoint'):
        assert getattr(a, name) == getattr(b, name), name
    assert b.describe(1) == ('train', 1, [], ['b', 'c d'])
    a.save(f)                                                        # over an existing file
    assert SubgraphIndex.load(f).rows == a.rows
    with pytest.raises(ValueError):
        a.save(tmp_path / 'index.txt')


def test_index_from_embeddings_defaults_and_refusals(tmp_path):
    from subgnn_amd.neighbors import SubgraphIndex
    E = torch.zeros(3, 2)
    a = SubgraphIndex.from_embeddings(E)
    assert a.subgraphs == [[], [], []] and a.labels == [[], [], []] and a.rows == [0, 1, 2] and a.metric == 'cosine'
    assert a.checkpoint is None
    f = tmp_path / 'e.npz'
    a.save(f)
    b = SubgraphIndex.load(f)
    assert b.subgraphs == a.subgraphs and b.labels == a.labels and b.splits == ['', '', ''] and b.checkpoint is None
    empty = SubgraphIndex.from_embeddings(torch.zeros(0, 2), [], [])
    empty.save(f)
    assert len(SubgraphIndex.load(f)) == 0
    with pytest.raises(ValueError):
        SubgraphIndex.from_embeddings(E, subgraphs=[[1]])
    with pytest.raises(ValueError):
        SubgraphIndex.from_embeddings(E.double())
    with pytest.raises(ValueError):
        SubgraphIndex.from_embeddings(E, metric='manhattan')

    class _Lin:
        in_features = 5

    class _Model:
        lin = _Lin()

    class _P:
        model = _Model()
    a.save(f)
    with pytest.raises(ValueError, match='width 2'):
        SubgraphIndex.load(f, predictor=_P())
    _Lin.in_features = 2
    assert SubgraphIndex.load(f, predictor=_P()).width == 2


# ---- command line -------------------------------------------------------------------------------------------------------------
BASE = ['-config_path', 'c.json', '-restoreModelPath', 'run', '-subgraphs', 'req.txt', '-out', 'out.txt']


def test_cli_parser_defaults():
    from subgnn_amd import neighbors
    a = neighbors.parse_args(BASE)
    assert a.k == 10 and a.metric == 'cosine' and a.splits == ('train', 'val', 'test') and a.index is None and a.batch_size is None
    a = neighbors.parse_args(BASE + ['-k', '3', '-metric', 'l2', '-splits', 'val,train', '-index', 'i.npz', '-batch_size', '4'])
    assert (a.k, a.metric, a.splits, a.index, a.batch_size) == (3, 'l2', ('val', 'train'), 'i.npz', 4)


@pytest.mark.parametrize('extra', [['-k', '0'], ['-k', '-2'], ['-metric', 'manhattan'], ['-out', 'req.txt'], ['-splits', 'train,dev'],
                                   ['-index', 'out.txt'], ['-index', 'i.npy'], ['-batch_size', '0']])
def test_cli_parser_refuses(extra, capsys):
    from subgnn_amd import neighbors
    with pytest.raises(SystemExit):
        neighbors.parse_args(BASE + extra)
    capsys.readouterr()


def test_output_line_round_trips_a_float32():
    from subgnn_amd.neighbors import format_line
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.standard_normal(200).astype(np.float32), (rng.standard_normal(200) * 1e-20).astype(np.float32),
                           np.array([np.float32(1) - np.float32(2.0 ** -24), 1.0, 0.0, -np.inf, np.inf, 3.4028235e38], dtype=np.float32)])
    for i, v in enumerate(vals):
        line = format_line(i, 2, v, 'val', 7, [4, 0, 11], ['x', 'y'])
        cols = line.split('\t')
        assert len(cols) == 7 and cols[0] == str(i) and cols[1] == '2' and cols[3:] == ['val', '7', '4-0-11', 'x-y']
        assert np.float32(float(cols[2])).view(np.uint32) == v.view(np.uint32), (v, cols[2])
    assert format_line(0, 0, np.float32(-np.inf), '', -1, [], []).split('\t') == ['0', '0', '-inf', '', '-1', '', '']


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_symbols_and_says_what_they_replace():
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    for name in ('sgnn_topk_rows', 'sgnn_topk_rows_workspace_bytes', 'sgnn_topk_max_k'):
        assert re.search(r'\b%s\s*\(' % name, txt), name
    assert 'Replaces no reference function' in txt[txt.index('n1   Nearest rows'):txt.index('sgnn_topk_max_k')]
    from subgnn_amd import build, _lib
    assert 'neighbors.hip' in build.SOURCES
    for name in ('sgnn_topk_rows', 'sgnn_topk_rows_workspace_bytes', 'sgnn_topk_max_k'):
        assert name in _lib.SIGNATURES


def test_the_limit_of_k_comes_from_the_library():
    from subgnn_amd import ops, _lib
    assert ops.TOPK_MAX_K == _lib.load().sgnn_topk_max_k() == NC.MAX_K == 64
    x = torch.zeros(2, 3)
    with pytest.raises(ValueError, match='64'):
        ops.topk_rows(x, x, 65)
    with pytest.raises(ValueError):
        ops.topk_rows(x, x, 1)                                       # CPU tensors: there is no CPU path


def test_bad_arguments_are_refused_on_the_host():
    """No GPU is touched: the checks precede any launch (NULL pointers never reach one)."""
    from subgnn_amd import _lib
    lib = _lib.load()
    assert lib.sgnn_topk_rows(None, 4, 1, None, 4, 0, 4, 1, 0, None, None, None, 0, None, None, None, 0, None) == -1

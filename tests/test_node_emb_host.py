"""CPU: the node-embedding pre-training's host-side rules -- the reference's message direction, PyG's gcn_norm, AP, the file
names SubGNN reads -- and the resources of its kernels (no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nx_edges(path):
    import networkx as nx
    return set(nx.read_edgelist(str(path), nodetype=int).edges)


def _messy_edge_list(tmp_path):
    """Self loops, repeated edges (both orientations), ids whose first appearances are shuffled against their values."""
    r = np.random.RandomState(5)
    ids = r.permutation(200) * 3 + 7
    e = ids[r.randint(0, 200, size=(900, 2))]
    e = np.concatenate([e, e[:50, ::-1], e[50:60], np.stack([ids[:8], ids[:8]], 1)])
    e = e[r.permutation(len(e))]
    p = tmp_path / 'edge_list.txt'
    p.write_text(''.join('%d %d\n' % (a, b) for a, b in e))
    return p, e


def _write_golden_edges(tmp_path):
    e = load_golden('density')['edge_list']
    p = tmp_path / 'edge_list.txt'
    p.write_text(''.join('%d %d\n' % (a, b) for a, b in e))
    return p, e


@pytest.mark.parametrize('which', ['density', 'messy'])
def test_reference_direction_is_networkx_edges(which, tmp_path):
    from subgnn_amd import train_node_emb as TNE
    from subgnn_amd.graph import load_graph
    path, e = _write_golden_edges(tmp_path) if which == 'density' else _messy_edge_list(tmp_path)
    want = _nx_edges(path)
    got = set(map(tuple, TNE.reference_edges(e).tolist()))
    assert got == want
    # the rule as the trainer applies it to the loaded graph (node_pos, sorted rows): the positives of the link loss
    m = TNE.Messages(load_graph(path, torch.device('cpu')), 'gin')
    pos = set(zip((m.pos_u.numpy() - 1).tolist(), (m.pos_v.numpy() - 1).tolist()))
    assert pos == want and m.pos_u.numel() == len(want)


def _dense_reference(edges_nx, n, conv, direction):
    """float64 restatement of PyG's GINConv (eps 0) / GCNConv (gcn_norm, add_remaining_self_loops) operator over node ids
    0..n-1, messages source -> target: A[i, j] = weight of j's contribution to i."""
    src = np.array([a for a, b in edges_nx], dtype=np.int64)
    dst = np.array([b for a, b in edges_nx], dtype=np.int64)
    if direction == 'both':
        nl = src != dst
        src, dst = np.concatenate([src, dst[nl]]), np.concatenate([dst, src[nl]])
    A = np.zeros((n, n))
    if conv == 'gin':
        np.add.at(A, (dst, src), 1.0)
        return A + np.eye(n)
    keep = src != dst                                          # add_remaining_self_loops: drop loops, one loop of weight 1 each
    src, dst = np.concatenate([src[keep], np.arange(n)]), np.concatenate([dst[keep], np.arange(n)])
    deg = np.bincount(dst, minlength=n).astype(np.float64)    # at the target
    dinv = deg ** -0.5
    np.add.at(A, (dst, src), dinv[src] * dinv[dst])
    return A


@pytest.mark.parametrize('conv', ['gin', 'gcn'])
@pytest.mark.parametrize('direction', ['reference', 'both'])
@pytest.mark.parametrize('which', ['density', 'messy'])
def test_operator_matches_dense_restatement(conv, direction, which, tmp_path):
    from subgnn_amd import train_node_emb as TNE
    from subgnn_amd.graph import load_graph
    path, _ = _write_golden_edges(tmp_path) if which == 'density' else _messy_edge_list(tmp_path)
    g = load_graph(path, torch.device('cpu'))
    m = TNE.Messages(g, conv, direction)
    A = m.dense().numpy()[1:, 1:]
    want = _dense_reference(_nx_edges(path), g.max_id, conv, direction)
    # ids that are not nodes (the messy list skips most values): isolated rows -- GIN I, GCN 1 (its own loop)
    assert np.allclose(A, want, rtol=1e-6, atol=1e-7)
    # the transposed operator is the transpose
    n = m.bwd.n_rows
    rp, col = m.bwd.rowptr, m.bwd.col.long()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    B = torch.zeros(n, n, dtype=torch.float64)
    B.index_put_((rows, col), m.bwd.w.double() if m.bwd.w is not None else torch.ones(col.numel(), dtype=torch.float64),
                 accumulate=True)
    B += torch.diag(m.a_self.double())
    assert np.allclose(B.numpy()[1:, 1:], want.T, rtol=1e-6, atol=1e-7)


def test_chunk_plan_lists_every_long_row_in_order():
    from subgnn_amd import ops
    chunk = ops.NE_CHUNK()
    deg = torch.tensor([0, 3, chunk, chunk + 1, 0, 4 * chunk + 7, 2])
    rowptr = torch.zeros(len(deg) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    csr = ops.MessageCSR(rowptr, torch.zeros(int(rowptr[-1]), dtype=torch.int32), None, torch.ones(len(deg)))
    assert csr.long_rows.tolist() == [3, 5]
    assert csr.chunk_first.tolist() == [0, 2, 7]
    assert csr.chunk_row.tolist() == [3, 3, 5, 5, 5, 5, 5]
    b3, b5 = int(rowptr[3]), int(rowptr[5])
    assert csr.chunk_beg.tolist() == [b3, b3 + chunk] + [b5 + k * chunk for k in range(5)]


def test_average_precision_matches_sklearn():
    from sklearn.metrics import average_precision_score
    from subgnn_amd.subgraph_utils import average_precision
    r = np.random.RandomState(3)
    for n, ties in ((50, False), (400, True), (1000, True)):
        y = r.rand(n) < 0.3
        s = np.round(r.rand(n), 1 if ties else 9)
        assert abs(average_precision(y, s) - average_precision_score(y, s)) < 1e-12


def test_metrics_of_a_scored_set():
    from sklearn.metrics import roc_auc_score, average_precision_score, accuracy_score, f1_score
    from subgnn_amd.train_node_emb import link_metrics
    r = np.random.RandomState(4)
    s = torch.from_numpy(r.rand(300).astype(np.float32))
    y = np.zeros(300, bool)
    y[:120] = True
    m = link_metrics(s, 120)
    sd = s.double().numpy()
    assert abs(m['roc'] - roc_auc_score(y, sd)) < 1e-12 and abs(m['ap'] - average_precision_score(y, sd)) < 1e-12
    assert m['acc'] == accuracy_score(y, sd > 0.5) and abs(m['f1'] - f1_score(y, sd > 0.5)) < 1e-12


@pytest.mark.parametrize('conv,etype', [('gin', 'gin'), ('gcn', 'graphsaint')])
def test_written_names_are_the_ones_subgnn_reads(conv, etype):
    from subgnn_amd.SubGNN import dataset_paths
    from subgnn_amd.train_node_emb import FILE_NAMES
    assert os.path.basename(dataset_paths('ds', etype)['embedding_path']) == FILE_NAMES[conv]


def test_edge_split_is_a_partition_of_80_10_10():
    from subgnn_amd.train_node_emb import edge_split
    tr, va, te = edge_split(1003, 7)
    assert (len(tr), len(va), len(te)) == (802, 100, 101)
    assert sorted(np.concatenate([tr, va, te]).tolist()) == list(range(1003))
    assert all(np.array_equal(a, b) for a, b in zip(edge_split(1003, 7), (tr, va, te)))
    assert not np.array_equal(edge_split(1003, 8)[0], tr)


def test_node_emb_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_resources as KR
    from subgnn_amd import build
    build.build(verbose=False)
    ks = [k for o in ('node_emb.o', 'optim.o') for k in KR.kernels(os.path.join(build.LIBDIR, o))
          if k['demangled'].startswith(('ne_', 'void ne_', 'void adam_step_kernel'))]
    names = ' '.join(k['demangled'] for k in ks)
    for want in ('ne_aggregate_kernel', 'ne_aggregate_finish_kernel', 'ne_negatives_kernel', 'ne_link_loss_kernel',
                 'ne_loss_finish_kernel', 'ne_relu_drop_bwd_kernel', 'adam_step_kernel<true>', 'adam_step_kernel<false>'):
        assert want in names, want
    for k in ks:
        assert k['private_segment_fixed_size'] == 0, k['demangled'][:80]
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k['demangled'][:80]

"""-m gpu: node-embedding pre-training (train_node_emb.py) -- the graph-convolution aggregation forward and transposed backward,
the draw-tape dropout and negatives, the link loss, Adam with coupled L2 and one whole training step against float64
restatements, reproducibility, and a pre-trained table read by the SubGNN driver."""
import json

import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _hub_graph():
    """~3000 ids, some never used (isolated rows), self loops, and two hubs of 2100 neighbours (> 4 chunks of 512): hub 0
    appears first (its neighbours all come later: a long TRANSPOSED row in the reference direction), hub 1 last (a long
    forward row)."""
    from subgnn_amd.graph import networkx_order_csr
    from subgnn_amd.ops import DeviceGraph
    r = np.random.RandomState(11)
    ids = np.setdiff1d(np.arange(2, 3200), r.choice(np.arange(2, 3200), 150, replace=False))
    e = ids[r.randint(0, len(ids), size=(9000, 2))]
    loops = np.stack([ids[:40], ids[:40]], 1)
    h0 = np.stack([np.zeros(2100, np.int64), r.choice(ids, 2100, replace=False)], 1)
    h1 = np.stack([r.choice(ids, 2100, replace=False), np.ones(2100, np.int64)], 1)
    edges = np.concatenate([h0, e, loops, h1])
    rowptr, col, order = networkx_order_csr(edges)
    return DeviceGraph(rowptr, col, order, DEV), edges


_G = {}


def hub_graph():
    if 'g' not in _G:
        _G['g'] = _hub_graph()
    return _G['g']


def _sparse(csr, a_self, transpose=False):
    n = csr.n_rows
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), csr.rowptr[1:] - csr.rowptr[:-1])
    col = csr.col.long()
    w = csr.w.double() if csr.w is not None else torch.ones(col.numel(), dtype=torch.float64, device=DEV)
    d = torch.arange(n, device=DEV)
    idx = torch.stack([torch.cat([rows, d]), torch.cat([col, d])])
    if transpose:
        idx = idx.flip(0)
    return torch.sparse_coo_tensor(idx, torch.cat([w, a_self.double()]), (n, n)).coalesce()


@pytest.mark.parametrize('F', [32, 64, 128, 256])
@pytest.mark.parametrize('conv', ['gin', 'gcn'])
@pytest.mark.parametrize('direction', ['reference', 'both'])
def test_aggregate_forward_and_transposed_backward(F, conv, direction):
    from subgnn_amd import ops
    from subgnn_amd.train_node_emb import Messages
    g, _ = hub_graph()
    m = Messages(g, conv, direction)
    if direction == 'reference':
        assert m.fwd.max_row > 4 * ops.NE_CHUNK() and m.bwd.max_row > 4 * ops.NE_CHUNK()
    gen = torch.Generator(device=DEV).manual_seed(F)
    X = torch.randn(m.fwd.n_rows, F, generator=gen, device=DEV)
    b = torch.randn(F, generator=gen, device=DEV)
    A = _sparse(m.fwd, m.a_self)
    out = ops.ne_aggregate(m.fwd, X, b)
    assert_close(out, torch.sparse.mm(A, X.double()) + b.double(), 'forward F=%d %s %s' % (F, conv, direction))
    assert torch.equal(out, ops.ne_aggregate(m.fwd, X, b))
    dX = ops.ne_aggregate(m.bwd, X)
    assert_close(dX, torch.sparse.mm(_sparse(m.fwd, m.a_self, transpose=True), X.double()), 'backward F=%d' % F)
    assert torch.equal(dX, ops.ne_aggregate(m.bwd, X))


def test_aggregate_at_benchmark_scale():
    from subgnn_amd import ops, synthetic
    from subgnn_amd.train_node_emb import Messages
    g = ops.DeviceGraph.from_device_csr(*synthetic.barabasi_albert_csr_device(1_000_000, 10, 5, DEV))
    m = Messages(g, 'gcn')
    assert m.bwd.n_chunks > 0
    X = torch.randn(m.fwd.n_rows, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    out = ops.ne_aggregate(m.fwd, X)
    assert_close(out, torch.sparse.mm(_sparse(m.fwd, m.a_self), X.double()), 'forward 1M')
    dX = ops.ne_aggregate(m.bwd, X)
    assert_close(dX, torch.sparse.mm(_sparse(m.fwd, m.a_self, transpose=True), X.double()), 'backward 1M')
    assert torch.equal(dX, ops.ne_aggregate(m.bwd, X))


def test_dropout_mask_is_the_draw_tape():
    from oracle.tape import draw64_np
    from subgnn_amd import ops
    from subgnn_amd.train_node_emb import Messages
    g, _ = hub_graph()
    m = Messages(g, 'gin')
    X = torch.rand(m.fwd.n_rows, 64, device=DEV) + 0.1                    # positive: relu passes everything
    p, seed, sid = 0.4, 77, (12 << 32) | 5
    out = ops.ne_aggregate(m.fwd, X, relu=True, dropout=p, seed=seed, stream_id=sid)
    plain = ops.ne_aggregate(m.fwd, X)
    n = m.fwd.n_rows
    v, f = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(64, dtype=np.uint64), indexing='ij')
    keep = (draw64_np(seed, sid, v, f) >> np.uint64(32)) >= np.uint64(ops.dropout_threshold(p))
    keep_t = torch.from_numpy(keep).to(DEV)
    assert torch.equal(out[1:] != 0, keep_t[1:])
    assert_close(out[1:][keep_t[1:]], plain[1:][keep_t[1:]].double() / (1 - p), 'kept values')
    assert 0.55 < keep.mean() < 0.65


def test_negatives_match_the_host_twin():
    from oracle.tape import draw64
    from subgnn_amd import ops
    g, edges = hub_graph()
    n, seed, sid = 3000, 9, (11 << 32) | (1 << 24)
    u, v = ops.ne_negatives(g, n, seed, sid, item_base=17)
    rp, cs = g.rowptr.cpu().numpy(), g.col_sorted.cpu().numpy()
    adj = set()
    for a in range(g.max_id + 1):
        for b in cs[rp[a]:rp[a + 1]]:
            adj.add((a, int(b)))
    N = g.max_id
    want_u, want_v = [], []
    for i in range(n):
        ru = rv = 0
        for att in range(64):
            d = draw64(seed, sid, 17 + i, att)
            a = 1 + (((d >> 32) * N) >> 32)
            b = 1 + (((d & 0xFFFFFFFF) * N) >> 32)
            if a != b and (a, b) not in adj:
                ru, rv = a, b
                break
        want_u.append(ru)
        want_v.append(rv)
    assert u.cpu().tolist() == want_u and v.cpu().tolist() == want_v
    e1 = set(map(tuple, (edges + 1).tolist()))
    for a, b in zip(want_u, want_v):
        assert a != b and a != 0 and (a, b) not in e1 and (b, a) not in e1


def _ref_loss(Z, pu, pv, n_pos):
    """utils.el_dot + calc_loss_both literally, in float64 (without the detach)."""
    dots = (Z[pu] * Z[pv]).sum(1)
    s = torch.sigmoid(dots)
    pred = torch.stack((1 - s, s), 1)
    y = torch.zeros(len(pu), dtype=torch.long, device=Z.device)
    y[:n_pos] = 1
    return torch.nn.functional.nll_loss(torch.nn.functional.log_softmax(pred, dim=-1), y), s


@pytest.mark.parametrize('F', [32, 64, 256])
def test_link_loss_and_gradient(F):
    from subgnn_amd import ops
    N = 5000
    gen = torch.Generator(device=DEV).manual_seed(F)
    Z = torch.randn(N + 1, F, device=DEV, generator=gen) * (2.0 / F ** 0.5)
    pu = torch.randint(1, N + 1, (4000,), device=DEV, generator=gen, dtype=torch.int32)
    pv = torch.randint(1, N + 1, (4000,), device=DEV, generator=gen, dtype=torch.int32)
    nu = torch.randint(1, N + 1, (1000,), device=DEV, generator=gen, dtype=torch.int32)
    nv = torch.randint(1, N + 1, (1000,), device=DEV, generator=gen, dtype=torch.int32)
    Zg = Z.clone().requires_grad_(True)
    pre = ops.sort_edges_by_key(torch.cat([pu, pv]), N)
    loss, s = ops.link_loss(Zg, pu, pv, nu, nv, pos_sorted=pre)
    (loss * 3.0).backward()
    Zr = Z.double().requires_grad_(True)
    rl, rs = _ref_loss(Zr, torch.cat([pu, nu]).long(), torch.cat([pv, nv]).long(), 4000)
    (rl * 3.0).backward()
    assert_close(loss, rl.detach(), 'loss')
    assert_close(s, rs.detach(), 's')
    assert_close(Zg.grad, Zr.grad, 'dZ')


@pytest.mark.parametrize('n', [10008, 10007])
@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('wd', [0.0, 5e-4])
def test_adam_step_matches_torch(wd, scaled, n):
    """ops.adam_step (sgnn_adam_step) == torch.optim.Adam(weight_decay = wd) over five steps, in both gradient forms: coupled
    L2 (the node-embedding trainer) and the gradient times a device scalar (dist.ShardedTableAdam's clip coefficient; torch
    gets the gradient multiplied first), on a length that is a multiple of 4 and on one that is not.  Both forms at once are
    refused."""
    from subgnn_amd import ops, _lib
    gen = torch.Generator(device=DEV).manual_seed(2)
    p0 = torch.randn(n, device=DEV, generator=gen)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=5e-3, weight_decay=wd)
    scale = torch.full((1,), 0.37, device=DEV) if scaled else None
    if scaled and wd:
        with pytest.raises(_lib.SubgnnHipError):
            ops.adam_step(p, torch.zeros_like(p), m, v, 5e-3, (0.9, 0.999), 1e-8, 1, grad_scale=scale, weight_decay=wd)
        assert torch.equal(p, p0)
        return
    for t in range(1, 6):
        grad = torch.randn(n, device=DEV, generator=gen) * 0.01
        ops.adam_step(p, grad, m, v, 5e-3, (0.9, 0.999), 1e-8, t, grad_scale=scale, weight_decay=wd)
        q.grad = grad * scale if scaled else grad.clone()
        opt.step()
    assert_close(p, q.detach(), 'Adam(weight_decay=%g, scaled=%s, n=%d)' % (wd, scaled, n), tol=1e-5)


@pytest.mark.parametrize('hidden, output', [(64, 32), (260, 20), (512, 100)])     # (the ragged and <64, 2> forms in one step)
@pytest.mark.parametrize('conv', ['gin', 'gcn'])
@pytest.mark.parametrize('direction', ['reference', 'both'])
def test_one_training_step_against_float64(conv, direction, hidden, output):
    from oracle.tape import draw64_np
    from subgnn_amd import ops, tape
    from subgnn_amd.train_node_emb import Messages, Trainer, edge_split, BETAS, ADAM_EPS
    g, _ = hub_graph()
    m = Messages(g, conv, direction)
    tr = Trainer(g, m, edge_split(m.pos_u.numel(), 3), conv, hidden, output, 1e-3, 5e-4, 0.4, 3)
    p0 = [p.detach().double().clone() for p in tr.params]
    tr.step(0)
    grads = [p.grad.detach() for p in tr.params]
    nu, nv = tr.last_negatives
    # float64 replica given the same negatives and masks
    A = _sparse(m.fwd, m.a_self).to_dense()
    n, hid = A.shape[0], hidden
    v, f = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(hid, dtype=np.uint64), indexing='ij')
    keep = (draw64_np(3, tr.stream(tape.STREAM_NE_DROP, epoch=0), v, f) >> np.uint64(32)) >= np.uint64(ops.dropout_threshold(0.4))
    mask = torch.from_numpy(keep).to(DEV).double() / 0.6
    P = [p.clone().requires_grad_(True) for p in p0]
    T, b1, W2, b2 = P
    H = torch.relu(A @ T + b1) * mask
    Z = A @ (H @ W2.t()) + b2
    pu = torch.cat([tr.train_u, nu]).long()
    pv = torch.cat([tr.train_v, nv]).long()
    loss, _ = _ref_loss(Z, pu, pv, tr.train_u.numel())
    loss.backward()
    for k, (gp, rp) in enumerate(zip(grads, P)):
        assert_close(gp, rp.grad, 'grad %d' % k)
    for k, (p, rp, q0) in enumerate(zip(tr.params, P, p0)):
        gt = rp.grad + 5e-4 * q0
        mm, vv = (1 - BETAS[0]) * gt, (1 - BETAS[1]) * gt * gt
        want = q0 - 1e-3 / (1 - BETAS[0]) * mm / (vv.sqrt() / (1 - BETAS[1]) ** 0.5 + ADAM_EPS)
        # an element whose gradient is zero up to rounding may step either way: judged by its gradient above
        firm = gt.abs() > 1e-5 * gt.abs().max()
        assert firm.float().mean() > 0.5
        assert_close(p.detach()[firm], want.detach()[firm], 'param %d after Adam' % k)


def test_two_runs_write_identical_tables():
    from subgnn_amd.train_node_emb import train
    g, _ = hub_graph()
    a = train(g, 'gcn', epochs=5, seed=4, hidden=64, output=32)
    b = train(g, 'gcn', epochs=5, seed=4, hidden=64, output=32)
    assert a['embeddings'].shape == (g.max_id, 32)
    assert torch.equal(a['embeddings'], b['embeddings'])
    assert [h['loss'] for h in a['history']] == [h['loss'] for h in b['history']]


def test_density_dataset_pretrained_and_read_by_the_driver(tiny, tmp_path):
    from test_gpu_train_driver import CONFIG
    from subgnn_amd import config, train_config, prepare_dataset as pd, precompute_graph_metrics as pgm
    from subgnn_amd.graph import load_graph
    from subgnn_amd.train_node_emb import train
    out, info = pd.write_dataset(tmp_path / 'ds', 'density', seed=9, embed_dim=16, embeddings='gin', n=400, m=3,
                                 n_subgraphs=40, n_subgraph_nodes=8, n_bins=3)
    table = torch.load(out / 'gin_embeddings.pth')
    assert table.shape == (info['n_nodes'], 16) and torch.isfinite(table).all()
    rec = json.loads((out / 'node_emb.json').read_text())
    assert len(rec['history']) == 100 and rec['hparams']['output'] == 16
    g = load_graph(out / 'edge_list.txt', DEV)
    trained = train(g, epochs=100, seed=9, output=16)
    untrained = train(g, epochs=0, seed=9, output=16)
    assert trained['test']['roc'] > untrained['test']['roc']
    assert torch.equal(trained['embeddings'].cpu(), table)
    pgm.calculate_stats(out)
    fix = dict(tiny.hp)
    for k in ('batch_size', 'learning_rate', 'n_layers'):
        fix.pop(k, None)
    fix.update({'max_epochs': 1, 'seed': 1, 'lin_dropout': 0.0, 'compute_similarities': True, 'node_embed_size': 16})
    cfg = tmp_path / 'config.json'
    cfg.write_text(CONFIG % json.dumps(fix))
    config.PROJECT_ROOT = tmp_path
    best, model, trainer = train_config.train_model(train_config.read_json(cfg), log=lambda *a: None)
    assert model.hparams['node_embed_size'] == 16 and torch.isfinite(torch.tensor(trainer.history[0]['train_loss']))

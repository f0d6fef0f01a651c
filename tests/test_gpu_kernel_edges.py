"""-m gpu: the node-embedding kernels (csrc/node_emb.hip) and the clip + Adam tail (csrc/optim.hip) at the widths, lengths
and inputs the trainer's default shapes never reach -- every <L, C> form of the aggregation and the link loss with ragged
widths, rows at the chunk boundary, the loss grid's second sweep, saturated dots, self pairs, the negative sampler running
out of draws, non-finite gradients, launch-group and size edges of the optimizer tail -- each against a float64 restatement
or torch itself."""
import contextlib

import numpy as np
import pytest
import torch

from helpers import assert_close
from test_gpu_node_emb import _ref_loss, _sparse, hub_graph

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

WIDTHS = [4, 20, 36, 100, 132, 260, 512]       # <8,1> .. <64,2>; all but 4, 36 and 512 leave lanes of the last float4 group idle


@contextlib.contextmanager
def _nan_buffers(monkeypatch):
    """Every float buffer the ops allocate inside the block starts as NaN instead of whatever the allocator hands back (often
    the previous call's correct result): an output row or a pair the kernel fails to write then shows."""
    empty, empty_like, full, full_like = torch.empty, torch.empty_like, torch.full, torch.full_like

    def nan_empty(*size, dtype=None, device=None, **kw):
        if dtype is not None and not dtype.is_floating_point:
            return empty(*size, dtype=dtype, device=device, **kw)
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        return full(shape, float('nan'), dtype=dtype, device=device, **kw)

    def nan_empty_like(t, **kw):
        return full_like(t, float('nan'), **kw) if (kw.get('dtype') or t.dtype).is_floating_point else empty_like(t, **kw)
    with monkeypatch.context() as m:
        m.setattr(torch, 'empty', nan_empty)
        m.setattr(torch, 'empty_like', nan_empty_like)
        yield


def _keep_mask(n, F, p, seed, sid):
    from oracle.tape import draw64_np
    from subgnn_amd import ops
    v, f = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(F, dtype=np.uint64), indexing='ij')
    keep = (draw64_np(seed, sid, v, f) >> np.uint64(32)) >= np.uint64(ops.dropout_threshold(p))
    return torch.from_numpy(keep).to(DEV)


# ---- A1: every <L, C> instantiation at ragged widths ----------------------------------------------------------------------

@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('conv', ['gin', 'gcn'])
@pytest.mark.parametrize('direction', ['reference', 'both'])
def test_aggregate_every_width_with_epilogue(F, conv, direction, monkeypatch):
    """Forward with bias, relu and dropout and the transposed backward on the hub graph at widths that run every dispatch form
    and leave idle lanes (F = 20: 5 of 8 float4 lanes; 260: the second float4 of one lane of 64 in <64, 2>): values against
    the float64 sparse product, the kept elements against the draw tape for every f < F, bit-repeatable."""
    from subgnn_amd import ops
    from subgnn_amd.train_node_emb import Messages
    g, _ = hub_graph()
    m = Messages(g, conv, direction)
    gen = torch.Generator(device=DEV).manual_seed(1000 + F)
    X = torch.randn(m.fwd.n_rows, F, generator=gen, device=DEV)
    b = torch.randn(F, generator=gen, device=DEV)
    p, seed, sid = 0.4, 5 + F, (3 << 32) | F
    with _nan_buffers(monkeypatch):
        out = ops.ne_aggregate(m.fwd, X, b, relu=True, dropout=p, seed=seed, stream_id=sid)
        plain = ops.ne_aggregate(m.fwd, X, b)
        dX = ops.ne_aggregate(m.bwd, X)
    keep = _keep_mask(m.fwd.n_rows, F, p, seed, sid)
    pre = torch.sparse.mm(_sparse(m.fwd, m.a_self), X.double()) + b.double()
    assert_close(plain, pre, 'forward F=%d %s %s' % (F, conv, direction))
    assert_close(out, torch.relu(pre) * keep / (1 - p), 'relu + dropout F=%d %s %s' % (F, conv, direction))
    # the same additions decide relu: an element is non-zero iff it is kept and its (kernel) pre-activation is positive
    assert torch.equal(out != 0, keep & (plain > 0))
    assert_close(dX, torch.sparse.mm(_sparse(m.fwd, m.a_self, transpose=True), X.double()), 'backward F=%d' % F)
    assert torch.equal(out, ops.ne_aggregate(m.fwd, X, b, relu=True, dropout=p, seed=seed, stream_id=sid))
    assert torch.equal(dX, ops.ne_aggregate(m.bwd, X))


@pytest.mark.parametrize('F', [2, 6, 516])
def test_aggregate_refuses_unsupported_widths(F):
    """F not a multiple of 4, or above 512: SGNN_ERR_UNSUPPORTED_D before anything is launched -- the output is not touched."""
    from subgnn_amd import ops, _lib
    from subgnn_amd.ops import _ptr
    from subgnn_amd.train_node_emb import Messages
    g, _ = hub_graph()
    m = Messages(g, 'gcn')
    X = torch.randn(m.fwd.n_rows, F, device=DEV)
    with pytest.raises(_lib.SubgnnHipError, match='SGNN_ERR_UNSUPPORTED_D'):
        ops.ne_aggregate(m.fwd, X)
    c = m.fwd
    out = torch.full_like(X, 7.0)
    partial = torch.zeros(max(c.n_chunks, 1) * F, device=DEV)
    rc = _lib.load().sgnn_ne_aggregate(_ptr(c.rowptr), _ptr(c.col), _ptr(c.w), _ptr(c.a_self), _ptr(X), None, c.n_rows, F,
                                       _ptr(c.chunk_row), _ptr(c.chunk_beg), c.n_chunks, _ptr(c.long_rows), _ptr(c.chunk_first),
                                       c.long_rows.numel(), 0, 0, 1.0, 0, 0, _ptr(out), _ptr(partial), None)
    torch.cuda.synchronize()
    assert rc == -5 and bool((out == 7.0).all()) and bool((partial == 0).all())


# ---- A2: rows at the chunk boundary ---------------------------------------------------------------------------------------

HUBS = (511, 512, 513, 1024, 1025, 1537)


def _star_graph():
    """Six star hubs with exactly HUBS leaves of their own, each hub first in the file: in the reference direction every edge
    runs hub -> leaf, so the long rows are the TRANSPOSED graph's; in 'both' they are forward rows too.  Ids are taken from a
    range with gaps, so some rows are isolated."""
    from subgnn_amd.graph import networkx_order_csr
    from subgnn_amd.ops import DeviceGraph
    r = np.random.RandomState(3)
    pool = np.setdiff1d(np.arange(sum(HUBS) + len(HUBS) + 300), r.choice(np.arange(1, sum(HUBS)), 300, replace=False))
    edges, k = [], 0
    for n in HUBS:
        hub, leaves = pool[k], pool[k + 1:k + 1 + n]
        edges.append(np.stack([np.full(n, hub), leaves], 1))
        k += n + 1
    edges = np.concatenate(edges)
    rowptr, col, order = networkx_order_csr(edges)
    return DeviceGraph(rowptr, col, order, DEV)


def _row_lengths(csr):
    return (csr.rowptr[1:] - csr.rowptr[:-1]).cpu().numpy()


@pytest.mark.parametrize('F', [20, 260])
@pytest.mark.parametrize('conv', ['gin', 'gcn'])
@pytest.mark.parametrize('direction', ['reference', 'both'])
def test_aggregate_rows_at_the_chunk_boundary(F, conv, direction, monkeypatch):
    """Rows of 511 and 512 entries stay whole, 513 and 1024 take two chunks, 1025 three and 1537 four (the last one chunk of a
    single entry): the plan of MessageCSR, and forward and backward against the float64 sparse product."""
    from subgnn_amd import ops
    from subgnn_amd.train_node_emb import Messages
    assert ops.NE_CHUNK() == 512
    g = _star_graph()
    m = Messages(g, conv, direction)
    longs = m.bwd if direction == 'reference' else m.fwd
    lens = _row_lengths(longs)
    assert set(HUBS) <= set(lens.tolist()) and int((lens == 0).sum()) > 300
    if direction == 'reference':
        assert m.fwd.max_row == 1 and m.fwd.n_chunks == 0
    rows = longs.long_rows.cpu().numpy()
    first = longs.chunk_first.cpu().numpy()
    beg = longs.chunk_beg.cpu().numpy()
    rp = longs.rowptr.cpu().numpy()
    assert sorted(lens[rows].tolist()) == [513, 1024, 1025, 1537]
    for i, r in enumerate(rows):
        n = int(first[i + 1] - first[i])
        assert n == {513: 2, 1024: 2, 1025: 3, 1537: 4}[int(lens[r])]
        assert (beg[first[i]:first[i + 1]] == rp[r] + 512 * np.arange(n)).all()
        assert (longs.chunk_row[first[i]:first[i + 1]] == int(r)).all()
    gen = torch.Generator(device=DEV).manual_seed(F)
    X = torch.randn(m.fwd.n_rows, F, generator=gen, device=DEV)
    b = torch.randn(F, generator=gen, device=DEV)
    with _nan_buffers(monkeypatch):
        out = ops.ne_aggregate(m.fwd, X, b)
        dX = ops.ne_aggregate(m.bwd, X)
    assert_close(out, torch.sparse.mm(_sparse(m.fwd, m.a_self), X.double()) + b.double(), 'forward F=%d' % F)
    assert_close(dX, torch.sparse.mm(_sparse(m.fwd, m.a_self, transpose=True), X.double()), 'backward F=%d' % F)
    assert torch.equal(dX, ops.ne_aggregate(m.bwd, X))


# ---- A3: graph_conv as an autograd op -------------------------------------------------------------------------------------

@pytest.mark.parametrize('F', [20, 260])
@pytest.mark.parametrize('dropout', [0.0, 0.4])
def test_graph_conv_autograd_against_float64(F, dropout, monkeypatch):
    """out, dX and dbias of ops.graph_conv (relu [-> dropout]) against float64 autograd of relu(A X + b) * mask / (1 - p).
    GIN on the hub graph with X and b on a 1/8 grid: every sum is exact in float32, so both sides take the same relu
    decisions, and the zero rows of X (among them the isolated ones) meet zero bias entries -- pre-activations of exactly 0,
    where the kernel's "out > 0" rule must agree with torch's relu gradient (0)."""
    from subgnn_amd import ops
    from subgnn_amd.train_node_emb import Messages
    g, _ = hub_graph()
    m = Messages(g, 'gin', 'both')
    n = m.fwd.n_rows
    gen = torch.Generator(device=DEV).manual_seed(F)
    X = torch.randint(-8, 9, (n, F), generator=gen, device=DEV).float() / 8
    lens = torch.from_numpy(_row_lengths(m.fwd)).to(DEV)
    zero_rows = (lens == 0) | (torch.rand(n, generator=gen, device=DEV) < 0.05)
    X[zero_rows] = 0
    b = torch.randint(-4, 5, (F,), generator=gen, device=DEV).float() / 8
    b[::3] = 0
    G = torch.randn(n, F, generator=gen, device=DEV)
    seed, sid = 21, (7 << 32) | F
    Xg, bg = X.clone().requires_grad_(True), b.clone().requires_grad_(True)
    with _nan_buffers(monkeypatch):
        out = ops.graph_conv(Xg, bg, m.fwd, m.bwd, relu=True, dropout=dropout, seed=seed, stream_id=sid)
        (out * G).sum().backward()
    A = _sparse(m.fwd, m.a_self)
    Xr, br = X.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = torch.sparse.mm(A, Xr) + br
    assert int((pre.detach() == 0).sum()) > 100
    want = torch.relu(pre)
    if dropout:
        want = want * _keep_mask(n, F, dropout, seed, sid) / (1 - dropout)
    (want * G.double()).sum().backward()
    assert_close(out, want.detach(), 'graph_conv out F=%d p=%g' % (F, dropout))
    assert_close(Xg.grad, Xr.grad, 'graph_conv dX F=%d p=%g' % (F, dropout))
    assert_close(bg.grad, br.grad, 'graph_conv dbias F=%d p=%g' % (F, dropout))
    with pytest.raises(ValueError, match='relu'):
        ops.graph_conv(Xg, bg, m.fwd, m.bwd, relu=False, dropout=0.4)


# ---- A4: the link loss ------------------------------------------------------------------------------------------------------

def _ref_dots(d, n_pos):
    """_ref_loss on the dots: float64 loss, s and d loss / d dot."""
    d = d.double().detach().requires_grad_(True)
    s = torch.sigmoid(d)
    y = torch.zeros(d.numel(), dtype=torch.long, device=d.device)
    y[:n_pos] = 1
    loss = torch.nn.functional.nll_loss(torch.nn.functional.log_softmax(torch.stack((1 - s, s), 1), dim=-1), y)
    loss.backward()
    return loss.detach(), s.detach(), d.grad


def _check_link_loss(Z, pu, pv, n_pos, what, monkeypatch):
    from subgnn_amd import ops
    with _nan_buffers(monkeypatch):
        loss, s, gd = ops.ne_link_loss(Z, pu, pv, n_pos)
    d = (Z.double()[pu.long()] * Z.double()[pv.long()]).sum(1)
    rl, rs, rg = _ref_dots(d, n_pos)
    assert_close(loss, rl.view(1), what + ' loss')
    assert_close(s, rs, what + ' s')
    assert_close(gd, rg, what + ' d loss / d dot')
    l2, s2, g2 = ops.ne_link_loss(Z, pu, pv, n_pos)
    assert torch.equal(loss, l2) and torch.equal(s, s2) and torch.equal(gd, g2)
    return d


@pytest.mark.parametrize('F, P', [(20, 5000), (132, 5000), (260, 5000), (512, 5000), (20, 300_000), (512, 40_000)])
def test_link_loss_widths_and_grid_sweeps(F, P, monkeypatch):
    """Every dispatch form with idle lanes, and more pairs than one sweep of the capped grid covers (4096 blocks of 32 pairs
    at F <= 32, of 4 pairs at F > 256): 300 000 pairs at F = 20 and 40 000 at F = 512 make every block loop three times."""
    N = 6000
    gen = torch.Generator(device=DEV).manual_seed(F + P)
    Z = torch.randn(N + 1, F, device=DEV, generator=gen) * (2.0 / F ** 0.5)
    pu = torch.randint(1, N + 1, (P,), device=DEV, generator=gen, dtype=torch.int32)
    pv = torch.randint(1, N + 1, (P,), device=DEV, generator=gen, dtype=torch.int32)
    _check_link_loss(Z, pu, pv, P * 4 // 5, 'F=%d P=%d' % (F, P), monkeypatch)


@pytest.mark.parametrize('F', [20, 260])
@pytest.mark.parametrize('case', ['no positives', 'all positives', 'one pair', 'saturated'])
def test_link_loss_label_counts_and_saturated_dots(F, case, monkeypatch):
    """n_pos = 0, n_pos = n_pairs, a single pair, and dots spread over about +-40, where s rounds to 1 (or to a tiny
    number): the gradient's s (1 - s) is sigmoid(d) sigmoid(-d) there, not s times a 1 - s rounded to 0."""
    N, P = 3000, 20000
    gen = torch.Generator(device=DEV).manual_seed(F)
    scale = (2.0 / F ** 0.5) if case != 'saturated' else (15.0 / F ** 0.5) ** 0.5
    Z = torch.randn(N + 1, F, device=DEV, generator=gen) * scale
    if case == 'one pair':
        P = 1
    pu = torch.randint(1, N + 1, (P,), device=DEV, generator=gen, dtype=torch.int32)
    pv = torch.randint(1, N + 1, (P,), device=DEV, generator=gen, dtype=torch.int32)
    n_pos = {'no positives': 0, 'all positives': P, 'one pair': 1, 'saturated': P // 2}[case]
    d = _check_link_loss(Z, pu, pv, n_pos, '%s F=%d' % (case, F), monkeypatch)
    if case == 'saturated':
        assert float(d.abs().max()) > 40 and float((d.abs() > 17).double().mean()) > 0.1      # s rounds to 1 above ~17
    if case == 'one pair':
        _check_link_loss(Z, pu, pv, 0, 'one negative pair F=%d' % F, monkeypatch)


@pytest.mark.parametrize('F', [20, 260, 512])
def test_link_loss_self_and_duplicated_pairs(F):
    """ops.link_loss with positives that repeat and that include u == v self pairs (the trainer's positives hold every self
    loop): dZ[u] then gets both terms, 2 g Z[u]; against float64 autograd of _ref_loss.  F above 256 is scattered in column
    blocks (the row scatter's widest form is 256)."""
    from subgnn_amd import ops
    N = 2000
    gen = torch.Generator(device=DEV).manual_seed(F)
    Z = torch.randn(N + 1, F, device=DEV, generator=gen) * (1.5 / F ** 0.5)
    pu = torch.randint(1, N + 1, (3000,), device=DEV, generator=gen, dtype=torch.int32)
    pv = torch.randint(1, N + 1, (3000,), device=DEV, generator=gen, dtype=torch.int32)
    pv[:400] = pu[:400]                                           # self pairs
    pu[400:700], pv[400:700] = pu[700:1000], pv[700:1000]         # duplicated pairs
    pu[1000:1100] = pu[1100:1200].flip(0)
    pv[1000:1100] = pu[1000:1100]                                 # self pairs repeated
    nu = torch.randint(1, N + 1, (800,), device=DEV, generator=gen, dtype=torch.int32)
    nv = torch.randint(1, N + 1, (800,), device=DEV, generator=gen, dtype=torch.int32)
    nu[:100], nv[:100] = nu[100:200], nv[100:200]                 # duplicated negatives
    Zg = Z.clone().requires_grad_(True)
    pre = ops.sort_edges_by_key(torch.cat([pu, pv]), N)
    loss, s = ops.link_loss(Zg, pu, pv, nu, nv, pos_sorted=pre)
    (loss * 2.5).backward()
    Zr = Z.double().requires_grad_(True)
    rl, rs = _ref_loss(Zr, torch.cat([pu, nu]).long(), torch.cat([pv, nv]).long(), pu.numel())
    (rl * 2.5).backward()
    assert_close(loss, rl.detach(), 'loss')
    assert_close(s, rs.detach(), 's')
    assert_close(Zg.grad, Zr.grad, 'dZ with self and duplicated pairs')


def test_training_with_an_output_wider_than_the_row_scatter():
    """train(output = 260): the link loss's backward scatters dZ in column blocks (it raised SGNN_ERR_UNSUPPORTED_D above 256
    columns); two runs write the same finite table."""
    from subgnn_amd.train_node_emb import train
    g, _ = hub_graph()
    a = train(g, 'gcn', epochs=3, seed=2, hidden=64, output=260)
    b = train(g, 'gcn', epochs=3, seed=2, hidden=64, output=260)
    assert a['embeddings'].shape == (g.max_id, 260) and bool(torch.isfinite(a['embeddings']).all())
    assert torch.equal(a['embeddings'], b['embeddings'])
    assert len({h['loss'] for h in a['history']}) == 3


# ---- A5: the negative sampler running out of draws ----------------------------------------------------------------------

def _twin_negatives(g, n, seed, sid, item_base=0, max_attempts=64):
    """sgnn_ne_negatives restated on the host with the pure-Python draw tape."""
    from oracle.tape import draw64
    rp, cs = g.rowptr.cpu().numpy(), g.col_sorted.cpu().numpy()
    N = g.max_id
    u, v = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        for att in range(max_attempts):
            d = draw64(seed, sid, item_base + i, att)
            a = 1 + (((d >> 32) * N) >> 32)
            b = 1 + (((d & 0xFFFFFFFF) * N) >> 32)
            row = cs[rp[a]:rp[a + 1]]
            j = np.searchsorted(row, b)
            if a != b and not (j < len(row) and row[j] == b):
                u[i], v[i] = a, b
                break
    return u, v


def _graph(edges):
    from subgnn_amd.graph import networkx_order_csr
    from subgnn_amd.ops import DeviceGraph
    rowptr, col, order = networkx_order_csr(np.asarray(edges, dtype=np.int64))
    return DeviceGraph(rowptr, col, order, DEV)


K20 = [(a, b) for a in range(20) for b in range(a + 1, 20)]


@pytest.mark.parametrize('graph', ['K20', 'one node'])
def test_negatives_exhausted_give_zero_pairs(graph):
    """A complete graph (every u != v is an edge) and a graph of one node id (every draw is u == v): no pair is ever
    accepted, and every result is (0, 0), as the host twin says."""
    from subgnn_amd import ops
    g = _graph(K20 if graph == 'K20' else [(0, 0)])
    assert g.max_id == (20 if graph == 'K20' else 1)
    n, seed, sid = 300, 4, (2 << 32) | 9
    u, v = ops.ne_negatives(g, n, seed, sid, item_base=5)
    wu, wv = _twin_negatives(g, n, seed, sid, item_base=5)
    assert not wu.any() and not wv.any()
    assert u.cpu().tolist() == wu.tolist() and v.cpu().tolist() == wv.tolist()


@pytest.mark.parametrize('item_base, max_attempts', [(0, 1), (17, 2), ((1 << 32) + 12345, 64)])
def test_negatives_attempt_limit_and_large_item_base(item_base, max_attempts):
    """One or two attempts leave many pairs (0, 0) on the hub graph, exactly those the twin leaves; an item_base above 2^32
    (draw items are 64-bit) matches too."""
    from subgnn_amd import ops
    g, _ = hub_graph()
    n, seed, sid = 2000, 13, (11 << 32) | 3
    u, v = ops.ne_negatives(g, n, seed, sid, item_base=item_base, max_attempts=max_attempts)
    wu, wv = _twin_negatives(g, n, seed, sid, item_base, max_attempts)
    assert u.cpu().tolist() == wu.tolist() and v.cpu().tolist() == wv.tolist()
    if max_attempts == 1:
        assert 0 < int((wu == 0).sum()) < n


def test_training_on_a_complete_graph_refuses_instead_of_writing(tmp_path):
    """train_node_emb.generate on K20: no negative exists, so the trainer raises 'graph too dense' and writes no table."""
    from subgnn_amd import train_node_emb
    (tmp_path / 'edge_list.txt').write_text(''.join('%d %d\n' % e for e in K20))
    with pytest.raises(RuntimeError, match='graph too dense'):
        train_node_emb.generate(tmp_path, epochs=2, hidden=16, output=8, device=DEV)
    assert not any(tmp_path.glob('*.pth')) and not (tmp_path / 'node_emb.json').exists()


# ---- B1: non-finite gradients through ClipAdam -----------------------------------------------------------------------------

def _same_nonfinite(a, b, what, norm_tol=2e-6):
    """a == b where b is NaN or +-inf, assert_close on the finite rest."""
    a, b = a.detach().double(), b.detach().double()
    assert torch.equal(torch.isnan(a), torch.isnan(b)), '%s: NaN at other places' % what
    assert torch.equal(torch.isinf(b), torch.isinf(a)) and torch.equal(a[torch.isinf(b)], b[torch.isinf(b)]), what
    fin = torch.isfinite(b)
    assert_close(a[fin], b[fin], what, norm_tol=norm_tol)


def _torch_clip(params, max_norm):
    """clip_grad_norm_ -> (coefficient, total norm) as it applies them."""
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return torch.stack([torch.clamp(max_norm / (total + 1e-6), max=1.0), total])


@pytest.mark.parametrize('capturable', [False, True])
@pytest.mark.parametrize('poison', ['nan-table', 'nan-small', 'inf-table', 'inf-small'])
def test_clip_adam_non_finite_gradients_match_torch(poison, capturable):
    """ClipAdam(max_norm = 0.5) == clip_grad_norm_ + torch.optim.Adam over three steps whose middle one carries a NaN or +inf
    gradient element, in the table or in a small parameter, then a finite step.  A NaN norm makes the coefficient NaN and every
    parameter NaN (torch's clamp keeps NaN); an infinite norm makes it 0 (NaN only where inf * 0 lands).  The row-skip table
    path stays bit-identical to the dense one: under a NaN coefficient its untouched rows turn NaN too."""
    from subgnn_amd import optim
    gen = torch.Generator().manual_seed(len(poison))
    rows, D = 2001, 32
    shapes = [(rows, D), (D, 9), (D,)]
    init = [torch.randn(*s, generator=gen) for s in shapes]
    models = [[torch.nn.Parameter(t.clone().to(DEV)) for t in init] for _ in range(3)]
    o_skip = optim.ClipAdam(models[0], lr=0.01, max_norm=0.5, big_bytes=rows * D * 4, capturable=capturable)
    o_dense = optim.ClipAdam(models[1], lr=0.01, max_norm=0.5, big_bytes=rows * D * 4, capturable=capturable,
                             skip_untouched_rows=False)
    o_ref = torch.optim.Adam(models[2], lr=0.01)
    assert len(o_skip.tail.seen) == 1 and not o_dense.tail.seen
    for it in range(3):
        pick = torch.rand(rows, generator=gen) < 0.1
        pick[0] = False
        grads = [torch.randn(rows, D, generator=gen) * pick.unsqueeze(1), torch.randn(D, 9, generator=gen),
                 torch.randn(D, generator=gen)]
        if it == 1:
            bad = float('nan') if poison.startswith('nan') else float('inf')
            if poison.endswith('table'):
                grads[0][int(torch.nonzero(pick)[3]), 5] = bad
            else:
                grads[1][4, 2] = bad
        for ps in models:
            for p, gr in zip(ps, grads):
                p.grad = gr.clone().to(DEV)
        want = _torch_clip(models[2], 0.5)
        o_skip.step(); o_dense.step(); o_ref.step()
        for opt, ps, name in ((o_skip, models[0], 'row-skip'), (o_dense, models[1], 'dense')):
            _same_nonfinite(opt.last_clip, want, '%s %s step %d: (coefficient, norm)' % (poison, name, it), norm_tol=None)
            for k, (a, b) in enumerate(zip(ps, models[2])):
                _same_nonfinite(a, b, '%s %s step %d parameter %d' % (poison, name, it, k))
        for opt in (o_skip, o_dense, o_ref):
            opt.zero_grad()
        for name in ('exp_avg', 'exp_avg_sq'):
            a, b = o_skip.state[id(models[0][0])][name], o_dense.state[id(models[1][0])][name]
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
        a, b = models[0][0].detach(), models[1][0].detach()
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]), it
    if poison.startswith('nan'):
        assert all(bool(torch.isnan(p).all()) for p in models[0])
    else:
        assert 0 < int(torch.isnan(models[0][0 if poison.endswith('table') else 1]).sum()) < D


def test_adam_step_propagates_a_nan_grad_scale():
    """dist.ShardedTableAdam's form: ops.adam_step(grad_scale = a device NaN) turns the whole slice NaN, as torch's Adam on
    the NaN-multiplied gradient does."""
    from subgnn_amd import ops
    n = 4099
    p = torch.randn(n, device=DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ops.adam_step(p, torch.randn(n, device=DEV), m, v, 1e-3, (0.9, 0.999), 1e-8, 1,
                  grad_scale=torch.full((1,), float('nan'), device=DEV))
    assert bool(torch.isnan(p).all() and torch.isnan(m).all() and torch.isnan(v).all())


# ---- B2: launch groups and sizes of the optimizer tail ---------------------------------------------------------------------

def _run_against_torch(init, steps, max_norm, capturable, big_bytes, missing=lambda it, i: False, skip=True, tol=2e-6):
    from subgnn_amd import optim
    gen = torch.Generator().manual_seed(len(init) + steps)
    ref = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    got = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    o_ref = torch.optim.Adam(ref, lr=0.01)
    o_got = optim.ClipAdam(got, lr=0.01, max_norm=max_norm, big_bytes=big_bytes, capturable=capturable,
                           skip_untouched_rows=skip)
    for it in range(steps):
        grads = [torch.randn(*t.shape, generator=gen).to(DEV) * (3.0 if it % 2 else 0.1) for t in init]
        for ps in (ref, got):
            for i, (p, gr) in enumerate(zip(ps, grads)):
                p.grad = None if missing(it, i) else gr.clone()
        want = _torch_clip(ref, max_norm)
        o_ref.step(); o_got.step()
        coef, norm = o_got.last_clip.double().cpu()
        assert abs(float(norm) - float(want[1])) <= 1e-5 * float(want[1]), (float(norm), float(want[1]))
        assert abs(float(coef) - float(want[0])) <= 1e-5 * float(want[0]), (float(coef), float(want[0]))
        o_ref.zero_grad(); o_got.zero_grad()
        for k, (a, b) in enumerate(zip(got, ref)):
            assert_close(a.detach(), b.detach(), 'step %d parameter %d (%d elements)' % (it, k, a.numel()), norm_tol=tol)
    want_steps = [int(o_ref.state[p]['step']) if p in o_ref.state else 0 for p in ref]
    assert [int(e['step']) for _, e in sorted(o_got.state_dict()['state'].items())] == want_steps
    return got, o_got


@pytest.mark.parametrize('capturable', [False, True])
@pytest.mark.parametrize('n_params', [72, 73])
@pytest.mark.parametrize('max_norm', [0.5, 1e-8])
def test_clip_adam_launch_group_edges(n_params, max_norm, capturable):
    """Exactly OPT_MAXT = 72 parameters (one launch) and 73 (a second launch of one), some without a gradient on some steps
    (their host step counts fall behind and split the launch groups), with a normal clip and with a coefficient of ~1e-9."""
    gen = torch.Generator().manual_seed(n_params)
    init = [torch.randn(int(n), generator=gen) for n in torch.randint(1, 3000, (n_params,), generator=gen)]
    init[0] = torch.randn(20001, generator=gen)
    _run_against_torch(init, 4, max_norm, capturable, big_bytes=20001 * 4,
                       missing=lambda it, i: (i % 5 == 4 and it == 1) or (i == n_params - 1 and it == 2))


@pytest.mark.parametrize('capturable', [False, True])
def test_clip_adam_steps_zero_element_parameters(capturable):
    """A zero-element parameter with a (zero-element) gradient is stepped as torch steps it: nothing to update, but its step
    count advances; the others are clipped and updated as usual."""
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(300, 64, generator=gen), torch.randn(0, generator=gen), torch.randn(17, generator=gen),
            torch.randn(0, 64, generator=gen)]
    got, o_got = _run_against_torch(init, 3, 0.5, capturable, big_bytes=300 * 64 * 4, missing=lambda it, i: i == 3 and it == 0)
    assert len(o_got.big) == 1 and got[1].numel() == 0


@pytest.mark.parametrize('form', ['dense', 'table'])
def test_clip_adam_parameter_larger_than_one_grid(form):
    """One parameter above OPT_MAX_BLOCKS x OPT_CHUNK = 8 388 608 floats, so that each of its workgroups strides over more
    than one chunk: a dense vector whose length is not a multiple of 4, and a 140 000 x 64 table with its row-skip path
    (gradients on a few rows), bit-identical to the dense update of the same table and equal to torch."""
    from subgnn_amd import optim
    gen = torch.Generator().manual_seed(9)
    if form == 'dense':
        init = [torch.randn(8_388_608 + 4099, generator=gen), torch.randn(64, 9, generator=gen)]
        _run_against_torch(init, 3, 0.5, False, big_bytes=1 << 40)
        return
    rows, D = 140_000, 64
    init = [torch.randn(rows, D, generator=gen), torch.randn(D, 9, generator=gen)]
    models = [[torch.nn.Parameter(t.clone().to(DEV)) for t in init] for _ in range(3)]
    o_skip = optim.ClipAdam(models[0], lr=0.01, max_norm=0.5, big_bytes=rows * D * 4)
    o_dense = optim.ClipAdam(models[1], lr=0.01, max_norm=0.5, big_bytes=rows * D * 4, skip_untouched_rows=False)
    o_ref = torch.optim.Adam(models[2], lr=0.01)
    assert len(o_skip.tail.seen) == 1 and not o_dense.tail.seen
    for it in range(3):
        pick = torch.rand(rows, generator=gen) < 0.05
        pick[0] = False
        grads = [torch.randn(rows, D, generator=gen) * pick.unsqueeze(1), torch.randn(D, 9, generator=gen)]
        for ps in models:
            for p, gr in zip(ps, grads):
                p.grad = gr.to(DEV)
        want = _torch_clip(models[2], 0.5)
        for opt in (o_skip, o_dense, o_ref):
            opt.step()
            opt.zero_grad()
        assert abs(float(o_skip.last_clip[1]) - float(want[1])) <= 1e-5 * float(want[1])
        assert torch.equal(models[0][0], models[1][0]) and torch.equal(models[0][1], models[1][1]), it
        for k, (a, b) in enumerate(zip(models[0], models[2])):
            assert_close(a.detach(), b.detach(), 'table step %d parameter %d' % (it, k), norm_tol=2e-6)

"""GPU counterpart of the reference's prepare_dataset/train_node_emb.py (+ model.py, preprocess.py, utils.py): pre-trains the
node-embedding table SubGNN reads (``gin_embeddings.pth`` / ``graphsaint_gcn_embeddings.pth``, train_config.py:227-232) on
the whole base graph, without PyTorch Geometric and without the reference's dense one-hot feature matrix (``np.eye(N)``,
preprocess.py:39 -- 4 TB at 1M nodes).

Model (model.py:15-36): two graph convolutions, relu and dropout between them.  With one-hot features the first layer's
Linear(N, hidden) is a trainable (N, hidden) table T, so both layers are  out = A X + b  for a sparse operator A:
  GIN  (GINConv, eps = 0, nn = one Linear):  A = I + adjacency of the message graph (a self loop of the edge list counts again);
  GCN  (GCNConv, PyG gcn_norm):  add_remaining_self_loops (weight 1), deg = in-degree at the target + 1,
       A[i, j] = deg[j]^-1/2 deg[i]^-1/2.
Layer 2 is aggregated AFTER its Linear (at the narrower output width: A (H W^T) = (A H) W^T).

Message direction (preprocess.py:38,60): ``edge_index = list(G.edges)`` of ``nx.read_edgelist(nodetype=int)`` lists every
undirected edge once, from the node that comes earlier in networkx node order (first appearance in the file) to the later one;
messages flow source -> target, so in the reference's model a node hears only its EARLIER neighbours.  That is the default,
``edge_direction='reference'`` (on a device-built CSR, node order = id order: u -> v iff u < v); ``'both'`` uses the symmetric
graph.  The positives of the link loss are the edges of the graph either way.

Training (train_node_emb.py:40-110, utils.py:22-56): edges split 80/10/10; every epoch the train edges plus n_pos // 4 negatives
are scored with s = sigmoid(z_u . z_v), loss = nll(log_softmax(stack(1 - s, s)), y); Adam with coupled L2; val ROC-AUC, AP,
accuracy and F1 at 0.5 on the val edges plus fresh negatives, computed from the epoch's training-mode output as the reference
does; the parameters of the epoch where best_val_acc <= val_acc + 1e-3 are kept; the eval-mode output (no dropout) of the kept
parameters is saved, shape (N, output), row i = the node labelled i.

A reference defect, documented and not copied: ``el_dot`` detaches the embeddings (utils.py:51) and ``calc_loss_both`` sets
``loss.requires_grad = True`` on the result (utils.py:35), so ``loss.backward()`` (train_node_emb.py:76) reaches no parameter and
Adam skips every one of them (their gradients are None: not even the weight decay applies).  The reference therefore ships the
UNTRAINED network's output.  Here the loss trains the network; ``epochs=0`` reproduces what the reference effectively writes.

Deliberate differences:
  * full batch over the whole graph instead of GraphSAINT / NeighborSampler mini-batches (whose PyG random streams cannot be
    restated offline);
  * negatives are true non-edges of the base graph in either direction and never self pairs (PyG's negative_sampling only
    avoids the positive set it is given);
  * the edge split, the negatives and the dropout masks come from the draw tape (tape.STREAM_NE_*): parity with the reference is
    at the level of the math, not of PyG's or numpy's streams;
  * the hyper-parameter search visits the parameter types and their values in the listed order (the reference shuffles both
    with python's random) and keeps copies of the best values (the reference aliases the two dicts);
  * node ids absent from the edge list get a row like isolated nodes (the reference needs ids 0..N-1).
"""
import argparse
import json
import time
from pathlib import Path

import numpy as np
import torch

from . import ops, tape
from .graph import load_graph
from .subgraph_utils import average_precision, roc_auc

# config_prepare_dataset.py:46-56: the first value of each grid is the default
GRID = {'hidden': [128, 256], 'output': [64], 'lr': [1e-3, 5e-3], 'wd': [5e-4, 5e-5], 'dropout': [0.4, 0.5]}
DEFAULTS = {k: v[0] for k, v in GRID.items()}
EPOCHS = 100
EPS = 1e-3                    # train_node_emb.py:25  (eps = 10e-4)
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
FILE_NAMES = {'gin': 'gin_embeddings.pth', 'gcn': 'graphsaint_gcn_embeddings.pth'}    # train_config.py:227-232


def reference_edges(edges):
    """``list(nx.read_edgelist(path, nodetype=int).edges)`` restated with numpy: edges (E, 2) 0-based ids in file order ->
    (M, 2) directed pairs (earlier node in first-appearance order, later node), each undirected edge once, self loops once."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if edges.size == 0:
        return edges
    ids, first = np.unique(edges.reshape(-1), return_index=True)
    pos = np.empty(int(ids.max()) + 1, dtype=np.int64)
    pos[ids] = np.argsort(np.argsort(first, kind='stable'), kind='stable')
    a, b = edges[:, 0], edges[:, 1]
    swap = pos[b] < pos[a]
    src, dst = np.where(swap, b, a), np.where(swap, a, b)
    pairs = np.unique(np.stack([src, dst], 1), axis=0)
    return pairs


class Messages:
    """The message operator of one (graph, conv, edge_direction), built once per graph from DeviceGraph.col_sorted and
    node_pos: ``fwd`` (row = target), ``bwd`` (its transpose, row = source; the backward of the aggregation), and the
    positive edges (pos_u, pos_v) of the link loss (1-based ids, each edge of the graph once)."""

    def __init__(self, g, conv='gin', edge_direction='reference'):
        if conv not in ('gin', 'gcn'):
            raise ValueError("conv must be 'gin' or 'gcn'")
        if edge_direction not in ('reference', 'both'):
            raise ValueError("edge_direction must be 'reference' or 'both'")
        self.conv, self.edge_direction = conv, edge_direction
        dev = g.rowptr.device
        n = g.max_id + 1                                                  # rows 0 (PAD, no edges) .. max_id
        rowptr, col = g.rowptr, g.col_sorted[:g.nnz].to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])
        first = torch.ones_like(col, dtype=torch.bool)                   # an id twice in a row counts once (nx.Graph)
        if col.numel() > 1:
            first[1:] = (col[1:] != col[:-1]) | (rows[1:] != rows[:-1])
        pos = g.node_pos.to(torch.int64)
        is_self = (col == rows) & first
        earlier = (pos[col] < pos[rows]) & first & ~is_self               # col -> row in the reference direction
        later = (pos[col] > pos[rows]) & first & ~is_self
        if edge_direction == 'reference':
            fk, bk = earlier, later
        else:
            fk = bk = first & ~is_self
        n_self = torch.zeros(n, dtype=torch.float32, device=dev)
        n_self.index_add_(0, rows[is_self], torch.ones(int(is_self.sum()), dtype=torch.float32, device=dev))
        f_rowptr, f_col = self._sub(rowptr, fk), col[fk].to(torch.int32)
        b_rowptr, b_col = self._sub(rowptr, bk), col[bk].to(torch.int32)
        real = torch.zeros(n, dtype=torch.bool, device=dev)
        real[1:] = True
        if conv == 'gin':
            a_self = torch.where(real, 1.0 + n_self, torch.zeros_like(n_self))
            fw = bw = None
        else:
            deg = (f_rowptr[1:] - f_rowptr[:-1]).to(torch.float32) + 1.0     # add_remaining_self_loops: one loop of weight 1
            dinv = torch.where(real, deg.pow(-0.5), torch.zeros_like(deg))
            a_self = dinv * dinv
            fw = dinv[rows[fk]] * dinv[col[fk]]
            bw = dinv[rows[bk]] * dinv[col[bk]]
        self.a_self = a_self.contiguous()
        self.fwd = ops.MessageCSR(f_rowptr, f_col, fw, self.a_self)
        self.bwd = ops.MessageCSR(b_rowptr, b_col, bw, self.a_self)
        pk = earlier | is_self
        self.pos_u, self.pos_v = col[pk].to(torch.int32), rows[pk].to(torch.int32)
        self.n_nodes = g.max_id

    @staticmethod
    def _sub(rowptr, keep):
        c = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=rowptr.device)
        c[1:] = torch.cumsum(keep.to(torch.int64), 0)
        return c[rowptr]

    def dense(self):
        """The forward operator as a dense float64 (N + 1, N + 1) CPU matrix (tests)."""
        n = self.fwd.n_rows
        A = torch.zeros(n, n, dtype=torch.float64)
        rp, col = self.fwd.rowptr.cpu(), self.fwd.col.cpu().long()
        rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
        w = self.fwd.w.cpu().double() if self.fwd.w is not None else torch.ones(col.numel(), dtype=torch.float64)
        A.index_put_((rows, col), w, accumulate=True)
        A += torch.diag(self.a_self.cpu().double())
        return A


def edge_split(n_edges, seed):
    """80/10/10 split of the edge numbers (create_dataset, preprocess.py:66-70): the permutation orders the edges by their
    draw64(seed, STREAM_NE_SPLIT, e, 0) -> (train, val, test) int64 numpy index arrays."""
    keys = tape.draw64_np(seed, tape.stream_id(tape.STREAM_NE_SPLIT), np.arange(n_edges, dtype=np.uint64), 0)
    perm = np.argsort(keys, kind='stable')
    a, b = 8 * n_edges // 10, 9 * n_edges // 10
    return perm[:a], perm[a:b], perm[b:]


def link_metrics(s, n_pos):
    """calc_roc_score (utils.py:103-113): ROC-AUC, AP, accuracy and F1 at 0.5; pairs < n_pos are the positives."""
    s = s.detach().cpu().numpy().astype(np.float64)
    y = np.zeros(s.size, dtype=bool)
    y[:n_pos] = True
    pred = s > 0.5
    tp, fp, fn = int(np.sum(pred & y)), int(np.sum(pred & ~y)), int(np.sum(~pred & y))
    f1 = 2.0 * tp / (2 * tp + fp + fn) if tp + fp + fn else 0.0
    return {'roc': roc_auc(y, s), 'ap': average_precision(y, s), 'acc': float(np.mean(pred == y)), 'f1': f1}


class Trainer:
    """One model (one hyper-parameter setting) on one graph.  ``step(epoch)`` runs the training epoch on the GPU (forward,
    negatives, loss, backward, Adam) and returns (loss, Z) as device tensors; ``validate`` scores the val pairs on the host."""

    def __init__(self, g, msgs, split, conv, hidden, output, lr, wd, dropout, seed, run=0):
        self.g, self.m, self.conv = g, msgs, conv
        self.lr, self.wd, self.dropout, self.seed, self.run = lr, wd, dropout, seed, run
        dev = g.rowptr.device
        n = g.max_id + 1
        gen = torch.Generator(device=dev).manual_seed(int(seed) * 1000003 + run)

        def uniform(shape, bound):
            return (torch.rand(shape, generator=gen, device=dev) * 2 - 1) * bound
        N = g.max_id
        if conv == 'gin':          # nn.Linear(N, hidden) / nn.Linear(hidden, output): U(+-1/sqrt(fan_in)) weights and biases
            T, b1 = uniform((n, hidden), N ** -0.5), uniform((hidden,), N ** -0.5)
            W2, b2 = uniform((output, hidden), hidden ** -0.5), uniform((output,), hidden ** -0.5)
        else:                      # GCNConv: glorot weights, zero biases
            T, b1 = uniform((n, hidden), (6.0 / (N + hidden)) ** 0.5), torch.zeros(hidden, device=dev)
            W2, b2 = uniform((output, hidden), (6.0 / (hidden + output)) ** 0.5), torch.zeros(output, device=dev)
        T[0] = 0                   # the PAD row: no node, no gradient, stays 0 under the decay
        self.params = [p.contiguous().requires_grad_(True) for p in (T, b1, W2, b2)]
        self.state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in self.params]
        self.t = 0
        tr, va, te = (torch.from_numpy(np.asarray(x, dtype=np.int64)).to(dev) for x in split)
        pu, pv = msgs.pos_u, msgs.pos_v
        self.train_u, self.train_v = pu[tr].contiguous(), pv[tr].contiguous()
        self.val_u, self.val_v = pu[va].contiguous(), pv[va].contiguous()
        self.test_u, self.test_v = pu[te].contiguous(), pv[te].contiguous()
        self.train_sorted = ops.sort_edges_by_key(torch.cat([self.train_u, self.train_v]), g.max_id)

    def stream(self, kind, split=0, epoch=0):
        return tape.stream_id(kind, split, layer=self.run, epoch=epoch)

    def forward(self, params=None, train=True, epoch=0):
        T, b1, W2, b2 = params or self.params
        m = self.m
        H = ops.graph_conv(T, b1, m.fwd, m.bwd, relu=True, dropout=self.dropout if train else 0.0, seed=self.seed,
                           stream_id=self.stream(tape.STREAM_NE_DROP, epoch=epoch))
        return ops.graph_conv(ops.linear(H, W2, None), b2, m.fwd, m.bwd)

    def negatives(self, n, split, epoch):
        return ops.ne_negatives(self.g, n, self.seed, self.stream(tape.STREAM_NE_NEG, split, epoch))

    def step(self, epoch):
        for p in self.params:
            p.grad = None
        Z = self.forward(epoch=epoch)
        nu, nv = self.negatives(self.train_u.numel() // 4, 'train', epoch)
        loss, _ = ops.link_loss(Z, self.train_u, self.train_v, nu, nv, pos_sorted=self.train_sorted)
        loss.backward()
        self.t += 1
        with torch.no_grad():
            for p, (m, v) in zip(self.params, self.state):
                ops.adam_step(p, p.grad.contiguous(), m, v, self.lr, BETAS, ADAM_EPS, self.t, weight_decay=self.wd)
        self.last_negatives = (nu, nv)
        return loss.detach(), Z.detach()

    def score(self, Z, pu, pv, split, epoch):
        nu, nv = self.negatives(pu.numel() // 4, split, epoch)
        if bool((nu == 0).any()):
            raise RuntimeError('negative sampling: no non-edge found in 64 draws (graph too dense)')
        _, s, _ = ops.ne_link_loss(Z, torch.cat([pu, nu]), torch.cat([pv, nv]), pu.numel(), want_grad=False)
        return link_metrics(s, pu.numel())

    def validate(self, Z, epoch):
        if bool((self.last_negatives[0] == 0).any()):
            raise RuntimeError('negative sampling: no non-edge found in 64 draws (graph too dense)')
        return self.score(Z, self.val_u, self.val_v, 'val', epoch)

    @torch.no_grad()
    def embeddings(self, params=None):
        """Eval-mode output (no dropout), (N + 1, output) with the PAD row 0."""
        return self.forward(params, train=False)


def _train_one(g, msgs, split, conv, hp, epochs, seed, run, best, history):
    tr = Trainer(g, msgs, split, conv, hp['hidden'], hp['output'], hp['lr'], hp['wd'], hp['dropout'], seed, run)
    if epochs == 0 and best['params'] is None:          # what the reference effectively ships: the untrained network
        best.update(params=[p.detach().clone() for p in tr.params], hp=dict(hp), trainer=tr)
    for ep in range(epochs):
        loss, Z = tr.step(ep)
        val = tr.validate(Z, ep)
        history.append(dict(run=run, epoch=ep, loss=float(loss.item()), **{'val_' + k: v for k, v in val.items()}))
        if best['val_acc'] <= val['acc'] + EPS:
            best.update(val_acc=val['acc'], params=[p.detach().clone() for p in tr.params], hp=dict(hp), trainer=tr)
    return tr


def train(g, conv='gin', edge_direction='reference', hidden=128, output=64, lr=1e-3, wd=5e-4, dropout=0.4, epochs=EPOCHS, seed=0,
          search=False, log=None):
    """In-memory entry: pre-trains on the DeviceGraph ``g`` -> dict(embeddings = (N, output) float32 device tensor, row i = node
    id i + 1, hparams, history (per-epoch loss / val metrics), test metrics).  ``search``: the reference's coordinate search over
    GRID (train_node_emb.py:126-152), ``epochs`` per setting, the parameters of the best epoch over all of them kept."""
    msgs = Messages(g, conv, edge_direction)
    split = edge_split(msgs.pos_u.numel(), seed)
    hp = dict(hidden=hidden, output=output, lr=lr, wd=wd, dropout=dropout)
    best = dict(val_acc=-1.0, params=None, hp=None, trainer=None)
    history = []
    if not search:
        _train_one(g, msgs, split, conv, hp, epochs, seed, 0, best, history)
    else:
        run = 0
        for key in GRID:
            for val in GRID[key]:
                cur = dict(hp, **{key: val})
                if log:
                    log(json.dumps(cur))
                _train_one(g, msgs, split, conv, cur, epochs, seed, run, best, history)
                run += 1
            hp[key] = best['hp'][key]
    tr = best['trainer']
    Z = tr.embeddings(best['params'])
    test = tr.score(Z, tr.test_u, tr.test_v, 'test', 0)
    return dict(embeddings=Z[1:].contiguous(), hparams=best['hp'], history=history, test=test, best_val_acc=best['val_acc'])


def generate(dataset_dir, conv='gin', edge_direction='reference', hidden=128, output=64, lr=1e-3, wd=5e-4, dropout=0.4,
             epochs=EPOCHS, seed=0, search=False, device=None):
    """Reads ``edge_list.txt`` (graph.load_graph) and writes the table SubGNN reads -- gin_embeddings.pth (GIN) or
    graphsaint_gcn_embeddings.pth (GCN, embedding_type 'graphsaint') -- plus node_emb.json (hyper-parameters, per-epoch loss and
    val metrics, test metrics).  Returns the table's path."""
    d = Path(dataset_dir)
    device = device or torch.device('cuda')
    g = load_graph(d / 'edge_list.txt', device)
    t0 = time.time()
    res = train(g, conv, edge_direction, hidden, output, lr, wd, dropout, epochs, seed, search)
    path = d / FILE_NAMES[conv]
    torch.save(res['embeddings'].cpu(), path)
    with open(d / 'node_emb.json', 'w') as f:
        json.dump(dict(conv=conv, edge_direction=edge_direction, epochs=epochs, seed=seed, search=search, hparams=res['hparams'],
                       best_val_acc=res['best_val_acc'], test=res['test'], history=res['history'],
                       seconds=time.time() - t0), f, indent=1)
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description='Pre-train the node embeddings SubGNN reads (GIN / GCN link prediction)')
    ap.add_argument('dataset_dir')
    ap.add_argument('--conv', choices=('gin', 'gcn'), default='gin')
    ap.add_argument('--edge-direction', choices=('reference', 'both'), default='reference')
    for k, v in DEFAULTS.items():
        ap.add_argument('--' + k, type=type(v), default=v)
    ap.add_argument('--epochs', type=int, default=EPOCHS)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--search', action='store_true', help='coordinate search over the reference grid')
    a = ap.parse_args(argv)
    p = generate(a.dataset_dir, a.conv, a.edge_direction, a.hidden, a.output, a.lr, a.wd, a.dropout, a.epochs, a.seed, a.search)
    print(p)


if __name__ == '__main__':
    main()

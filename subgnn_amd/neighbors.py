"""Which known subgraphs does a subgraph resemble?  An index of subgraph embeddings and its nearest-row search.

``Predictor.predict(..., return_embeddings=True)`` makes a subgraph's embedding a function of the model and the node set alone
(subgnn_amd/predict.py), so embeddings of different requests compare with each other and with the dataset's own subgraphs.
``SubgraphIndex`` holds such embeddings (N, H) on the device with, per row, the node list in the dataset's numbering, the label
string(s), the split and the row within the split; ``ops.topk_rows`` (csrc/neighbors.hip) searches it: scores formed tile by
tile on the fp32 MFMA, each query's best k kept on chip, a strict total order (ties by the smaller row), no (Q, N) matrix.

The index of a model's own splits is built from the KEYED draws of ``Predictor.predict``, not from the splits' own: a query that
is a dataset subgraph then lands exactly on its row.

    python -m subgnn_amd.neighbors -config_path C -restoreModelPath DIR [-restoreModelName F] -subgraphs FILE -out FILE
                                   [-k 10] [-metric cosine|dot|l2] [-splits train,val,test] [-index FILE.npz] [-batch_size B]
"""
import argparse
import os

import numpy as np
import torch

from . import cli, ops

METRICS = ('cosine', 'dot', 'l2')
SPLITS = ('train', 'val', 'test')
LABEL_SEP = '-'                 # between the label strings of a multi-label row, as in subgraphs.pth


def _label_list(l):
    if l is None:
        return []
    return [l] if isinstance(l, str) else [str(x) for x in l]


class SubgraphIndex:
    def __init__(self, embeddings, subgraphs=None, labels=None, splits=None, rows=None, metric='cosine', checkpoint=None):
        if metric not in METRICS:
            raise ValueError('metric must be one of %s, got %r' % (METRICS, metric))
        E = torch.as_tensor(embeddings)
        if E.dim() != 2 or E.dtype != torch.float32:
            raise ValueError('embeddings must be a (N, H) float32 matrix')
        n = E.shape[0]
        self.embeddings = E.contiguous()
        self.subgraphs = [[int(v) for v in s] for s in subgraphs] if subgraphs is not None else [[] for _ in range(n)]
        self.labels = [_label_list(l) for l in labels] if labels is not None else [[] for _ in range(n)]
        self.splits = [str(s) for s in splits] if splits is not None else [''] * n
        self.rows = [int(r) for r in rows] if rows is not None else list(range(n))
        for name, v in (('subgraphs', self.subgraphs), ('labels', self.labels), ('splits', self.splits), ('rows', self.rows)):
            if len(v) != n:
                raise ValueError('%d %s for %d embeddings' % (len(v), name, n))
        self.metric = metric
        self.checkpoint = None if checkpoint is None else str(checkpoint)
        self._aux = None
        self._bank = None

    def __len__(self):
        return self.embeddings.shape[0]

    @property
    def width(self):
        return self.embeddings.shape[1]

    # ------------------------------------------------------------------ constructors -----
    @classmethod
    def from_embeddings(cls, E, subgraphs=None, labels=None, metric='cosine'):
        return cls(E, subgraphs=subgraphs, labels=labels, metric=metric)

    @classmethod
    def from_predictor(cls, predictor, splits=SPLITS, batch_size=None, metric='cosine'):
        """The model's own ``*_sub_G`` lists embedded through ``Predictor.predict`` (the keyed draws).  Reads the lists and the
        labels; the model's splits stay the objects they were."""
        m = predictor.model
        subs, labels, names, rows = [], [], [], []
        for sp in splits:
            if sp not in SPLITS:
                raise ValueError('unknown split %r' % (sp,))
            own = getattr(m, sp + '_sub_G')
            lab = getattr(m, sp + '_sub_G_label')
            for i, sg in enumerate(own):
                subs.append([int(v) - 1 for v in sg])                    # model ids are the dataset's + 1 (read_data)
                li = lab[i]
                ks = [int(x) for x in li] if isinstance(li, (list, tuple)) else [int(li)]
                labels.append([predictor.label_names[k] if predictor.label_names is not None else str(k) for k in ks])
                names.append(sp)
                rows.append(i)
        if not subs:
            raise ValueError('the splits %s hold no subgraph' % (tuple(splits),))
        E = predictor.predict(subs, batch_size=batch_size, return_embeddings=True)['embeddings']
        return cls(E.detach().float(), subs, labels, names, rows, metric, getattr(predictor, 'restored_from', None))

    # ------------------------------------------------------------------ files ------------
    def save(self, path):
        """One ``.npz``: the embeddings, the ragged node lists and label lists as pointer + value arrays, splits, rows, metric,
        checkpoint name.  Written under a temporary name and moved into place."""
        path = str(path)
        if not path.endswith('.npz'):
            raise ValueError('an index file is a .npz file')
        sub_ptr = np.zeros(len(self) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.subgraphs], out=sub_ptr[1:])
        lab_ptr = np.zeros(len(self) + 1, dtype=np.int64)
        np.cumsum([len(l) for l in self.labels], out=lab_ptr[1:])
        flat_labels = [x for l in self.labels for x in l]
        tmp = path[:-4] + '.tmp%d.npz' % os.getpid()
        try:
            np.savez(tmp, embeddings=self.embeddings.detach().cpu().numpy(), sub_ptr=sub_ptr,
                     sub_ids=np.asarray([v for s in self.subgraphs for v in s], dtype=np.int64), lab_ptr=lab_ptr,
                     lab_names=np.asarray(flat_labels, dtype=np.str_) if flat_labels else np.zeros(0, dtype='<U1'),
                     splits=np.asarray(self.splits, dtype=np.str_) if len(self) else np.zeros(0, dtype='<U1'),
                     rows=np.asarray(self.rows, dtype=np.int64), metric=np.asarray(self.metric),
                     checkpoint=np.asarray('' if self.checkpoint is None else self.checkpoint))
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    @classmethod
    def load(cls, path, device='cpu', predictor=None):
        """``predictor``: refuse a file whose embedding width is not the width of that model's subgraph embeddings."""
        with np.load(str(path), allow_pickle=False) as z:
            E = torch.from_numpy(z['embeddings'])
            sp, si = z['sub_ptr'], z['sub_ids']
            lp, ln = z['lab_ptr'], z['lab_names']
            idx = cls(E.to(device), [si[sp[i]:sp[i + 1]].tolist() for i in range(len(sp) - 1)],
                      [[str(x) for x in ln[lp[i]:lp[i + 1]]] for i in range(len(lp) - 1)], [str(s) for s in z['splits']],
                      z['rows'].tolist(), str(z['metric']), str(z['checkpoint']) or None)
        if predictor is not None:
            want = embedding_width(predictor)
            if idx.width != want:
                raise ValueError('%s holds embeddings of width %d, the model\'s are %d wide' % (path, idx.width, want))
        return idx

    # ------------------------------------------------------------------ queries ----------
    def _bank_aux(self):
        if self._aux is None:
            self._aux = ops.topk_aux(self.embeddings, self.metric)
        return self._aux

    def query_embeddings(self, E, k, exclude=None):
        """-> (scores (Q, k) float32, indices (Q, k) int64): the rows of the index nearest to every row of ``E``, best first,
        in the order of ops.topk_rows; ``exclude`` (Q,) int64: a row each query skips, or -1."""
        E = torch.as_tensor(E)
        if E.dim() != 2 or E.shape[1] != self.width:
            raise ValueError('queries must be (Q, %d)' % self.width)
        E = E.to(self.embeddings.device)
        return ops.topk_rows(E, self.embeddings, k, metric=self.metric, exclude=exclude, b_aux=self._bank_aux())

    def query(self, predictor, subgraphs, k, batch_size=None):
        """Embed the requests (node lists in the dataset's numbering) and search -> dict: ``scores``, ``indices``,
        ``embeddings`` (Q, H) and ``subgraphs`` (the mapped node sets of the requests: model ids, ascending)."""
        if embedding_width(predictor) != self.width:
            raise ValueError('the index holds embeddings of width %d, the model\'s are %d wide' % (self.width, embedding_width(predictor)))
        res = predictor.predict(subgraphs, batch_size=batch_size, return_embeddings=True)
        E = res['embeddings'].detach().float().contiguous()
        scores, indices = self.query_embeddings(E, k)
        return {'scores': scores, 'indices': indices, 'embeddings': E, 'subgraphs': res['subgraphs']}

    def self_neighbors(self, k):
        """Every row's nearest other rows (itself excluded): leave-one-out inspection of the index."""
        me = torch.arange(len(self), dtype=torch.int64, device=self.embeddings.device)
        return self.query_embeddings(self.embeddings, k, exclude=me)

    # ------------------------------------------------------------------ node overlap -----
    def _overlap_device(self):
        E = self.embeddings
        return E.device if E.is_cuda else torch.device('cuda', torch.cuda.current_device())

    def _overlap_bank(self):
        """The rows' node sets (ascending, repeats dropped) with their postings (ops.SetBank), built on first use and kept."""
        if self._bank is None:
            sets = ops.Ragged.from_lists([sorted(set(s)) for s in self.subgraphs], self._overlap_device())
            self._bank = ops.SetBank(sets)
        return self._bank

    def overlaps(self, lists, k=10, measure='jaccard', exclude=None):
        """Which rows share nodes with the requests (node lists in the index's numbering; repeats are dropped, a negative id is
        an error, an empty request gives fillers) -> dict of device tensors: ``rows`` (Q, k) int64, best first, fillers -1;
        ``inter`` (Q, k) int32, the shared nodes; ``touched`` (Q,) int32, the rows that share a node; ``scores`` (Q, k)
        float32 of ``measure`` ('jaccard', 'containment', 'coverage', 'count').  The order is that of ops.overlap_topk: exact,
        equal measures by the smaller row.  No model is needed."""
        sets = []
        for s in lists:
            ids = sorted({int(v) for v in s})
            if ids and (ids[0] < 0 or ids[-1] > 0x7fffffff):
                raise ValueError('a request holds an id outside 0 .. 2^31 - 1')
            sets.append(ids)
        bank = self._overlap_bank()
        q = ops.Ragged.from_lists(sets, bank.post_ptr.device)
        rows, inter, touched, scores = ops.overlap_topk(q, bank, k, measure, exclude=exclude)
        return {'rows': rows, 'inter': inter, 'touched': touched, 'scores': scores}

    def self_overlaps(self, k=10, measure='jaccard'):
        """Every row's best other rows by shared nodes, itself excluded (``touched`` still counts it): ``overlaps``."""
        bank = self._overlap_bank()
        me = torch.arange(len(self), dtype=torch.int64, device=bank.post_ptr.device)
        rows, inter, touched, scores = ops.overlap_topk(bank.sets, bank, k, measure, exclude=me)
        return {'rows': rows, 'inter': inter, 'touched': touched, 'scores': scores}

    def cluster(self, n_clusters, metric=None, medoids=5, **kmeans_args):
        """k-means of the index's rows on the device (ops.kmeans) -> ``subgnn_amd.cluster.Clustering``.  ``metric`` None: the
        index's own ('dot' is refused); ``medoids``: typical rows kept per cluster; further arguments go to ops.kmeans."""
        from .cluster import cluster_index
        return cluster_index(self, n_clusters, metric, medoids, **kmeans_args)

    def describe(self, row):
        """(split, row within the split, node list, label strings) of a row of the index."""
        return self.splits[row], self.rows[row], self.subgraphs[row], self.labels[row]


def embedding_width(predictor):
    return int(predictor.model.lin.in_features)


# ---------------------------------------------------------------------- files, CLI --------
def format_line(request, rank, score, split, row, nodes, label_strings):
    """``request<TAB>rank<TAB>score<TAB>split<TAB>row<TAB>n1-n2-...<TAB>label[-label]`` (9 significant digits: a float32
    survives the round trip)."""
    return '%d\t%d\t%.9g\t%s\t%d\t%s\t%s' % (request, rank, float(score), split, row, '-'.join(str(int(n)) for n in nodes),
                                             LABEL_SEP.join(label_strings))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Nearest known subgraphs of requested subgraphs, by the embeddings of a checkpoint')
    cli.add_run_arguments(ap)
    ap.add_argument('-subgraphs', type=str, required=True, help='one subgraph per line: n1-n2-... (further columns ignored)')
    ap.add_argument('-out', type=str, required=True,
                    help='text file: request<TAB>rank<TAB>score<TAB>split<TAB>row<TAB>n1-n2-...<TAB>label[-label] per (request, rank)')
    ap.add_argument('-k', type=int, default=10, help='neighbours per request')
    ap.add_argument('-metric', type=str, default='cosine', help='cosine, dot or l2')
    ap.add_argument('-splits', type=str, default=','.join(SPLITS), help='the splits whose subgraphs are indexed, comma-separated')
    ap.add_argument('-index', type=str, default=None, help='a .npz index file: loaded if it exists, else built and saved there')
    ap.add_argument('-batch_size', type=int, default=None, help='chunk the forward passes (default: one batch)')
    args = ap.parse_args(argv)
    if args.k < 1:
        ap.error('-k must be at least 1')
    if args.metric not in METRICS:
        ap.error('-metric must be one of %s' % ', '.join(METRICS))
    args.splits = cli.parse_splits(ap, args.splits)
    cli.require_positive(ap, args, ('batch_size',))
    if args.index is not None and not args.index.endswith('.npz'):
        ap.error('-index takes a .npz file name')
    if args.out == args.subgraphs or (args.index is not None and args.index in (args.out, args.subgraphs)):
        ap.error('-subgraphs, -out and -index must be different files')
    return args


def main(argv=None):
    args = parse_args(argv)
    from .predict import read_requests
    requests = read_requests(args.subgraphs)
    p = cli.open_predictor(args)
    index = cli.open_index(p, args)
    res = index.query(p, requests, args.k, batch_size=args.batch_size)
    scores, indices = res['scores'].cpu().numpy(), res['indices'].cpu().numpy()

    def lines():                                                         # formed while -out is written
        for i in range(scores.shape[0]):
            for r in range(scores.shape[1]):
                j = int(indices[i, r])                                   # (-1: fewer than k rows in the index)
                yield format_line(i, r, scores[i, r], *(index.describe(j) if j >= 0 else ('', -1, [], [])))
    cli.write_lines(args.out, lines())
    return res


if __name__ == '__main__':
    main()

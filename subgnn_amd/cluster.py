"""Which groups does a bank of subgraph embeddings fall into?  k-means over a ``SubgraphIndex`` and what each cluster holds.

``SubgraphIndex.cluster`` runs ``ops.kmeans`` (csrc/kmeans.hip: every Lloyd iteration assigns the rows under topk_rows' score
and total order and forms the per-cluster sums in one launch, no (N, K) matrix, no float atomics, repeatable bit for bit) and
returns a ``Clustering``: labels, centres, sizes, each row's score, per cluster the most typical rows (medoids: best score
first, then the smaller row), the counts of the index's label strings, the majority label and its purity, and overall purity
and normalised mutual information against the first label string of each row.

    python -m subgnn_amd.cluster -config_path C -restoreModelPath DIR [-restoreModelName F] -n_clusters K -out FILE
           [-summary FILE.json] [-metric cosine|l2] [-splits train,val,test] [-index FILE.npz] [-init k-means++|random]
           [-n_init R] [-max_iter I] [-seed S] [-medoids M] [-subgraphs FILE]
"""
import argparse
import json
import os

import numpy as np
import torch

from . import cli, ops
from .neighbors import LABEL_SEP, SPLITS

METRICS = ('cosine', 'l2')
INITS = ('k-means++', 'random')
HEADER = 'split\trow\tcluster\tscore\tnodes\tlabels'


# ---------------------------------------------------------------------- figures -----------
def contingency(labels, classes):
    """(n clusters present .. , n classes) counts of two integer label vectors, as int64 (rows: values of ``labels``)."""
    labels, classes = np.asarray(labels, dtype=np.int64), np.asarray(classes, dtype=np.int64)
    _, li = np.unique(labels, return_inverse=True)
    _, ci = np.unique(classes, return_inverse=True)
    m = np.zeros((li.max() + 1 if len(li) else 0, ci.max() + 1 if len(ci) else 0), dtype=np.int64)
    np.add.at(m, (li, ci), 1)
    return m


def purity(labels, classes):
    """The share of rows that carry their cluster's majority class."""
    m = contingency(labels, classes)
    return float(m.max(axis=1).sum() / m.sum()) if m.size and m.sum() else 0.0


def nmi(labels, classes):
    """Normalised mutual information of two labelings, natural logarithms, normalised by the arithmetic mean of the two
    entropies (scikit-learn's default); 1.0 when both are constant."""
    m = contingency(labels, classes).astype(np.float64)
    n = m.sum()
    if n == 0:
        return 1.0
    a, b = m.sum(axis=1), m.sum(axis=0)
    if len(a) == 1 and len(b) == 1:
        return 1.0

    def entropy(c):
        c = c[c > 0]
        return float(-np.sum((c / n) * (np.log(c) - np.log(n))))
    i, j = np.nonzero(m)
    v = m[i, j]
    mi = float(np.sum((v / n) * (np.log(v) - np.log(n)) + (v / n) * (-np.log(a[i]) - np.log(b[j]) + 2 * np.log(n))))
    mi = max(mi, 0.0)
    h = 0.5 * (entropy(a) + entropy(b))
    return float(mi / max(h, np.finfo(np.float64).eps))


def medoid_rows(labels, scores, n_clusters, metric, m):
    """Per cluster the rows by (score best first, then smaller row), at most ``m`` -> list of lists.  A torch sort."""
    labels, scores = torch.as_tensor(labels).long().cpu(), torch.as_tensor(scores).double().cpu()
    key = scores if metric == 'l2' else -scores
    order = torch.argsort(key, stable=True)                      # rows ascending within equal keys
    order = order[torch.argsort(labels[order], stable=True)]     # then grouped by cluster, keeping that order
    lab = labels[order].tolist()
    out = [[] for _ in range(n_clusters)]
    for r, k in zip(order.tolist(), lab):
        if len(out[k]) < m:
            out[k].append(r)
    return out


class Clustering:
    """The result of ``SubgraphIndex.cluster`` (fields: see the module's head)."""

    def __init__(self, labels, centers, sizes, scores, inertia, n_iter, converged, metric, center_aux=None, medoids=None,
                 label_counts=None, purity_=0.0, nmi_=0.0):
        self.labels = torch.as_tensor(labels).long()
        self.centers = torch.as_tensor(centers)
        self.sizes = torch.as_tensor(sizes).long()
        self.scores = torch.as_tensor(scores)
        self.inertia, self.n_iter, self.converged = float(inertia), int(n_iter), bool(converged)
        if metric not in METRICS:
            raise ValueError('metric must be one of %s, got %r' % (METRICS, metric))
        self.metric = metric
        self.center_aux = None if center_aux is None else torch.as_tensor(center_aux)
        K = self.centers.shape[0]
        self.medoids = [list(map(int, m)) for m in medoids] if medoids is not None else [[] for _ in range(K)]
        self.label_counts = [dict(c) for c in label_counts] if label_counts is not None else [{} for _ in range(K)]
        self.purity, self.nmi = float(purity_), float(nmi_)

    @property
    def n_clusters(self):
        return self.centers.shape[0]

    @property
    def majority(self):
        """Per cluster the most frequent label string (ties: the smaller string), None for a cluster without labels."""
        return [min(c, key=lambda s: (-c[s], s)) if c else None for c in self.label_counts]

    @property
    def cluster_purity(self):
        return [max(c.values()) / sum(c.values()) if c else 0.0 for c in self.label_counts]

    def assign(self, E):
        """(cluster (Q) int64, score (Q) float32) of new embeddings, through ``ops.topk_rows(E, centers, 1)`` with the
        centres' aux vector of the last iteration: the index's own rows get their ``labels`` back."""
        E = torch.as_tensor(E)
        if E.dim() != 2 or E.shape[1] != self.centers.shape[1]:
            raise ValueError('embeddings must be (Q, %d)' % self.centers.shape[1])
        E = E.to(self.centers.device)
        if self.metric == 'cosine':
            E = ops.kmeans_unit_rows(E)
        b_aux = self.center_aux if self.center_aux is not None else ops.topk_aux(self.centers, self.metric)
        s, i = ops.topk_rows(E, self.centers, 1, metric=self.metric, b_aux=b_aux)
        return i[:, 0], s[:, 0]

    # ------------------------------------------------------------------ files ------------
    def save(self, path):
        """One ``.npz`` without pickles, written under a temporary name and moved into place."""
        path = str(path)
        if not path.endswith('.npz'):
            raise ValueError('a clustering file is a .npz file')
        K = self.n_clusters
        med_ptr = np.zeros(K + 1, dtype=np.int64)
        np.cumsum([len(m) for m in self.medoids], out=med_ptr[1:])
        lc_ptr = np.zeros(K + 1, dtype=np.int64)
        np.cumsum([len(c) for c in self.label_counts], out=lc_ptr[1:])
        names = [s for c in self.label_counts for s in sorted(c)]
        tmp = path[:-4] + '.tmp%d.npz' % os.getpid()
        cpu = lambda t: t.detach().cpu().numpy()
        try:
            np.savez(tmp, labels=cpu(self.labels), centers=cpu(self.centers), sizes=cpu(self.sizes), scores=cpu(self.scores),
                     center_aux=cpu(self.center_aux) if self.center_aux is not None else np.zeros(0, dtype=np.float32),
                     inertia=np.asarray(self.inertia), n_iter=np.asarray(self.n_iter), converged=np.asarray(self.converged),
                     metric=np.asarray(self.metric), med_ptr=med_ptr,
                     med_rows=np.asarray([r for m in self.medoids for r in m], dtype=np.int64), lc_ptr=lc_ptr,
                     lc_names=np.asarray(names, dtype=np.str_) if names else np.zeros(0, dtype='<U1'),
                     lc_counts=np.asarray([c[s] for c in self.label_counts for s in sorted(c)], dtype=np.int64),
                     purity=np.asarray(self.purity), nmi=np.asarray(self.nmi))
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    @classmethod
    def load(cls, path, device='cpu'):
        with np.load(str(path), allow_pickle=False) as z:
            mp, mr, lp, ln, lc = z['med_ptr'], z['med_rows'], z['lc_ptr'], z['lc_names'], z['lc_counts']
            K = len(mp) - 1
            aux = z['center_aux']
            return cls(torch.from_numpy(z['labels']).to(device), torch.from_numpy(z['centers']).to(device),
                       torch.from_numpy(z['sizes']).to(device), torch.from_numpy(z['scores']).to(device), float(z['inertia']),
                       int(z['n_iter']), bool(z['converged']), str(z['metric']),
                       torch.from_numpy(aux).to(device) if len(aux) else None,
                       [mr[mp[k]:mp[k + 1]].tolist() for k in range(K)],
                       [{str(s): int(c) for s, c in zip(ln[lp[k]:lp[k + 1]], lc[lp[k]:lp[k + 1]])} for k in range(K)],
                       float(z['purity']), float(z['nmi']))

    def summary(self, arguments=None):
        """A JSON-ready dict: per cluster size, label counts, majority, purity and medoid rows; the overall figures."""
        maj, pur = self.majority, self.cluster_purity
        sizes = self.sizes.tolist()
        return {'n_clusters': self.n_clusters, 'metric': self.metric, 'inertia': self.inertia, 'n_iter': self.n_iter,
                'converged': self.converged, 'purity': self.purity, 'nmi': self.nmi, 'arguments': arguments or {},
                'clusters': [{'cluster': k, 'size': int(sizes[k]), 'label_counts': self.label_counts[k], 'majority': maj[k],
                              'purity': pur[k], 'medoids': self.medoids[k]} for k in range(self.n_clusters)]}


def label_figures(labels, label_lists, n_clusters):
    """(per-cluster counts of every label string, overall purity, nmi): purity and nmi take the FIRST label string of a row
    as its class; rows without a label form a class of their own."""
    labels = np.asarray(labels, dtype=np.int64)
    counts = [{} for _ in range(n_clusters)]
    for k, ls in zip(labels.tolist(), label_lists):
        for s in ls:
            counts[k][s] = counts[k].get(s, 0) + 1
    first = [ls[0] if ls else '' for ls in label_lists]
    names = {s: i for i, s in enumerate(sorted(set(first)))}
    classes = np.asarray([names[s] for s in first], dtype=np.int64)
    if len(labels) == 0:
        return counts, 0.0, 1.0
    return counts, purity(labels, classes), nmi(labels, classes)


def cluster_index(index, n_clusters, metric=None, medoids=5, **kmeans_args):
    """``SubgraphIndex.cluster``."""
    metric = index.metric if metric is None else metric
    if metric not in METRICS:
        raise ValueError('clustering takes the metrics %s, got %r' % (METRICS, metric))
    if int(medoids) < 0:
        raise ValueError('medoids must not be negative')
    res = ops.kmeans(index.embeddings, n_clusters, metric=metric, **kmeans_args)
    labels = res['assign'].long()
    K = res['centers'].shape[0]
    counts, pur, mi = label_figures(labels.cpu().numpy(), index.labels, K)
    return Clustering(labels, res['centers'], res['sizes'], res['score'], res['inertia'], res['n_iter'], res['converged'],
                      metric, res['c_aux'], medoid_rows(labels, res['score'], K, metric, int(medoids)), counts, pur, mi)


# ---------------------------------------------------------------------- files, CLI --------
def format_line(split, row, cluster, score, nodes, label_strings):
    """``split<TAB>row<TAB>cluster<TAB>score<TAB>n1-n2-...<TAB>label[-label]`` (9 significant digits: a float32 survives)."""
    return '%s\t%d\t%d\t%.9g\t%s\t%s' % (split, row, cluster, float(score), '-'.join(str(int(n)) for n in nodes),
                                         LABEL_SEP.join(label_strings))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Cluster the subgraph embeddings of a checkpoint with k-means on the device')
    cli.add_run_arguments(ap)
    ap.add_argument('-n_clusters', type=int, required=True)
    ap.add_argument('-out', type=str, required=True, help='text file: a header, then %s per row' % HEADER.replace('\t', '<TAB>'))
    ap.add_argument('-summary', type=str, default=None, help='a .json file: per-cluster sizes, label counts, purity, medoids')
    ap.add_argument('-metric', type=str, default='cosine', help='cosine or l2')
    ap.add_argument('-splits', type=str, default=','.join(SPLITS), help='the splits whose subgraphs are clustered, comma-separated')
    ap.add_argument('-index', type=str, default=None, help='a .npz index file: loaded if it exists, else built and saved there')
    ap.add_argument('-init', type=str, default='k-means++', help='k-means++ or random')
    ap.add_argument('-n_init', type=int, default=1)
    ap.add_argument('-max_iter', type=int, default=100)
    ap.add_argument('-seed', type=int, default=0)
    ap.add_argument('-medoids', type=int, default=5, help='typical rows listed per cluster')
    ap.add_argument('-subgraphs', type=str, default=None, help='requests, one per line (n1-n2-...): embedded and assigned too')
    ap.add_argument('-batch_size', type=int, default=None, help='chunk the forward passes (default: one batch)')
    args = ap.parse_args(argv)
    if args.n_clusters < 1:
        ap.error('-n_clusters must be at least 1')
    if args.metric not in METRICS:
        ap.error('-metric must be one of %s' % ', '.join(METRICS))
    if args.init not in INITS:
        ap.error('-init must be one of %s' % ', '.join(INITS))
    if args.n_init < 1 or args.max_iter < 1:
        ap.error('-n_init and -max_iter must be at least 1')
    if args.medoids < 0:
        ap.error('-medoids must not be negative')
    args.splits = cli.parse_splits(ap, args.splits)
    cli.require_positive(ap, args, ('batch_size',))
    if args.index is not None and not args.index.endswith('.npz'):
        ap.error('-index takes a .npz file name')
    if args.summary is not None and not args.summary.endswith('.json'):
        ap.error('-summary takes a .json file name')
    files = [f for f in (args.out, args.summary, args.index, args.subgraphs) if f is not None]
    if len(set(files)) != len(files):
        ap.error('-out, -summary, -index and -subgraphs must be different files')
    return args


def main(argv=None):
    args = parse_args(argv)
    from .predict import read_requests
    requests = read_requests(args.subgraphs) if args.subgraphs is not None else None
    p = cli.open_predictor(args)
    index = cli.open_index(p, args)
    cl = index.cluster(args.n_clusters, metric=args.metric, medoids=args.medoids, init=args.init, n_init=args.n_init,
                       max_iter=args.max_iter, seed=args.seed)
    labels, scores = cl.labels.cpu().numpy(), cl.scores.cpu().numpy()

    def lines():                                                         # formed while -out is written: the rows, then the requests
        for j in range(len(index)):
            sp, row, nodes, ls = index.describe(j)
            yield format_line(sp, row, labels[j], scores[j], nodes, ls)
        if requests is not None:
            res = p.predict(requests, batch_size=args.batch_size, return_embeddings=True)
            k, s = cl.assign(res['embeddings'].detach().float().contiguous())
            k, s = k.cpu().numpy(), s.cpu().numpy()
            for i, nodes in enumerate(requests):
                yield format_line('request', i, k[i], s[i], nodes, [])
    cli.write_lines(args.out, lines(), HEADER)
    if args.summary is not None:
        arguments = {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(args).items()}
        tmp = args.summary[:-5] + '.tmp%d.json' % os.getpid()
        with open(tmp, 'w') as f:
            json.dump(cl.summary(arguments), f, indent=1, sort_keys=True)
        os.replace(tmp, args.summary)
    return cl


if __name__ == '__main__':
    main()

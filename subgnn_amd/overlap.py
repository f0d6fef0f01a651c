"""Which known subgraphs share nodes with a subgraph, and do the splits leak?  Node-overlap search over a subgraph dataset.

Every other comparison in this package goes through the model; this one compares subgraphs by the nodes they hold
(``SubgraphIndex.overlaps`` / ``self_overlaps`` -> ops.overlap_topk, csrc/overlap.hip): integers throughout, an exact order, no
model and no checkpoint.

    python -m subgnn_amd.overlap (-index FILE.npz | DATASET_DIR) -out FILE [-subgraphs FILE] [-k 10]
                                 [-measure jaccard|containment|coverage|count] [-splits train,val,test] [-summary FILE.json]

``DATASET_DIR`` holds a ``subgraphs.pth``; ``-index`` takes a file ``SubgraphIndex.save`` wrote.  With ``-subgraphs`` (one
request per line, ``n1-n2-...``) the best rows of every request are listed, without it every row's best other rows.
``-summary`` answers the leak question for every ordered pair of different splits: how many rows of the first have an identical
row in the second, how many a best Jaccard of at least 1/2, and the mean best Jaccard.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import cli, ops
from .neighbors import LABEL_SEP, SPLITS, SubgraphIndex

MEASURES = tuple(ops.OVERLAP_MEASURES)
HEADER = 'request\trank\tscore\tshared\tsplit\trow\tsubgraph\tlabel'


def format_line(request, rank, score, shared, split, row, nodes, label_strings):
    """``request<TAB>rank<TAB>score<TAB>shared<TAB>split<TAB>row<TAB>n1-n2-...<TAB>label[-label]`` (9 significant digits: a
    float32 survives the round trip)."""
    return '%d\t%d\t%.9g\t%d\t%s\t%d\t%s\t%s' % (request, rank, float(score), int(shared), split, row,
                                                '-'.join(str(int(n)) for n in nodes), LABEL_SEP.join(label_strings))


def index_of_dataset(path, splits=SPLITS):
    """The subgraphs of ``path``/subgraphs.pth (subgraph_utils.read_subgraphs) of the named splits as a SubgraphIndex without
    embeddings: node lists, label strings, split and row within the split."""
    from . import subgraph_utils
    sub_f = os.path.join(str(path), 'subgraphs.pth')
    tr, trl, va, val, te, tel = subgraph_utils.read_subgraphs(sub_f)
    names = subgraph_utils.label_names(sub_f)
    parts = {'train': (tr, trl), 'val': (va, val), 'test': (te, tel)}
    subs, labels, where, rows = [], [], [], []
    for sp in splits:
        own, lab = parts[sp]
        lab = lab.reshape(-1).tolist() if isinstance(lab, torch.Tensor) else lab
        for i, sg in enumerate(own):
            ks = lab[i] if isinstance(lab[i], (list, tuple)) else [lab[i]]
            subs.append(sg)
            labels.append([names[int(x)] for x in ks])
            where.append(sp)
            rows.append(i)
    return SubgraphIndex(torch.zeros((len(subs), 0), dtype=torch.float32), subs, labels, where, rows)


def restrict(index, splits):
    """The rows of ``index`` whose split is one of ``splits`` (all rows where the index names no splits)."""
    keep = [i for i, s in enumerate(index.splits) if s in splits or s == '']
    if len(keep) == len(index):
        return index
    return SubgraphIndex(index.embeddings[keep], [index.subgraphs[i] for i in keep], [index.labels[i] for i in keep],
                         [index.splits[i] for i in keep], [index.rows[i] for i in keep], index.metric, index.checkpoint)


def lines_of(index, res):
    """The output lines of an ``overlaps`` / ``self_overlaps`` result (without the header); a filler has split '' and row -1."""
    rows, inter, scores = (res[k].cpu().numpy() for k in ('rows', 'inter', 'scores'))
    out = []
    for i in range(rows.shape[0]):
        for r in range(rows.shape[1]):
            j = int(rows[i, r])
            if j < 0:
                out.append(format_line(i, r, 0.0, 0, '', -1, [], []))
            else:
                out.append(format_line(i, r, scores[i, r], inter[i, r], *index.describe(j)))
    return out


def split_summary(index, splits):
    """For every ordered pair of different splits among ``splits`` that the index holds: ``rows`` of the first, how many of
    them have an ``identical`` row (the same node set) in the second, how many a best Jaccard >= 1/2 (``jaccard_ge_half``;
    compared in integers), and ``mean_best_jaccard`` (0 for a row that shares nothing) -> list of dicts."""
    dev = index._overlap_device()
    sets = {sp: [sorted(set(index.subgraphs[i])) for i in range(len(index)) if index.splits[i] == sp] for sp in splits}
    ragged = {sp: ops.Ragged.from_lists(s, dev) for sp, s in sets.items() if s}
    banks = {sp: ops.SetBank(r) for sp, r in ragged.items()}
    out = []
    for a in splits:
        for b in splits:
            if a == b or a not in ragged or b not in ragged:
                continue
            rows, inter, _touched, _scores = ops.overlap_topk(ragged[a], banks[b], 1, 'jaccard')
            i = inter[:, 0].long()
            nq, nb = ragged[a].lengths, banks[b].sizes[rows[:, 0].clamp_min(0)]
            union = nq + nb - i
            met = i > 0
            best = torch.where(met, i.double() / union.clamp_min(1).double(), torch.zeros_like(i, dtype=torch.float64))
            out.append({'first': a, 'second': b, 'rows': int(i.numel()), 'identical': int((met & (i == union)).sum()),
                        'jaccard_ge_half': int((met & (2 * i >= union)).sum()), 'mean_best_jaccard': float(best.mean())})
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Subgraphs of a dataset that share nodes with requested subgraphs, or with each other')
    ap.add_argument('dataset', type=str, nargs='?', default=None, help='a dataset directory: its subgraphs.pth is read')
    ap.add_argument('-index', type=str, default=None, help='a .npz index file (SubgraphIndex.save) in place of a dataset directory')
    ap.add_argument('-out', type=str, required=True, help='text file: a header, then ' + HEADER.replace('\t', '<TAB>'))
    ap.add_argument('-subgraphs', type=str, default=None,
                    help="one request per line: n1-n2-... (further columns ignored); without it every row's best other rows")
    ap.add_argument('-k', type=int, default=10, help='rows per request (default 10)')
    ap.add_argument('-measure', type=str, default='jaccard', help=', '.join(MEASURES))
    ap.add_argument('-splits', type=str, default=','.join(SPLITS), help='the splits that are searched, comma-separated')
    ap.add_argument('-summary', type=str, default=None, help='a .json file: overlap between every ordered pair of splits')
    args = ap.parse_args(argv)
    if (args.index is None) == (args.dataset is None):
        ap.error('give a dataset directory or -index FILE.npz, not both')
    if args.index is not None and not args.index.endswith('.npz'):
        ap.error('-index takes a .npz file name')
    if args.k < 1 or args.k > 64:
        ap.error('-k must be in 1 .. 64')
    if args.measure not in MEASURES:
        ap.error('-measure must be one of %s' % ', '.join(MEASURES))
    args.splits = tuple(s for s in args.splits.split(',') if s)
    if not args.splits or any(s not in SPLITS for s in args.splits) or len(set(args.splits)) != len(args.splits):
        ap.error('-splits takes a comma-separated list of %s, each once' % ', '.join(SPLITS))
    if args.summary is not None and not args.summary.endswith('.json'):
        ap.error('-summary takes a .json file name')
    files = [f for f in (args.index, args.out, args.subgraphs, args.summary) if f is not None]
    if len(set(files)) != len(files):
        ap.error('-index, -out, -subgraphs and -summary must be different files')
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.index is not None:
        index = restrict(SubgraphIndex.load(args.index), args.splits)
    else:
        index = index_of_dataset(args.dataset, args.splits)
    if len(index) == 0:
        raise SystemExit('no subgraph in the splits %s' % ','.join(args.splits))
    if args.subgraphs is not None:
        from .predict import read_requests
        res = index.overlaps(read_requests(args.subgraphs), args.k, args.measure)
    else:
        res = index.self_overlaps(args.k, args.measure)
    cli.write_lines(args.out, lines_of(index, res), HEADER)
    if args.summary is not None:
        with open(args.summary, 'w') as f:
            json.dump({'splits': list(args.splits), 'pairs': split_summary(index, args.splits)}, f, indent=1)
            f.write('\n')
    return res


if __name__ == '__main__':
    main()

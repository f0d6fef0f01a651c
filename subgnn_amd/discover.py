"""Where in the graph are further subgraphs of a class: candidate subgraphs sampled around seed nodes on the device, scored by
the trained model and ranked.

Every seed gets ``per_seed`` candidates: the node sets of random walks with restarts from it (ops.seeded_walk_sets), each grown
until it holds its target size.  A candidate is connected and holds its seed.  Candidates are prepared as any request is
(Predictor.prepare_sets: every draw keyed by the content of the drawing set) and sent through the model; a node set that was
sampled twice is scored once.  The score of a candidate is the mean over draws of the target class's logit.

A candidate's draws are those of its item number (seed index * per_seed + candidate) on the tape, whatever else a launch
samples, so only scalars are kept per candidate while the chunks go by: the node lists of the candidates that are returned are
sampled again from their item numbers afterwards.

    python -m subgnn_amd.discover -config_path CONFIG -restoreModelPath DIR [-restoreModelName F] -seeds FILE|all -out FILE
                                  [-target LABEL] [-sizes 5,10,20] [-per_seed 16] [-restart 0.15] [-max_steps N] [-draws E]
                                  [-top N] [-top_per_seed N] [-novel] [-batch_size B] [-sample_seed S]
                                  [-max_overlap T] [-overlap_pool M]

``-max_overlap T`` makes the list diverse: of the ranked candidates (the first ``-overlap_pool`` of them) one is dropped when a
better candidate that is kept shares more than T of their joint nodes with it (Jaccard; ops.overlap_diverse, csrc/overlap.hip).
"""
import argparse

import numpy as np
import torch

from . import cli, ops, scoring, tape
from .suggest import read_pool

ALL = 'all'
HEADER = 'rank\tseed\tscore\tscore_std\tprob\tsubgraph\tlabel\tknown'


def map_seeds(p, seeds):
    """Seed ids in the dataset's numbering (or ``'all'``: every node with an edge) -> the model's, as ``suggest.map_pool`` maps a
    pool: without the ids that are no nodes of the graph, ascending, without repeats -> int32 numpy array.  None left is an
    error."""
    if isinstance(seeds, str):
        if seeds != ALL:
            raise ValueError("seeds must be 'all' or a sequence of node ids, got %r" % (seeds,))
        flat = np.nonzero(p.freeze()['degree'] > 0)[0].astype(np.int32)
    else:
        flat = p.map_subgraphs([[int(v) for v in seeds]], allow_empty=True)[1]
    if flat.shape[0] == 0:
        raise ValueError('seeds: no node of the graph among them')
    return flat


def known_keys(p):
    """The content keys (ops.set_keys) of the model's own train / val / test subgraphs, mapped as a request would be -> sorted
    int64 device tensor.  Computed once and kept with the frozen facts."""
    f = p.freeze()
    if 'known_keys' not in f:
        m = p.model
        dev = m.device
        own = [[v - 1 for v in sg] for sp in ('train', 'val', 'test') for sg in getattr(m, sp + '_sub_G')]
        ptr, flat = p.map_subgraphs(own, allow_empty=True)
        if flat.shape[0] == 0:
            flat = np.zeros(1, dtype=np.int32)
        keys = ops.set_keys(ops.Ragged(torch.from_numpy(ptr).to(dev), torch.from_numpy(flat).to(dev)))
        f['known_keys'] = torch.unique(keys[torch.from_numpy(ptr[1:] > ptr[:-1]).to(dev)])
    return f['known_keys']


def rank_order(score, item):
    """The candidates in the order of the result: descending ``score``, then ascending item number; NaN last -> index array."""
    score, item = np.asarray(score, dtype=np.float64), np.asarray(item, dtype=np.int64)
    nan = np.isnan(score)
    return np.lexsort((item, np.where(nan, 0.0, -score), nan))


def select(order, seed_index, top=None, top_per_seed=None):
    """Of the ranked candidates ``order`` (indices) at most ``top_per_seed`` of every seed, then the first ``top`` -> index array."""
    order = np.asarray(order, dtype=np.int64)
    if top_per_seed is not None and order.size:
        s = np.asarray(seed_index, dtype=np.int64)[order]
        by_seed = np.argsort(s, kind='stable')                                          # ranked within every seed
        starts = np.flatnonzero(np.r_[True, s[by_seed][1:] != s[by_seed][:-1]])
        place = np.arange(order.size) - np.repeat(starts, np.diff(np.r_[starts, order.size]))
        keep = np.zeros(order.size, dtype=bool)
        keep[by_seed] = place < top_per_seed
        order = order[keep]
    return order if top is None else order[:top]


def diverse(g, seeds_t, walk, c, pool, max_overlap, top):
    """Of the ranked candidates ``pool`` (indices into the kept scalars ``c``) those the greedy selection accepts, in rank order
    -> (index array, the number of pool candidates it suppressed).  Their node lists are sampled again from their item numbers
    (and checked against the scored keys), then ops.overlap_diverse runs once."""
    if pool.size == 0:
        return pool, 0
    sel = torch.from_numpy(pool).to(seeds_t.device)
    again = ops.seeded_walk_sets(g, seeds_t, item_ids=c['item'][sel].contiguous(), **walk)
    if not torch.equal(again.keys, c['keys'][sel]):
        raise RuntimeError('discover: the regenerated candidates are not the scored ones')
    if bool((again.lengths == 0).any()):
        raise RuntimeError('discover: a regenerated candidate is empty')
    accepted, n, by = ops.overlap_diverse(again.sets, max_overlap, pool.size if top is None else top)
    n = int(n.item())
    return pool[accepted[:n].cpu().numpy()], int((by >= 0).sum().item())


def discover(p, seeds, sizes=(8,), per_seed=16, target=None, restart=0.15, max_steps=None, draws=1, top=100, top_per_seed=None,
             novel=False, batch_size=None, max_variants=65536, sample_seed=None, max_overlap=None, overlap_pool=4096):
    """``Predictor.discover``.  -> dict, for the returned candidates in rank order (device tensors unless said otherwise):
      ``subgraphs`` node lists in the dataset's numbering, ascending (Python lists); ``seed`` (N,) int64, dataset ids;
      ``item``      (N,) int64: seed index * per_seed + candidate, the number the candidate's draws are keyed by;
      ``keys``      (N,) int64 holding the uint64 content keys; ``steps`` (N,) int32, the walk's steps;
      ``logits``    (N, K) float32, mean over draws; ``score`` the target's mean logit, ``score_std`` its sample standard
                    deviation over draws (0 for one), ``prob`` the target's mean probability (softmax; sigmoid for a multi-label
                    model); ``labels`` of the mean logits, as ``predict`` forms them; ``target`` (N,) int64;
      ``known``     (N,) bool: the node set is one of the model's own train / val / test subgraphs;
      ``n_sampled`` the candidates drawn, ``n_distinct`` the different node sets among them (ints).
    ``seeds``: node ids in the dataset's numbering, or ``'all'``; ids that are no nodes of the graph and repeats are dropped.
    ``sizes``: the target sizes of a seed's ``per_seed`` candidates, taken cyclically.  ``target``: an int class, or None: every
    candidate is scored by the class of its own largest mean logit.  ``novel=True`` leaves out the known sets before ranking.
    Order: descending score, then ascending item; NaN last.  ``top_per_seed`` keeps that many of every seed, then ``top`` cuts
    the list (None: no cut).  Of a node set sampled more than once the smallest item stands for it.  The items are sampled and
    scored in chunks of at most ``max_variants``; ``sample_seed`` is the tape seed of the walks (default: the model's).  The
    model's own splits stay as ``Predictor.prepare`` leaves them.
    ``max_overlap`` (None, or a Jaccard threshold in [0, 1]): the list is made diverse.  The candidates are ranked and
    ``top_per_seed`` applied as above; of the first ``overlap_pool`` of them, in rank order, one is dropped when an earlier one that
    is kept shares MORE than ``max_overlap`` of their joint nodes with it (ops.overlap_diverse: greedy, exact in integers), until
    ``top`` are kept.  The result gains ``n_suppressed`` (int): the candidates of the pool that were dropped for it."""
    per_seed, E = scoring.positive(per_seed, 'per_seed'), scoring.positive(draws, 'draws')
    max_variants = scoring.positive(max_variants, 'max_variants')
    top = None if top is None else scoring.positive(top, 'top')
    top_per_seed = None if top_per_seed is None else scoring.positive(top_per_seed, 'top_per_seed')
    if batch_size is not None:
        batch_size = scoring.positive(batch_size, 'batch_size')
    if max_overlap is not None:
        ops.overlap_threshold(max_overlap)
        overlap_pool = scoring.positive(overlap_pool, 'overlap_pool')
    m = p.model
    K, dev, g = m.num_classes, m.device, m.networkx_graph
    if target is not None:
        if isinstance(target, bool) or not isinstance(target, (int, np.integer)):
            raise ValueError('target: an int class or None')
        if not 0 <= int(target) < K:
            raise ValueError('target outside the classes 0 .. %d' % (K - 1))
    seeds_np = map_seeds(p, seeds)
    seeds_t = torch.from_numpy(seeds_np).to(dev)
    f = p.freeze()
    walk = dict(sizes=sizes, per_seed=per_seed, restart=restart, max_steps=max_steps,
                seed=f['seed'] if sample_seed is None else int(sample_seed), stream_id=tape.stream_id(tape.STREAM_DISCOVER, 'predict'))
    known_sorted = known_keys(p)
    total = seeds_np.shape[0] * per_seed
    seen = torch.empty(0, dtype=torch.int64, device=dev)
    kept = {k: [] for k in ('item', 'keys', 'steps', 'logits', 'score', 'score_std', 'prob', 'target')}
    for lo in range(0, total, max_variants):
        hi = min(lo + max_variants, total)
        res = ops.seeded_walk_sets(g, seeds_t, item_base=lo, n_items=hi - lo, **walk)
        first = ops.first_occurrence_mask(res.keys.view(1, -1)).view(-1).bool() & ~torch.isin(res.keys, seen)
        rows = first.nonzero().view(-1)
        if rows.numel() == 0:
            continue
        keys = res.keys[rows].contiguous()
        seen = torch.cat((seen, keys))
        packed = ops.Ragged.from_padded(res.nodes[rows].long())
        z = scoring.variant_logits(p, packed, keys, K, E, batch_size, rows.numel())                     # (E, n, K)
        mean = z.mean(dim=0)
        tgt = mean.argmax(dim=-1) if target is None else torch.full((rows.numel(),), int(target), dtype=torch.int64, device=dev)
        zt, pt = scoring.target_columns(p, z, tgt)                                                      # (E, n)
        score, score_std = scoring.mean_std(zt)
        kept['item'].append(rows + lo)
        kept['keys'].append(keys)
        kept['steps'].append(res.steps[rows])
        kept['logits'].append(mean)
        kept['score'].append(score)
        kept['score_std'].append(score_std)
        kept['prob'].append(pt.mean(dim=0))
        kept['target'].append(tgt)
    c = {k: torch.cat(v) for k, v in kept.items()}
    c['known'] = torch.isin(c['keys'], known_sorted)
    n_distinct = int(c['item'].numel())
    if novel:
        fresh = (~c['known']).nonzero().view(-1)
        c = {k: v[fresh] for k, v in c.items()}
    item = c['item'].cpu().numpy()
    n_suppressed = None
    if max_overlap is None:
        chosen = select(rank_order(c['score'].cpu().numpy(), item), item // per_seed, top, top_per_seed)
    else:
        pool = select(rank_order(c['score'].cpu().numpy(), item), item // per_seed, overlap_pool, top_per_seed)
        chosen, n_suppressed = diverse(g, seeds_t, walk, c, pool, max_overlap, top)
    sel = torch.from_numpy(chosen).to(dev)
    out = {k: v[sel] for k, v in c.items()}
    out['seed'] = seeds_t[out['item'] // per_seed].long() - 1
    out['labels'] = torch.sigmoid(out['logits']) > 0.5 if m.multilabel else out['logits'].argmax(dim=-1)
    # the node lists of the returned candidates, sampled again from their item numbers
    again = ops.seeded_walk_sets(g, seeds_t, item_ids=out['item'].contiguous(), **walk)
    if not torch.equal(again.keys, out['keys']):
        raise RuntimeError('discover: the regenerated candidates are not the scored ones')
    nodes, lens = again.nodes.cpu().numpy(), again.lengths.cpu().numpy()
    out['subgraphs'] = [(nodes[i, :lens[i]] - 1).tolist() for i in range(nodes.shape[0])]
    out['n_sampled'], out['n_distinct'] = total, n_distinct
    if n_suppressed is not None:
        out['n_suppressed'] = n_suppressed
    return out


# ---------------------------------------------------------------------- files, CLI --------
def format_line(rank, seed, score, score_std, prob, nodes, label_strings, known):
    """``rank\\tseed\\tscore\\tscore_std\\tprob\\tn1-n2-...\\tlabel[-label]\\tknown(0|1)``: ids in the dataset's numbering, the
    floats with 9 significant digits (a float32 survives the round trip)."""
    return '%d\t%d\t%s\t%s\t%s\t%s\t%s\t%d' % (rank, int(seed), '%.9g' % float(score), '%.9g' % float(score_std), '%.9g' % float(prob),
                                               '-'.join(str(int(v)) for v in nodes), '-'.join(label_strings), 1 if known else 0)


def lines_of(p, res):
    """The output lines of a ``discover`` result (without the header)."""
    seed, score, std, prob, known = (res[k].cpu().numpy() for k in ('seed', 'score', 'score_std', 'prob', 'known'))
    labels = res['labels'].cpu()
    return [format_line(r, seed[r], score[r], std[r], prob[r], nodes, p.names_of(labels[r]), known[r])
            for r, nodes in enumerate(res['subgraphs'])]


def parse_sizes(text):
    """``5,10,20`` -> [5, 10, 20]."""
    try:
        sizes = [int(w) for w in text.split(',')]
    except ValueError:
        raise ValueError('%r: sizes are integers separated by commas' % text) from None
    if not sizes or min(sizes) < 1 or max(sizes) > ops.SEEDED_MAX_SIZE:
        raise ValueError('sizes are in 1 .. %d' % ops.SEEDED_MAX_SIZE)
    return sizes


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Sample candidate subgraphs around seed nodes and rank them by a class, from a checkpoint')
    cli.add_run_arguments(ap)
    ap.add_argument('-seeds', type=str, required=True, help="a file of node ids (whitespace separated), or 'all': every node with an edge")
    ap.add_argument('-out', type=str, required=True, help='text file: a header, then ' + HEADER.replace('\t', '<TAB>'))
    ap.add_argument('-target', type=str, default=None,
                    help='label string of subgraphs.pth to score for (default: per candidate, the class of the largest mean logit)')
    ap.add_argument('-sizes', type=str, default='8', help='target sizes of a seed\'s candidates, taken cyclically (default 8)')
    ap.add_argument('-per_seed', type=int, default=16, help='candidates per seed (default 16)')
    ap.add_argument('-restart', type=float, default=0.15, help='probability of a step back to the seed (default 0.15)')
    ap.add_argument('-max_steps', type=int, default=None, help='steps of a walk at most (default 16 x the largest size)')
    ap.add_argument('-draws', type=int, default=1, help='anchor draws to average over (default 1: the answer of predict)')
    ap.add_argument('-top', type=int, default=100, help='at most this many lines (default 100)')
    ap.add_argument('-top_per_seed', type=int, default=None, help='at most this many candidates of one seed')
    ap.add_argument('-novel', action='store_true', help="leave out the dataset's own subgraphs")
    ap.add_argument('-batch_size', type=int, default=None, help='chunk the forward pass (default: one batch)')
    ap.add_argument('-sample_seed', type=int, default=None, help='tape seed of the walks (default: the run\'s seed)')
    ap.add_argument('-max_overlap', type=float, default=None,
                    help='drop a candidate that shares more than this Jaccard fraction of nodes with a better kept one (default: keep all)')
    ap.add_argument('-overlap_pool', type=int, default=4096, help='ranked candidates that -max_overlap looks at (default 4096)')
    args = ap.parse_args(argv)
    cli.require_positive(ap, args, ('per_seed', 'draws', 'top', 'top_per_seed', 'batch_size', 'overlap_pool'))
    if args.max_steps is not None and args.max_steps < 0:
        ap.error('-max_steps must not be negative')
    if not 0.0 <= args.restart <= 1.0:
        ap.error('-restart must be in [0, 1]')
    if args.max_overlap is not None and not 0.0 <= args.max_overlap <= 1.0:
        ap.error('-max_overlap must be in [0, 1]')
    try:
        args.sizes = parse_sizes(args.sizes)
    except ValueError as e:
        ap.error('-sizes: %s' % e)
    if args.out == args.seeds:
        ap.error('-seeds and -out must be different files')
    return args


def main(argv=None):
    args = parse_args(argv)
    seeds = ALL if args.seeds == ALL else read_pool(args.seeds)
    p = cli.open_predictor(args)
    res = p.discover(seeds, sizes=args.sizes, per_seed=args.per_seed, target=cli.label_index(p, args.target), restart=args.restart,
                     max_steps=args.max_steps, draws=args.draws, top=args.top, top_per_seed=args.top_per_seed, novel=args.novel,
                     batch_size=args.batch_size, sample_seed=args.sample_seed, max_overlap=args.max_overlap,
                     overlap_pool=args.overlap_pool)
    cli.write_lines(args.out, lines_of(p, res), HEADER)
    return res


if __name__ == '__main__':
    main()

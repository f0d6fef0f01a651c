"""Which node would make this subgraph more (or less) of a class if it were added: add-one-candidate scoring, and its greedy use.

For a request S and each of its candidates v (the k-hop border of S, or a pool of ids shared by all requests, without S's
members) the variant S + v is built on the device (ops.insertion_sets), prepared as any request is (Predictor.prepare_sets:
every draw is keyed by the CONTENT of the drawing set, so a component of S that v does not touch has the parent's anchors and
similarities bit for bit) and sent through the model.  The gain of v is the rise of the target class's logit,

    gain_logit(v) = mean over draws d of  z_target(S + v; d) - z_target(S; d),

both terms at the same draw d of the request's own anchors (``epoch_offset=d``); ``gain_std`` is the sample standard deviation
of that per-draw difference.  Every candidate has a variant.  ``grow`` adds the best candidate round by round.

    python -m subgnn_amd.suggest -config_path CONFIG -restoreModelPath DIR [-restoreModelName F] -subgraphs FILE -out FILE
                                 [-candidates border|FILE] [-hops K] [-target LABEL] [-draws E] [-top N] [-batch_size B]
                                 [-grow STEPS [-min_gain G]]
"""
import argparse

import numpy as np
import torch

from . import cli, ops, scoring

BORDER = 'border'
HEADER = 'request\tcandidate\tgain_logit\tgain_std\tgain_prob\tlabel_with'
GROW_HEADER = 'request\tstep\tadded\tgain_logit\tgain_std\tlabel_after'


def map_pool(p, candidates):
    """A pool of node ids in the dataset's numbering -> the model's, as ``Predictor.map_subgraphs`` maps a list: without the ids
    that are no nodes of the graph, ascending, without repeats -> int32 numpy array.  A pool with nothing left is an error."""
    ids = [int(v) for v in candidates]
    try:
        _ptr, flat = p.map_subgraphs([ids])
    except ValueError:
        raise ValueError('candidates: the pool holds no node of the graph') from None
    return flat


def candidate_rows(p, sets, candidates=BORDER, hops=1):
    """The candidate rows of the request ``sets`` -> (ops.Ragged of ascending rows, shared): the ``hops``-hop border of every
    set (one row per set), or the mapped pool (ONE row that every set takes)."""
    if isinstance(candidates, str):
        if candidates != BORDER:
            raise ValueError("candidates must be 'border' or a sequence of node ids, got %r" % (candidates,))
        g = p.model.networkx_graph
        if hops == 1 and ops.khop1_applies(g, sets.n):
            kept = ops.khop1_borders_sorted(g, sets)
            return ops.Ragged(kept.ptr, kept.ids), False
        return ops.sort_ragged(ops.khop_border(g, sets, hops)), False
    flat = map_pool(p, candidates)
    dev = sets.ptr.device
    ptr = torch.tensor([0, flat.shape[0]], dtype=torch.int64, device=dev)
    return ops.Ragged(ptr, torch.from_numpy(flat).to(dev), max_len=int(flat.shape[0])), True


def suggest(p, subgraphs, candidates=BORDER, hops=1, target=None, draws=1, batch_size=None, max_variants=65536):
    """``Predictor.suggest``.  -> dict:
      ``subgraphs``, ``logits``, ``probabilities``, ``labels`` (and the ``*_mean`` / ``*_std`` keys for ``draws > 1``): the
                    base request, as ``predict(draws=draws)`` gives them;
      ``target``    (R,) int64, the class per request: the argmax of the mean base logits (for a multi-label model too), or the
                    given int or sequence of R ints;
      ``ptr``       (R + 1,) int64: the candidates of request r are ``ptr[r]:ptr[r + 1]``, ascending by id;
      ``candidate_nodes`` (U,) int64, model ids;
      ``variant_logits`` (U, K): the logits of the request with the candidate, mean over draws; ``gain_logit``, ``gain_std`` (0
                    for one draw), ``gain_prob`` (U,): see the module's docstring; ``gain_prob`` is the same difference of the
                    target's probability (softmax; sigmoid for a multi-label model).
    ``candidates``: ``'border'`` -- the ``hops``-hop border of the request (none is no error: the request has no candidates)
    -- or a sequence of node ids in the dataset's numbering, a pool shared by all requests: ids that are no nodes of the graph
    are dropped, members of a request are skipped for that request.  The variants are prepared and forwarded in chunks of at
    most ``max_variants`` sets (a bound on memory, not a tuned number); ``batch_size`` chunks every forward pass.  The model's
    own splits stay as ``Predictor.prepare`` leaves them."""
    if isinstance(candidates, str) and candidates != BORDER:
        raise ValueError("candidates must be 'border' or a sequence of node ids, got %r" % (candidates,))
    hops = scoring.positive(hops, 'hops')
    E, max_variants = scoring.positive(draws, 'draws'), scoring.positive(max_variants, 'max_variants')
    if batch_size is not None:
        batch_size = scoring.positive(batch_size, 'batch_size')
    sets = p.request_sets(subgraphs)
    R, dev = sets.n, sets.ptr.device
    cand, shared = candidate_rows(p, sets, candidates, hops)
    out, base = p._predict_sets(sets, batch_size, False, E)                           # base: (E, R, K)
    K = base.shape[2]
    tgt = scoring.class_targets(target, base, R, K, dev)

    # the variants: every request with one of its candidates
    ins = ops.insertion_sets(sets, cand, shared)
    out.update({'target': tgt, 'ptr': ops.exclusive_scan(ins.variants), 'candidate_nodes': ins.cand.long()})

    var = scoring.variant_logits(p, ins.sets, ins.keys, K, E, batch_size, max_variants)           # (E, V, K)

    # per-variant differences, reduced on the device (the variants are the candidates, in order)
    parent = ins.parent.long()
    z_base, p_base = scoring.target_columns(p, base, tgt)
    z_var, p_var = scoring.target_columns(p, var, tgt[parent])
    out['variant_logits'] = var.mean(dim=0)
    out['gain_logit'], out['gain_std'] = scoring.mean_std(z_var - z_base[:, parent])
    out['gain_prob'] = (p_var - p_base[:, parent]).mean(dim=0)
    return out


# ---------------------------------------------------------------------- greedy growth -----
def choose(ptr, candidate_nodes, gain_logit, min_gain=0.0):
    """The candidate every request takes in one round of ``grow``: of its candidates ``ptr[r]:ptr[r + 1]`` the one of the largest
    ``gain_logit`` -- the smaller id on a tie -- if that gain is > ``min_gain``, else none -> list of R indices into the
    candidate arrays, -1 where the request stops.  Arrays or sequences on the host; a NaN gain is never taken."""
    ids, gain = np.asarray(candidate_nodes), np.asarray(gain_logit, dtype=np.float64)
    picks = []
    for r in range(len(ptr) - 1):
        best = -1
        for u in range(int(ptr[r]), int(ptr[r + 1])):
            if not gain[u] > min_gain:
                continue
            if best < 0 or gain[u] > gain[best] or (gain[u] == gain[best] and ids[u] < ids[best]):
                best = u
        picks.append(best)
    return picks


def grow(p, subgraphs, steps, target=None, min_gain=0.0, candidates=BORDER, hops=1, draws=1, batch_size=None):
    """``Predictor.grow``: for up to ``steps`` rounds ``suggest`` runs on the current sets and every request whose best candidate
    (``choose``) has ``gain_logit > min_gain`` takes it; a request without one stops, and the loop ends when all have.  The
    target of a request is fixed at round 0 (``target=None``: the argmax of its mean base logits then).  -> dict, per request:
      ``added``     the ids taken, in order, in the dataset's numbering; ``gain_logit`` / ``gain_std``: their gains;
      ``step_logits`` the (K,) logits of the request after each step (the chosen variant's, mean over draws);
      ``subgraphs`` the final sets in the dataset's numbering, ascending; ``logits`` (R, K): ``predict``'s of those;
      ``target``    (R,) int64."""
    steps = scoring.positive(steps, 'steps')
    min_gain = float(min_gain)
    R = len(subgraphs)
    current = [list(s) for s in subgraphs]
    added, gains, stds, step_logits = ([[] for _ in range(R)] for _ in range(4))
    active, tgt = list(range(R)), None
    for _round in range(steps):
        if not active:
            break
        res = suggest(p, [current[r] for r in active], candidates=candidates, hops=hops,
                      target=target if tgt is None else [tgt[r] for r in active], draws=draws, batch_size=batch_size)
        if tgt is None:
            tgt = res['target'].tolist()
        ids = res['candidate_nodes'].cpu().numpy()
        gl, gs = res['gain_logit'].cpu().numpy(), res['gain_std'].cpu().numpy()
        vl = res['variant_logits'].float().cpu()
        picks = choose(res['ptr'].tolist(), ids, gl, min_gain)
        still = []
        for i, r in enumerate(active):
            current[r] = [v - 1 for v in res['subgraphs'][i]]                         # the mapped set, dataset numbering
            u = picks[i]
            if u < 0:
                continue
            v = int(ids[u]) - 1
            current[r] = sorted(current[r] + [v])
            added[r].append(v)
            gains[r].append(float(gl[u]))
            stds[r].append(float(gs[u]))
            step_logits[r].append(vl[u].clone())
            still.append(r)
        active = still
    final = p.predict(current, batch_size=batch_size)
    if tgt is None:                                                                   # (no request: request_sets has raised)
        tgt = []
    return {'added': added, 'gain_logit': gains, 'gain_std': stds, 'step_logits': step_logits,
            'subgraphs': [[v - 1 for v in s] for s in final['subgraphs']], 'logits': final['logits'],
            'target': torch.tensor(tgt, dtype=torch.int64, device=final['logits'].device)}


# ---------------------------------------------------------------------- files, CLI --------
def candidate_order(gain_logit, candidate_ids):
    """The candidates of one request in the order of the output: descending ``gain_logit``, then ascending id."""
    return sorted(range(len(candidate_ids)), key=lambda u: (-float(gain_logit[u]), int(candidate_ids[u])))


def format_line(request, candidate, gain_logit, gain_std, gain_prob, label_strings):
    """``request\\tcandidate\\tgain_logit\\tgain_std\\tgain_prob\\tlabel_with``: ``candidate`` is a node id in the dataset's
    numbering, the floats have 9 significant digits (a float32 survives the round trip)."""
    return '%d\t%d\t%s\t%s\t%s\t%s' % (request, int(candidate), '%.9g' % float(gain_logit), '%.9g' % float(gain_std),
                                       '%.9g' % float(gain_prob), '-'.join(label_strings))


def format_grow_line(request, step, added, gain_logit, gain_std, label_strings):
    """``request\\tstep\\tadded\\tgain_logit\\tgain_std\\tlabel_after``."""
    return '%d\t%d\t%d\t%s\t%s\t%s' % (request, step, int(added), '%.9g' % float(gain_logit), '%.9g' % float(gain_std),
                                       '-'.join(label_strings))


def lines_of(p, res, top=None):
    """The output lines of a ``suggest`` result (without the header)."""
    ptr = res['ptr'].cpu().numpy()
    ids = res['candidate_nodes'].cpu().numpy()
    gl, gs, gp = (res[k].cpu().numpy() for k in ('gain_logit', 'gain_std', 'gain_prob'))
    vl = res['variant_logits'].float().cpu()
    lines = []
    for r in range(ptr.shape[0] - 1):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        for k in candidate_order(gl[lo:hi], ids[lo:hi])[:top]:
            u = lo + k
            lines.append(format_line(r, ids[u] - 1, gl[u], gs[u], gp[u], cli.predicted_names(p, vl[u])))
    return lines


def grow_lines_of(p, res):
    """The output lines of a ``grow`` result (without the header): one per request and accepted step."""
    return [format_grow_line(r, k, v, res['gain_logit'][r][k], res['gain_std'][r][k], cli.predicted_names(p, res['step_logits'][r][k]))
            for r, steps in enumerate(res['added']) for k, v in enumerate(steps)]


def read_pool(path):
    """A candidate file: node ids in the dataset's numbering, separated by whitespace or newlines -> list of ints."""
    out = []
    with open(path) as fin:
        for word in fin.read().split():
            try:
                out.append(int(word))
            except ValueError:
                raise ValueError('%s: %r is no node id' % (path, word)) from None
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Score the nodes a subgraph could gain (or grow it greedily), from a checkpoint')
    cli.add_run_arguments(ap)
    ap.add_argument('-subgraphs', type=str, required=True, help='one subgraph per line: n1-n2-... (further columns ignored)')
    ap.add_argument('-out', type=str, required=True, help='text file: a header, then ' + HEADER.replace('\t', '<TAB>') +
                    ' (with -grow: ' + GROW_HEADER.replace('\t', '<TAB>') + ')')
    ap.add_argument('-candidates', type=str, default=BORDER,
                    help="'border' (default: the -hops border of every request) or a file of node ids, a pool shared by all requests")
    ap.add_argument('-hops', type=int, default=1, help='depth of the border (default 1)')
    ap.add_argument('-target', type=str, default=None,
                    help='label string of subgraphs.pth to score for (default: per request, the class of the largest mean logit)')
    ap.add_argument('-draws', type=int, default=1, help='anchor draws to average over (default 1: the answer of predict)')
    ap.add_argument('-top', type=int, default=None, help='at most this many lines per request')
    ap.add_argument('-batch_size', type=int, default=None, help='chunk the forward pass (default: one batch)')
    ap.add_argument('-grow', type=int, default=None, metavar='STEPS', help='add the best candidate, for up to STEPS rounds')
    ap.add_argument('-min_gain', type=float, default=None, help='with -grow: a candidate is taken if its gain_logit is above this (default 0)')
    args = ap.parse_args(argv)
    cli.require_positive(ap, args, ('hops', 'draws', 'top', 'batch_size', 'grow'))
    if args.grow is None and args.min_gain is not None:
        ap.error('-min_gain applies to -grow')
    if args.grow is not None and args.top is not None:
        ap.error('-top applies to the candidate list, not to -grow')
    if args.min_gain is None:
        args.min_gain = 0.0
    if args.min_gain != args.min_gain:
        ap.error('-min_gain must be a number')
    if args.out == args.subgraphs or args.out == args.candidates:
        ap.error('-subgraphs, -candidates and -out must be different files')
    return args


def main(argv=None):
    args = parse_args(argv)
    from .predict import read_requests
    requests = read_requests(args.subgraphs)
    pool = BORDER if args.candidates == BORDER else read_pool(args.candidates)
    p = cli.open_predictor(args)
    target = cli.label_index(p, args.target)
    if args.grow is not None:
        res = p.grow(requests, args.grow, target=target, min_gain=args.min_gain, candidates=pool, hops=args.hops,
                     draws=args.draws, batch_size=args.batch_size)
        header, lines = GROW_HEADER, grow_lines_of(p, res)
    else:
        res = p.suggest(requests, candidates=pool, hops=args.hops, target=target, draws=args.draws, batch_size=args.batch_size)
        header, lines = HEADER, lines_of(p, res, args.top)
    cli.write_lines(args.out, lines, header)
    return res


if __name__ == '__main__':
    main()

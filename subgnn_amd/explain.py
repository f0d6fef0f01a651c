"""Which members of a subgraph made the model say that: leave-one-out attribution over nodes or components.

For a request S and each of its units u (a node, or a connected component of S) the variant S \\ u is built on the device
(ops.occlusion_sets), prepared as any request is (Predictor.prepare_sets: every draw is keyed by the CONTENT of the drawing
set, so the components a variant keeps have the parent's anchors and similarities bit for bit) and sent through the model.
The attribution of u is the drop of the explained class's logit,

    delta_logit(u) = mean over draws d of  z_target(S; d) - z_target(S \\ u; d),

both terms at the same draw d of the request's own anchors (``epoch_offset=d``); ``delta_std`` is the sample standard deviation
of that per-draw difference -- the anchor noise, reported instead of hidden.  A unit whose removal leaves nothing has no variant.

    python -m subgnn_amd.explain -config_path CONFIG -restoreModelPath DIR [-restoreModelName F] -subgraphs FILE -out FILE
                                 [-unit node|component] [-target LABEL] [-draws E] [-top N] [-batch_size B]
"""
import argparse

import torch

from . import cli, ops, scoring

UNITS = ('node', 'component')
HEADER = 'request\tunit\tdelta_logit\tdelta_std\tdelta_prob\tlabel_without'


def component_members(sets, labels, n_units):
    """The members of every component of every set, components in unit order (by set, then by smallest position) ->
    (ptr int64 (n_units + 1), ids int64), on the device.  ``labels``: ops.cc_labels of ``sets``."""
    dev = sets.ptr.device
    total = int(sets.ptr[-1].item())
    lengths = sets.lengths
    row = torch.repeat_interleave(torch.arange(sets.n, device=dev), lengths)
    start = sets.ptr[:-1][row]
    pos = torch.arange(total, device=dev) - start
    lab = labels[:total].long()
    unit_of_root = torch.cumsum((lab == pos).long(), 0) - 1            # units are numbered by set, then by root position
    unit = unit_of_root[start + lab]
    order = torch.sort(unit, stable=True).indices
    return ops.exclusive_scan(torch.bincount(unit, minlength=n_units)), sets.nodes[:total].long()[order]


def explain(p, subgraphs, unit='node', target=None, draws=1, batch_size=None, max_variants=65536):
    """``Predictor.explain``.  -> dict:
      ``subgraphs``, ``logits``, ``probabilities``, ``labels`` (and the ``*_mean`` / ``*_std`` keys for ``draws > 1``): the
                    base request, as ``predict(draws=draws)`` gives them;
      ``target``    (R,) int64, the class explained per request: the argmax of the mean base logits (for a multi-label model
                    too), or the given int or sequence of R ints;
      ``ptr``       (R + 1,) int64: the units of request r are ``ptr[r]:ptr[r + 1]``;
      ``unit_nodes`` node mode: (U,) int64, the unit's model id; component mode: (ptr (U + 1,), ids) of the components' members;
      ``valid``     (U,) bool: False where removing the unit leaves nothing (no variant);
      ``variant_logits`` (U, K): the variant's logits, mean over draws; ``delta_logit``, ``delta_std`` (0 for one draw),
      ``delta_prob`` (U,): see the module's docstring; ``delta_prob`` is the same difference of the target's probability
                    (softmax; sigmoid for a multi-label model).  NaN where not valid.
    The variants are prepared and forwarded in chunks of at most ``max_variants`` sets (a bound on memory, not a tuned
    number); ``batch_size`` chunks every forward pass.  The model's own splits stay as ``Predictor.prepare`` leaves them."""
    if unit not in UNITS:
        raise ValueError("unit must be 'node' or 'component', got %r" % (unit,))
    E, max_variants = scoring.positive(draws, 'draws'), scoring.positive(max_variants, 'max_variants')
    if batch_size is not None:
        batch_size = scoring.positive(batch_size, 'batch_size')
    g = p.model.networkx_graph
    sets = p.request_sets(subgraphs)
    R, dev = sets.n, sets.ptr.device
    out, base = p._predict_sets(sets, batch_size, False, E)                           # base: (E, R, K)
    K = base.shape[2]
    tgt = scoring.class_targets(target, base, R, K, dev)

    # the variants: every request without one of its units
    labels = ops.cc_labels(g, sets) if unit == 'component' else None
    occ = ops.occlusion_sets(sets, unit, labels)
    ptr = ops.exclusive_scan(occ.units)
    U = int(ptr[-1].item())
    out.update({'target': tgt, 'ptr': ptr})
    out['unit_nodes'] = sets.nodes[:U].long() if unit == 'node' else component_members(sets, labels, U)

    var = scoring.variant_logits(p, occ.sets, occ.keys, K, E, batch_size, max_variants)           # (E, V, K)

    # per-variant differences, reduced on the device and scattered to the variants' units
    parent = occ.parent.long()
    row = ptr[:-1][parent] + occ.unit.long()
    z_base, p_base = scoring.target_columns(p, base, tgt)
    z_var, p_var = scoring.target_columns(p, var, tgt[parent])
    d_logit, d_std = scoring.mean_std(z_base[:, parent] - z_var)

    def per_unit(values, shape):
        full = torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
        full[row] = values
        return full

    out['valid'] = torch.zeros(U, dtype=torch.bool, device=dev).index_fill_(0, row, True)
    out['variant_logits'] = per_unit(var.mean(dim=0), (U, K))
    out['delta_logit'] = per_unit(d_logit, (U,))
    out['delta_std'] = per_unit(d_std, (U,))
    out['delta_prob'] = per_unit((p_base[:, parent] - p_var).mean(dim=0), (U,))
    return out


# ---------------------------------------------------------------------- files, CLI --------
def unit_order(delta_logit, valid):
    """The units of one request in the order of the output: descending ``delta_logit``, then ascending rank, invalid units last."""
    return sorted(range(len(valid)), key=lambda u: (not valid[u], -float(delta_logit[u]) if valid[u] else 0.0, u))


def format_line(request, unit_ids, delta_logit, delta_std, delta_prob, label_strings):
    """``request\\tunit\\tdelta_logit\\tdelta_std\\tdelta_prob\\tlabel_without``: ``unit`` is a node id or ``n1-n2-...`` (the
    dataset's numbering), the floats have 9 significant digits (``nan`` for a unit without a variant, whose label is empty)."""
    return '%d\t%s\t%s\t%s\t%s\t%s' % (request, '-'.join(str(int(n)) for n in unit_ids), '%.9g' % float(delta_logit),
                                       '%.9g' % float(delta_std), '%.9g' % float(delta_prob), '-'.join(label_strings))


def lines_of(p, res, top=None):
    """The output lines of an ``explain`` result (without the header)."""
    ptr = res['ptr'].cpu().numpy()
    valid = res['valid'].cpu().numpy()
    dl, ds, dp = (res[k].cpu().numpy() for k in ('delta_logit', 'delta_std', 'delta_prob'))
    vl = res['variant_logits'].float().cpu()
    if isinstance(res['unit_nodes'], tuple):
        uptr, ids = (t.cpu().numpy() for t in res['unit_nodes'])
        members = lambda u: ids[uptr[u]:uptr[u + 1]] - 1
    else:
        ids = res['unit_nodes'].cpu().numpy()
        members = lambda u: ids[u:u + 1] - 1
    lines = []
    for r in range(ptr.shape[0] - 1):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        order = unit_order(dl[lo:hi], valid[lo:hi])
        for k in order[:top]:
            u = lo + k
            lines.append(format_line(r, members(u), dl[u], ds[u], dp[u], cli.predicted_names(p, vl[u]) if valid[u] else []))
    return lines


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Leave-one-out attribution of predictions over nodes or components, from a checkpoint')
    cli.add_run_arguments(ap)
    ap.add_argument('-subgraphs', type=str, required=True, help='one subgraph per line: n1-n2-... (further columns ignored)')
    ap.add_argument('-out', type=str, required=True, help='text file: a header, then ' + HEADER.replace('\t', '<TAB>'))
    ap.add_argument('-unit', type=str, default='node', choices=UNITS, help='what is left out: single nodes or whole components')
    ap.add_argument('-target', type=str, default=None,
                    help='label string of subgraphs.pth to explain (default: per request, the class of the largest mean logit)')
    ap.add_argument('-draws', type=int, default=1, help='anchor draws to average over (default 1: the answer of predict)')
    ap.add_argument('-top', type=int, default=None, help='at most this many lines per request')
    ap.add_argument('-batch_size', type=int, default=None, help='chunk the forward pass (default: one batch)')
    args = ap.parse_args(argv)
    cli.require_positive(ap, args, ('draws', 'top', 'batch_size'))
    if args.out == args.subgraphs:
        ap.error('-subgraphs and -out must be different files')
    return args


def main(argv=None):
    args = parse_args(argv)
    from .predict import read_requests
    requests = read_requests(args.subgraphs)
    p = cli.open_predictor(args)
    res = p.explain(requests, unit=args.unit, target=cli.label_index(p, args.target), draws=args.draws, batch_size=args.batch_size)
    cli.write_lines(args.out, lines_of(p, res, args.top), HEADER)
    return res


if __name__ == '__main__':
    main()

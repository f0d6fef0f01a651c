"""The property labels of SubGNN's synthetic benchmarks -- DENSITY, CUT RATIO, CORENESS, COMPONENT -- for a user's own graph
and subgraph lists, computed on the GPU.

``prepare_dataset.py`` states the four properties as networkx code (``density``, ``cut_ratio``, ``coreness``,
``n_components``; reference prepare_dataset/prepare_dataset.py:519-550), one induced graph per subgraph: fine for a recipe of
250 subgraphs, out of reach for 50 000 subgraphs of a 1M-node graph.  Here one launch (``ops.subgraph_properties``,
csrc/subgraph_props.hip) gives six integers per subgraph, and the property values are formed from them on the host by the
same expressions networkx and ``prepare_dataset`` use -- so they are bit-equal to those, and the letters the reference's
binning gives are the same letters.

An entry of a subgraph that is no node of the graph (0 = PAD, an id beyond the graph's, an id without edges) is dropped, as
``G.subgraph`` drops it; a repeated id counts once.

    python -m subgnn_amd.subgraph_properties DATASET_DIR --property density [--bins 3] [--out FILE]

re-labels the ``subgraphs.pth`` of a dataset directory by a property of its ``edge_list.txt``.
"""
import argparse
import os
from collections import Counter

import numpy as np

PROPERTIES = ('density', 'cut_ratio', 'coreness', 'cc')
# columns of ops.subgraph_properties' counts
N_MEMBERS, N_EDGES, N_SELF_LOOPS, N_BOUNDARY, N_COMPONENTS, CORE_SUM = range(6)


def _as_ragged(g, subgraphs):
    from . import ops
    if isinstance(subgraphs, ops.Ragged):
        return subgraphs
    return ops.Ragged.from_lists([list(s) for s in subgraphs], g.device)


def counts(g, subgraphs):
    """-> int64 numpy (n, 6): the integer counts of ``ops.subgraph_properties`` for a Ragged or a list of lists of device
    (1-based) ids.  The one place this module touches the device."""
    from . import ops
    c, _ = ops.subgraph_properties(g, _as_ragged(g, subgraphs), want_core=False)
    return c.cpu().numpy()


def values_from_counts(c, prop, n_graph_nodes, ignore_self_loops=False):
    """The property values from the integer counts (n, 6), by the oracle's own expressions:
    density   nx.density: m / (n (n - 1)) * 2 with m counting self loops, 0.0 for n <= 1 or m == 0;
    cut_ratio prepare_dataset.cut_ratio: boundary / (n (N - n)), nan where that divides by zero;
    coreness  np.average of nx.core_number: core_sum / n, nan for n == 0 (ValueError for a subgraph with a self loop, which
              nx.core_number refuses, unless ``ignore_self_loops``);
    cc        nx.number_connected_components (int64)."""
    if prop not in PROPERTIES:
        raise ValueError('prop must be one of %r, got %r' % (PROPERTIES, prop))
    c = np.asarray(c, dtype=np.int64).reshape(-1, 6)
    n = c[:, N_MEMBERS]
    if prop == 'cc':
        return c[:, N_COMPONENTS].copy()
    with np.errstate(divide='ignore', invalid='ignore'):
        if prop == 'density':
            m = c[:, N_EDGES] + c[:, N_SELF_LOOPS]
            d = m.astype(np.float64) / (n * (n - 1)).astype(np.float64) * 2
            return np.where((n <= 1) | (m == 0), 0.0, d)
        if prop == 'cut_ratio':
            den = n * (int(n_graph_nodes) - n)
            return np.where(den == 0, np.nan, c[:, N_BOUNDARY].astype(np.float64) / den.astype(np.float64))
        loops = np.nonzero(c[:, N_SELF_LOOPS] > 0)[0]
        if len(loops) and not ignore_self_loops:
            raise ValueError('subgraph %d has a self loop: networkx.core_number is not defined for it '
                             '(ignore_self_loops=True leaves self loops out)' % int(loops[0]))
        return np.where(n == 0, np.nan, c[:, CORE_SUM].astype(np.float64) / n.astype(np.float64))


def values(g, subgraphs, prop, ignore_self_loops=False):
    """float64 numpy values of ``prop`` (int64 for 'cc'), one per subgraph; see ``values_from_counts``."""
    if prop not in PROPERTIES:
        raise ValueError('prop must be one of %r, got %r' % (PROPERTIES, prop))
    return values_from_counts(counts(g, subgraphs), prop, g.n_nodes, ignore_self_loops)


def letters_of(vals, prop, n_bins=3):
    """``prepare_dataset.labels_of``'s binning rules on values that are already computed: 'cc' splits at [1, 5], density and
    cut ratio take as many equal-count bins as their recipe ranges have entries (three), any other property ``n_bins``."""
    from . import prepare_dataset as pd
    vals = [v.item() if hasattr(v, 'item') else v for v in vals]
    if prop == 'cc':
        ids = np.digitize(vals, bins=[1, 5])
    elif prop == 'density':
        ids = np.digitize(vals, bins=pd.equal_count_bins(vals, len(pd.DENSITY_RANGE)))
    elif prop == 'cut_ratio':
        ids = np.digitize(vals, bins=pd.equal_count_bins(vals, len(pd.CUT_RATIO_RANGE)))
    else:
        ids = np.digitize(vals, bins=pd.equal_count_bins(vals, n_bins))
    return pd.letters(ids)


def labels(g, subgraphs, prop, n_bins=3, ignore_self_loops=False):
    """-> (letters, values): the label letter ``prepare_dataset.labels_of`` gives every subgraph, and the values behind them."""
    vals = values(g, subgraphs, prop, ignore_self_loops)
    if len(vals) == 0:
        return [], vals
    return letters_of(vals, prop, n_bins), vals


def label_dataset(dataset_dir, prop, n_bins=3, out=None, device=None, ignore_self_loops=False):
    """Label the subgraphs of ``dataset_dir``/subgraphs.pth by ``prop`` of the graph in ``dataset_dir``/edge_list.txt.
    Writes a subgraphs file with the same subgraph and split columns and the label column replaced, to ``out`` (default
    ``subgraphs_<prop>.pth`` beside the input; never the input itself) -> (path, summary): the label histogram, the smallest
    and largest value, and how many subgraphs held ids that are no nodes of the graph."""
    from .graph import load_graph
    if prop not in PROPERTIES:
        raise ValueError('prop must be one of %r, got %r' % (PROPERTIES, prop))
    src = os.path.join(str(dataset_dir), 'subgraphs.pth')
    dst = os.path.join(str(dataset_dir), 'subgraphs_%s.pth' % prop) if out is None else str(out)
    if os.path.realpath(dst) == os.path.realpath(src):
        raise ValueError('label_dataset does not overwrite its input (%s)' % src)
    if device is None:
        device = 'cuda'
    g = load_graph(os.path.join(str(dataset_dir), 'edge_list.txt'), device)
    rows, subs = [], []
    with open(src) as f:
        for line in f:
            cols = line.split('\t')
            ids = [int(v) for v in cols[0].split('-') if v.strip() != ''] if len(cols) >= 3 else []
            if not ids:
                continue                                        # (read_subgraphs skips such lines too)
            rows.append(cols)
            subs.append([v + 1 for v in ids])                   # file ids are 0-based, device ids 1-based (0 = PAD)
    c = counts(g, subs) if subs else np.zeros((0, 6), dtype=np.int64)
    vals = values_from_counts(c, prop, g.n_nodes, ignore_self_loops)
    labs = letters_of(vals, prop, n_bins) if len(vals) else []
    with open(dst, 'w') as f:
        for cols, lab in zip(rows, labs):
            line = '\t'.join([cols[0], str(lab)] + cols[2:])
            f.write(line if line.endswith('\n') else line + '\n')
    dropped = int(sum(int(c[i, N_MEMBERS]) < len(set(s)) for i, s in enumerate(subs)))
    finite = np.asarray(vals, dtype=np.float64)
    finite = finite[np.isfinite(finite)]
    summary = dict(property=prop, n_subgraphs=len(subs), histogram=dict(sorted(Counter(labs).items())),
                   value_min=float(finite.min()) if len(finite) else None,
                   value_max=float(finite.max()) if len(finite) else None, sets_with_dropped_ids=dropped)
    return dst, summary


def main(argv=None):
    ap = argparse.ArgumentParser(description='Label the subgraphs of a dataset directory by a structural property (GPU)')
    ap.add_argument('dataset_dir')
    ap.add_argument('--property', required=True, choices=PROPERTIES)
    ap.add_argument('--bins', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--ignore-self-loops', action='store_true', help='coreness: leave self loops out instead of refusing them')
    a = ap.parse_args(argv)
    path, summary = label_dataset(a.dataset_dir, a.property, n_bins=a.bins, out=a.out, ignore_self_loops=a.ignore_self_loops)
    print(path)
    print(summary)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())

"""-m gpu: the kernels that share the id table and the union-find of csrc/id_table.h (degree sequences, component labels and
compaction, in-border flags, subgraph properties) on ONE ragged list that puts sets on both sides of the two tier edges and
two workspace-tier sets next to each other, against the CPU oracles.  Exact.

Entry counts, in this order: 2049, 2049, 64, 65, 2048, 2050, 0, 2049.  The first two are neighbours in the workspace: the
first's length is odd, so the second's region starts at byte 16 x 2049, inside a 128-byte line, and with 2049 entries (8192 of
8196 slots used) the last used line of a region reaches into the next one.  64 | 65 and 2048 | 2049 are the tier edges; the
last set ends the array.  One set of each tier repeats an id."""
import networkx as nx
import numpy as np
import pytest
import torch

import subgraph_props_cases as SC
from oracle import integer_half as IH, cbind
from test_gpu_integer import DEV, _dev_graph, _labels_to_sets, _ops, _rand_graph

pytestmark = pytest.mark.gpu
LENGTHS = (2049, 2049, 64, 65, 2048, 2050, 0, 2049)
_SETUP = []


def shared():
    """(oracle graph, device graph, the sets, their Ragged): built once, never written."""
    if not _SETUP:
        G = _rand_graph(3000, 3, 41)                            # ids 1..3000; self loops at 1, 4, 11; hubs 1 and 8
        rng = np.random.default_rng(12)
        rest = np.arange(1, G.max_id() + 1)
        rest = rest[~np.isin(rest, (1, 4, 8))]
        # every set that is not empty holds the hub with a self loop (1), a plain self loop (4) and the other hub (8)
        sets = [[1, 4, 8] + rng.choice(rest, n - 3, replace=False).tolist() if n else [] for n in LENGTHS]
        sets[1][10] = sets[1][2000]                             # a repeated id: workspace tier,
        sets[2][63] = sets[2][5]                                # wave tier,
        sets[4][2047] = sets[4][64]                             # LDS tier
        assert [len(s) for s in sets] == list(LENGTHS)
        _SETUP.append((G, _dev_graph(G), sets, _ops().Ragged.from_lists(sets, DEV)))
    return _SETUP[0]


def test_the_sets_sit_where_the_docstring_says():
    ops = _ops()
    _, _, sets, r = shared()
    assert [SC.tier(len(s)) for s in sets] == ['workspace', 'workspace', 'wave', 'lds', 'lds', 'workspace', 'wave', 'workspace']
    assert ops.CC_LDS_MAX == SC.LDS_MAX and r.max_len == 2050
    ptr = r.ptr.tolist()
    assert (16 * ptr[1]) % 128 != 0 and ptr[-1] == r.nodes.numel()
    for s in (1, 2, 4):
        assert len(set(sets[s])) == len(sets[s]) - 1


@pytest.mark.parametrize('srt', [True, False])
def test_degree_sequences(srt):
    ops = _ops()
    G, dg, sets, r = shared()
    rowptr, col = G.csr()
    ptr, flat = cbind.ragged(sets)
    ci, ce = cbind.degree_sequence(rowptr, col, None, ptr, flat, srt)
    gi, ge = ops.degree_sequence(dg, r, sort=srt, use_degree_dict=False)
    assert np.array_equal(gi.cpu().numpy()[:len(ci)], ci)
    assert np.array_equal(ge.cpu().numpy()[:len(ce)], ce)


def test_component_labels_and_the_component_tensor():
    ops = _ops()
    from subgnn_amd.subgraph_utils import components_from_labels
    G, dg, sets, r = shared()
    labels = ops.cc_labels(dg, r)
    lab = ops.Ragged(r.ptr, labels).to_lists()
    refs = [IH.connected_components(G, s) if s else [] for s in sets]
    for s, nodes in enumerate(sets):
        assert _labels_to_sets(nodes, lab[s]) == {frozenset(c) for c in refs[s]}, s
        for i, l in enumerate(lab[s]):
            assert l <= i and lab[s][l] == l, (s, i)           # the label is the smallest position in the component
    out = components_from_labels(r.ptr, r.nodes, labels, r.max_len).cpu().numpy()
    assert out.shape == (len(sets), max(len(c) for c in refs), max(len(cc) for c in refs for cc in c))
    for s in range(len(sets)):
        got = [[int(v) for v in row if v != 0] for row in out[s] if row[0] != 0]
        assert got == refs[s], s


def test_patch_in_border():
    ops = _ops()
    G, dg, sets, r = shared()
    flags = ops.Ragged(r.ptr, ops.patch_in_border(dg, r).to(torch.int32)).to_lists()
    for s, (v, f) in enumerate(zip(sets, flags)):
        want = set(IH.patch_in_border_nodes(G, v))
        assert set(f) <= {0, 1}, s
        assert [x for x, b in zip(v, f) if b] == [x for x in v if x in want], s


def test_subgraph_properties():
    ops = _ops()
    G, dg, sets, r = shared()
    Gx = nx.Graph()
    Gx.add_edges_from((u, v) for u in G.node_order for v in G.neighbors(u))
    counts, core = ops.subgraph_properties(dg, r)
    counts, core = counts.cpu().tolist(), ops.Ragged(r.ptr, core).to_lists()
    for s, nodes in enumerate(sets):
        want_counts, want_core = SC.oracle_counts(Gx, nodes)
        assert counts[s] == want_counts, s
        assert core[s] == want_core, s

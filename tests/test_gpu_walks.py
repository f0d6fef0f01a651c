"""-m gpu: the two workgroup-per-walk kernels -- the list kernel and the launch rule (``ops.triangular_walks(kernel=0)``,
``ops.triangular_walks_both``) and the bitmap kernel on its own (``kernel=2``) -- against the wavefront kernel (``kernel=1``) and
the oracle, element for element, on the cases of tests/walks_cases.py -- tests/test_walks_cases_host.py shows that they reach
the branches they are named for."""
import functools

import numpy as np
import pytest
import torch

from oracle import tape as T

import walks_cases as WC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SID = T.stream_id(T.STREAM_STRUCT_PATCH)
SID_INT, SID_BOR = T.stream_id(T.STREAM_WALK_INT), T.stream_id(T.STREAM_WALK_BOR)


def _ops():
    from subgnn_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _dev(G):
    rp, col = G.csr()
    return _ops().DeviceGraph(rp, col, np.asarray(G.node_order, dtype=np.int32), DEV)


@functools.lru_cache(maxsize=None)
def _ref(G, n, walk_len, item_base=0):
    return WC.graph_walks(G, n, walk_len, item_base=item_base)


def _graph_walks(G, n, walk_len, **kw):
    return _ops().triangular_walks(_dev(G), 0, n, walk_len, WC.BETA, WC.SEED, SID, **kw).cpu().numpy()


def _check_graph_walks(G, n, walk_len, tables=(True, False), variants=(0, WC.LIST_KERNEL)):
    """variant 0 is the launch rule (the bitmap kernel for launches of up to WC.FEW_WALKS walks on these small graphs),
    WC.LIST_KERNEL the list kernel whatever the size of the launch; kernel 2 the bitmap kernel whatever the size."""
    ref = _ref(G, n, walk_len)
    for kernel in (1, 2):
        assert np.array_equal(_graph_walks(G, n, walk_len, kernel=kernel), ref), kernel
    for hub_tables in tables:
        for variant in variants:
            got = _graph_walks(G, n, walk_len, hub_tables=hub_tables, variant=variant)
            assert np.array_equal(got, ref), (hub_tables, variant)


@pytest.mark.parametrize('deg', [511, 512, 513])
def test_lists_on_both_sides_of_the_hub_boundary(deg):
    """N(prev) of 1 (the pendants), 511, 512 and 513 entries: the LDS list against the hub bit, and against the global search
    where the tables are withheld."""
    G = WC.hub_graph(deg)
    assert (_dev(G).hub_tables() is not None) == (deg >= WC.LIST_MAX)
    _check_graph_walks(G, 200, 8)


@pytest.mark.parametrize('variant', [1, 2, 3, 4])
def test_two_linked_hubs_at_every_launch_shape(variant):
    G = WC.two_hubs_graph()
    assert _dev(G).hub_tables() is not None
    _check_graph_walks(G, 200, 8, variants=(variant,))


def test_self_loops_and_repeated_entries():
    G = WC.hub_graph(513, self_loops=True)
    assert _dev(G).hub_tables() is not None
    _check_graph_walks(G, 200, 8)
    G = WC.two_hubs_graph(duplicates=True)
    assert _dev(G).hub_tables() is None                    # repeated ids in a row: long lists are searched
    _check_graph_walks(G, 200, 8, tables=(True,))


def test_a_list_longer_than_the_ballot_cache():
    G = WC.star_graph()
    _check_graph_walks(G, 16, 4, variants=(0, WC.LIST_KERNEL, 4))       # caches of 256 and of 1024 chunks


def test_dead_ends_and_isolated_starts():
    _check_graph_walks(WC.dead_end_graph(), 20, 5, tables=(True,))
    _check_graph_walks(WC.random_graph(), 400, 3, tables=(True,))        # some start on a node without edges


@pytest.mark.parametrize('walk_len', [1, 2, 3, 50])
def test_walk_lengths(walk_len):
    _check_graph_walks(WC.random_graph(), 64, walk_len, tables=(True,))


@pytest.mark.parametrize('walks_per_patch', [1, 5])
def test_patch_modes_and_the_combined_launch(walks_per_patch):
    """Patches of 1, 96 and 97 nodes, an empty one, one without in-border nodes: modes 1 and 2 on their own and in one launch."""
    ops = _ops()
    G, views, inb = WC.patches()
    dg = _dev(G)
    vr, ir = ops.Ragged.from_lists(views, DEV), ops.Ragged.from_lists(inb, DEV)
    n, L = len(views) * walks_per_patch, 6
    K = WC.LIST_KERNEL
    both = ops.triangular_walks_both(dg, n, L, WC.BETA, WC.SEED, SID_INT, SID_BOR, vr, ir, walks_per_patch, variant=K)
    for kw in ({'variant': K, 'hub_tables': False}, {'variant': 0}, {'kernel': 2}):
        assert torch.equal(both, ops.triangular_walks_both(dg, n, L, WC.BETA, WC.SEED, SID_INT, SID_BOR, vr, ir, walks_per_patch, **kw))
    for k, (inside, sid) in enumerate(((True, SID_INT), (False, SID_BOR))):
        ref = WC.patch_walks(G, views, inb, walks_per_patch, L, inside)
        for kernel, variant in ((0, K), (0, 0), (1, 0), (2, 0)):
            got = ops.triangular_walks(dg, 1 if inside else 2, n, L, WC.BETA, WC.SEED, sid, patches=vr, in_border=ir,
                                       walks_per_patch=walks_per_patch, kernel=kernel, variant=variant)
            assert np.array_equal(got.cpu().numpy(), ref), (inside, kernel, variant)
        assert np.array_equal(both[k].cpu().numpy(), ref), inside
    lo, hi = 1, 4                                                     # patches 1 .. 3 as a share of the launch
    part = ops.triangular_walks_both(dg, (hi - lo) * walks_per_patch, L, WC.BETA, WC.SEED, SID_INT, SID_BOR,
                                     ops.Ragged.from_lists(views[lo:hi], DEV), ops.Ragged.from_lists(inb[lo:hi], DEV), walks_per_patch,
                                     item_base=lo * walks_per_patch, variant=K)
    assert torch.equal(part, both[:, lo * walks_per_patch:hi * walks_per_patch])


def test_item_base_gives_the_slice_of_the_whole_launch():
    G = WC.random_graph()
    whole = _graph_walks(G, 150, 7, variant=WC.LIST_KERNEL)
    assert np.array_equal(whole, _ref(G, 150, 7))
    for lo, hi in ((1, 2), (37, 150)):
        assert np.array_equal(_graph_walks(G, hi - lo, 7, item_base=lo, variant=WC.LIST_KERNEL), whole[lo:hi])


def test_more_walks_than_the_chip_holds_at_once():
    G = WC.random_graph()
    got = _graph_walks(G, 5000, 3)
    assert np.array_equal(got, _graph_walks(G, 5000, 3, kernel=1))
    assert np.array_equal(got[:500], _ref(G, 500, 3))


def test_the_bitmap_kernel_takes_several_items_per_workgroup_and_cleans_up_between_them():
    """WC.BITMAP_GRID workgroups, 64 walks more: the first 64 workgroups take a second item, on the bitmap their first walk
    used.  A bit left behind would turn a non-triangle candidate of the second walk into a triangle one
    (test_walks_cases_host: some of those walks meet both classes at a step, after a first walk of full length)."""
    G = WC.random_graph()
    n = WC.BITMAP_GRID + 64
    assert np.array_equal(_graph_walks(G, n, 6, kernel=2), _ref(G, n, 6))


def test_the_kernel_argument_is_checked_on_the_host():
    """Returns of the entry points, made before any launch."""
    ops = _ops()
    from subgnn_amd._lib import SubgnnHipError
    rowptr, col, order = WC.sparse_ids_csr()
    big = ops.DeviceGraph(rowptr, col, order, DEV)
    one = ops.Ragged.from_lists([[int(order[0])]], DEV)
    with pytest.raises(SubgnnHipError):                               # ids beyond the bitmap
        ops.triangular_walks(big, 0, 10, 4, WC.BETA, WC.SEED, SID, kernel=2)
    with pytest.raises(SubgnnHipError):
        ops.triangular_walks_both(big, 1, 4, WC.BETA, WC.SEED, SID_INT, SID_BOR, one, one, 1, kernel=2)
    G, views, inb = WC.patches()
    dg = _dev(G)
    vr, ir = ops.Ragged.from_lists(views, DEV), ops.Ragged.from_lists(inb, DEV)
    for kernel in (1, 3):                                             # the wavefront kernel has no combined launch
        with pytest.raises(SubgnnHipError):
            ops.triangular_walks_both(dg, len(views), 4, WC.BETA, WC.SEED, SID_INT, SID_BOR, vr, ir, 1, kernel=kernel)
    with pytest.raises(SubgnnHipError):
        ops.triangular_walks(dg, 0, 10, 4, WC.BETA, WC.SEED, SID, kernel=3)


def test_ids_beyond_any_lds_bitmap():
    ops = _ops()
    rowptr, col, order = WC.sparse_ids_csr()
    dg = ops.DeviceGraph(rowptr, col, order, DEV)
    out = [ops.triangular_walks(dg, 0, 300, 10, WC.BETA, WC.SEED, SID, kernel=k) for k in (0, 1)]
    assert torch.equal(out[0], out[1])
    assert int(out[0].max()) > 1_200_000 and int((out[0] != 0).sum()) > 300 * 5


def test_hub_tables_built_on_one_stream_are_complete_for_a_reader_on_another():
    """A pass's first walks build the graph's hub tables on the side stream while the degree sequences read them on the main
    one, with no event between the two: the tables (and the node records made from them) are whole when they are handed out --
    here they are built behind queued work on a side stream and copied at once on the default stream."""
    ops = _ops()
    G = WC.two_hubs_graph()
    rp, col = G.csr()
    fresh = [ops.DeviceGraph(rp, col, np.asarray(G.node_order, dtype=np.int32), DEV) for _ in range(2)]     # nothing cached
    want = fresh[1].hub_tables()
    want_rec = fresh[1].node_records()
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        side.wait_stream(torch.cuda.current_stream())
        for _ in range(20):
            a = (a @ a) * 1e-3                            # queued ahead of the build
        hub = fresh[0].hub_tables()
    idx, bits = hub[0].clone(), hub[1].clone()            # default stream, at once
    with torch.cuda.stream(side):
        rec = fresh[0].node_records()
    rec_copy = rec.clone()
    torch.cuda.synchronize()
    assert hub[2] == want[2] and torch.equal(idx, want[0]) and torch.equal(bits, want[1]) and int((bits != 0).sum()) > 0
    assert torch.equal(rec_copy, want_rec)


def test_a_launch_the_rule_sends_to_the_bitmap_kernel_builds_no_hub_tables():
    ops = _ops()
    G = WC.two_hubs_graph()
    rp, col = G.csr()
    dg = ops.DeviceGraph(rp, col, np.asarray(G.node_order, dtype=np.int32), DEV)
    got = ops.triangular_walks(dg, 0, WC.FEW_WALKS, 8, WC.BETA, WC.SEED, SID).cpu().numpy()
    assert '_hub_tables' not in dg.__dict__ and np.array_equal(got[:200], _ref(G, 200, 8))
    ops.triangular_walks(dg, 0, WC.FEW_WALKS + 1, 8, WC.BETA, WC.SEED, SID)
    assert dg.__dict__['_hub_tables'] is not None


def test_two_launches_in_a_row_give_the_same_walks():
    G = WC.two_hubs_graph()
    a = _graph_walks(G, 600, 8)
    b = _graph_walks(G, 600, 8)
    assert np.array_equal(a, b) and np.array_equal(a[:200], _ref(G, 200, 8))

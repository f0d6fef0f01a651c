"""Without a GPU: the oracle's walks over the graphs of tests/walks_cases.py really take the steps the cases of
tests/test_gpu_walks.py are named for -- the lengths of N(prev) on both sides of the hub boundary, prev and curr both hubs, both
candidate classes at one step, a list longer than every ballot cache, dead ends, walks that end at their first node, patches on
both sides of the hash limit -- so that the comparison on the GPU cannot pass without touching those branches.  The constants
walks_cases restates are the ones in samplers.hip and degree_sequence.hip."""
import os
import re

import pytest

import walks_cases as WC

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _all_steps(G, n, walk_len):
    walks = WC.graph_walks(G, n, walk_len)
    return walks, [s for w in walks for s in WC.steps(G, w)]


def test_constants_are_the_sources():
    src = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'samplers.hip')).read()
    defines = {k: int(v) for k, v in re.findall(r'^#define (W\w+) (\d+)\b', src, re.M)}
    assert defines['WKS_LIST_MAX'] == WC.LIST_MAX and defines['WK_CHUNKS'] == WC.WK_CHUNKS and defines['WK_HASH_MAX'] == WC.HASH_MAX
    assert defines['WKS_VARIANTS'] == len(WC.CHUNKS) == len(WC.THREADS) and defines['WKS_FEW_WALKS'] == WC.FEW_WALKS
    shapes = {int(v): (int(t), int(c)) for v, t, c in re.findall(r'case (\d): WKS_GO\((\d+), (\d+)\)', src)}
    shapes[0] = shapes[WC.LIST_KERNEL] = tuple(int(x) for x in re.search(r'default: WKS_GO\((\d+), (\d+)\)', src).groups())
    assert [shapes[v] for v in range(len(WC.CHUNKS))] == list(zip(WC.THREADS, WC.CHUNKS))
    assert re.search(r'dim3\(\(int\)\(g\.n_items < (\d+) \? g\.n_items : \1\)\), dim3\(WKB_THREADS\)', src).group(1) == str(WC.BITMAP_GRID)
    ds = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'degree_sequence.hip')).read()
    assert int(re.search(r'^#define DS_SEARCH (\d+)\b', ds, re.M).group(1)) == WC.LIST_MAX     # the hub tables' threshold


@pytest.mark.parametrize('deg', [511, 512, 513])
def test_hub_graph_walks_test_against_lists_of_1_and_of_deg_entries(deg):
    G = WC.hub_graph(deg)
    assert len(G.neighbors(1)) == deg
    _, st = _all_steps(G, 200, 8)
    lens = {s['prev_len'] for s in st}
    assert 1 in lens and deg in lens
    assert any(s['prev_len'] == deg and s['nt'] > 0 and s['nn'] > 0 for s in st)        # both classes against the long list
    assert any(s['prev_len'] < WC.LIST_MAX and s['curr_len'] == deg and s['nt'] > 0 and s['nn'] > 0 for s in st)


def test_two_hubs_graph_has_steps_from_hub_to_hub():
    for dup in (False, True):
        G = WC.two_hubs_graph(duplicates=dup)
        _, st = _all_steps(G, 200, 8)
        hub_hub = [s for s in st if s['prev_len'] >= WC.LIST_MAX and s['curr_len'] >= WC.LIST_MAX]
        assert hub_hub and any(s['nt'] > 0 and s['nn'] > 0 for s in hub_hub)
        rows = [G.neighbors(v) for v in G.node_order]
        assert any(len(r) != len(set(r)) for r in rows) == dup
        if dup:                                               # a repeated id in a long row and in a short one
            assert any(len(r) != len(set(r)) and len(r) >= WC.LIST_MAX for r in rows)
            assert any(len(r) != len(set(r)) and len(r) < WC.LIST_MAX for r in rows)


def test_self_loop_graph_tests_candidates_that_are_prev_itself():
    G = WC.hub_graph(513, self_loops=True)
    assert len(G.neighbors(1)) == 513 and 1 in G.neighbors(1) and 2 in G.neighbors(2)
    walks, st = _all_steps(G, 200, 8)
    assert any(s['prev'] == 1 and s['curr'] == 1 for s in st)              # the hub's loop taken: prev == curr, a hub
    assert any(s['prev_len'] == 513 and s['curr'] != 1 for s in st)        # candidate 1 tested against N(1), which holds 1
    assert any(s['prev'] == 2 or s['curr'] == 2 for s in st)


def test_star_walks_step_onto_a_list_longer_than_every_cache():
    G = WC.star_graph()
    assert len(G.neighbors(1)) == 64 * max(WC.CHUNKS) + 1
    _, st = _all_steps(G, 16, 4)
    onto = [s for s in st if s['curr'] == 1]
    assert onto and any(s['nt'] > 0 and s['nn'] > 0 for s in onto)         # picked out of the long list, both classes present
    assert any(s['prev'] == 1 for s in st)                                  # and tested against it at the step after


def test_dead_ends_and_walks_that_end_at_their_first_node():
    G = WC.dead_end_graph()
    walks = WC.graph_walks(G, 20, 5)
    assert any(WC.stopped_dead(G, w, 5) for w in walks)                     # nt + nn == 0 at a later step
    assert any(WC.stopped_at_start(G, w) for w in walks)                    # node 3: nn == 0 at the first step
    G = WC.random_graph()
    assert any(WC.stopped_at_start(G, w) for w in WC.graph_walks(G, 400, 3))


def test_second_items_of_a_bitmap_workgroup_meet_both_classes_after_a_full_first_walk():
    """Walk i >= BITMAP_GRID runs on the bitmap walk i - BITMAP_GRID used: a bit that one left set could only show at a step
    of the later walk that has both candidate classes -- and a walk of full length is one that held bits to its end."""
    G = WC.random_graph()
    n, L = WC.BITMAP_GRID + 64, 6
    walks = WC.graph_walks(G, n, L)
    assert any((walks[i - WC.BITMAP_GRID] != 0).all() and any(s['nt'] > 0 and s['nn'] > 0 for s in WC.steps(G, walks[i]))
               for i in range(WC.BITMAP_GRID, n))


def test_patches_lie_on_both_sides_of_the_hash_limit():
    G, views, inb = WC.patches()
    sizes = [len(v) for v in views]
    assert sizes[:4] == [1, WC.HASH_MAX, WC.HASH_MAX + 1, 0] and max(sizes) > WC.HASH_MAX + 1
    assert inb[4] == [] and views[4] and all(len(b) > 0 for b, v in zip(inb, views) if v and v is not views[4])
    assert any(len(b) > WC.HASH_MAX for b in inb) and any(0 < len(b) <= WC.HASH_MAX for b in inb)
    for inside in (True, False):
        ref = WC.patch_walks(G, views, inb, 5, 6, inside)
        assert (ref[3 * 5:4 * 5] == 0).all()                                # the empty patch: PAD rows
        assert (ref[4 * 5:5 * 5, 0] != 0).all() == inside                   # no in-border node: the border walks are PAD rows
        member = [set(v) for v in views]
        some_both = False
        for p, v in enumerate(views):
            ok = (lambda x, m=member[p]: x in m) if inside else (lambda x, m=member[p], b=set(inb[p]): x not in m or x in b)
            for w in ref[p * 5:(p + 1) * 5]:
                some_both |= any(s['nt'] > 0 and s['nn'] > 0 for s in WC.steps(G, w, ok))
        assert some_both

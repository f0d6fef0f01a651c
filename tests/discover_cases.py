"""The definition of the seeded walk sets (include/subgnn_hip.h: sgnn_seeded_walk_sets) in numpy and Python ints, the graph and
the cases the tests send through the kernel, and the kernel's launch limits restated.  No GPU, no library.

Item q is candidate q % per_seed of seed q // per_seed; its walk starts at the seed, steps to a uniformly drawn neighbour of the
current node or -- with probability restart_thr / 2^32 -- back to the seed, and collects the nodes it visits until it holds its
target size or has taken max_steps steps.  Draw 2t of the item decides the restart of step t, draw 2t + 1 the neighbour."""
import functools

import numpy as np

from subgnn_amd import tape

MAX_SIZE = 256                           # csrc/seeded_sets.hip SGNN_SEEDED_MAX_SIZE
GRID_CAP = 8192                          # csrc/seeded_sets.hip SGNN_SEEDED_GRID_CAP: the workgroups (one item each) of a launch
SIZES = (1, 2, 3, 63, 64, 65, 128, 255, 256)
SEED = 20261019
STREAM = tape.stream_id(tape.STREAM_DISCOVER, 'predict')
THR_DEFAULT = int(0.15 * 4294967296.0)   # restart = 0.15
THRS = (0, 1 << 31, 1 << 32)

# ---- the graph: ids 1 .. MAX_ID, row 0 (PAD) empty --------------------------------------------------------------------------
PATH = list(range(1, 11))                # a path 1 - 2 - ... - 10
HUB = 11                                 # a star: adjacent to every node of the sparse part
K5 = list(range(12, 17))                 # every node of degree 4
LOOP = 17                                # its only edge is a self loop
TRIPLE = [18, 19, 20]                    # a component of three nodes: 18 - 19 - 20
BARE = 21                                # an id without an edge (22 .. 29 have none either)
SPARSE = list(range(30, 340))            # 310 nodes, two random edges each (degree about 4) and the hub
MAX_ID = 340                             # (340 has no edge)
# seeds of the cases: both kinds of path node, the hub, a K5 node, the self loop, the triple, no edge, the sparse part, and three
# ids that are no nodes (the entry takes them; ops.seeded_walk_sets refuses them)
SEEDS = (1, 5, HUB, 12, LOOP, 18, BARE, 30, 100, 339, 0, MAX_ID + 1, -5)
MANY_PER_SEED = 30
assert len(SPARSE) * MANY_PER_SEED > GRID_CAP


@functools.lru_cache(maxsize=None)
def graph():
    """-> (rowptr int64[MAX_ID + 2], col_sorted int32): the CSR with ascending rows, every edge in both rows (a self loop once)."""
    edges = set()
    add = lambda a, b: edges.update({(a, b), (b, a)})
    for a, b in zip(PATH[:-1], PATH[1:]):
        add(a, b)
    for v in SPARSE:
        add(HUB, v)
    for i, a in enumerate(K5):
        for b in K5[i + 1:]:
            add(a, b)
    add(LOOP, LOOP)
    add(TRIPLE[0], TRIPLE[1])
    add(TRIPLE[1], TRIPLE[2])
    rng = np.random.default_rng(5)
    for v in SPARSE:
        for w in rng.choice(SPARSE, size=2, replace=False).tolist():
            if w != v:
                add(v, w)
    e = np.array(sorted(edges), dtype=np.int64)
    rowptr = np.zeros(MAX_ID + 2, dtype=np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=MAX_ID + 1), out=rowptr[1:])
    return rowptr, e[:, 1].astype(np.int32)


def degree(v):
    rowptr, _ = graph()
    return int(rowptr[v + 1] - rowptr[v])


# ---- the definition ---------------------------------------------------------------------------------------------------------
def sample(rowptr, col_sorted, seeds, sizes, per_seed, width, restart_thr, max_steps, seed, stream, item_base=0, n_items=None,
           item_ids=None):
    """-> dict: ``nodes`` int32 (n_items, width), ``len``, ``steps`` int32, ``keys`` uint64."""
    max_id, n_seeds = len(rowptr) - 2, len(seeds)
    if item_ids is None:
        if n_items is None:
            n_items = n_seeds * per_seed - item_base
        assert item_base >= 0 and item_base + n_items <= n_seeds * per_seed
        items = [item_base + i for i in range(n_items)]
    else:
        items = [int(q) for q in item_ids]
    out = {'nodes': np.zeros((len(items), width), dtype=np.int32), 'len': np.zeros(len(items), dtype=np.int32),
           'steps': np.zeros(len(items), dtype=np.int32), 'keys': np.zeros(len(items), dtype=np.uint64)}
    for i, q in enumerate(items):
        members, t = [], 0
        s = int(seeds[q // per_seed]) if 0 <= q < n_seeds * per_seed else 0
        if 1 <= s <= max_id:
            members.append(s)
            size = min(max(int(sizes[q % per_seed]), 1), width)
            if rowptr[s + 1] > rowptr[s] and max_steps > 0 and size > 1:
                draws = (tape.draw64_np(seed, stream, q, np.arange(2 * max_steps, dtype=np.uint64)) >> np.uint64(32)).tolist()
                cur = s
                while len(members) < size and t < max_steps:
                    if draws[2 * t] < restart_thr:
                        cur = s
                    else:
                        beg = int(rowptr[cur])
                        d = int(rowptr[cur + 1]) - beg
                        cur = int(col_sorted[beg + ((draws[2 * t + 1] * d) >> 32)])
                        if cur not in members:
                            members.append(cur)
                    t += 1
        members.sort()
        out['nodes'][i, :len(members)] = members
        out['len'][i], out['steps'][i] = len(members), t
        out['keys'][i] = tape.set_key_np(members)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------
def _case(seeds=SEEDS, sizes=(8,), per_seed=None, width=None, restart_thr=THR_DEFAULT, max_steps=None):
    sizes = list(sizes)
    width = max(sizes) if width is None else width
    return dict(seeds=np.asarray(seeds, dtype=np.int32), sizes=np.asarray(sizes, dtype=np.int32),
                per_seed=len(sizes) if per_seed is None else per_seed, width=width, restart_thr=restart_thr,
                max_steps=16 * width if max_steps is None else max_steps)


def _sizes_row(sizes, per_seed):
    return [sizes[c % len(sizes)] for c in range(per_seed)]


CASES = {}
for _n in SIZES:
    CASES['size %d' % _n] = _case(sizes=_sizes_row([_n], 2))                             # two candidates of every seed
CASES['mixed'] = _case(sizes=SIZES)
for _thr in THRS:
    CASES['restart_thr %d' % _thr] = _case(sizes=(64, 5), restart_thr=_thr)
for _steps in (0, 1, None):
    CASES['max_steps %s' % ('default' if _steps is None else _steps)] = _case(sizes=(3, 64), max_steps=_steps)
# sizes outside 1 .. width count as clamped: these walk as sizes 1, 4, 4, 2
CASES['clamped'] = _case(sizes=(0, 300, 7, 2), width=4, max_steps=64)
# more items than one trip of the grid-stride loop: short walks from every node of the sparse part
CASES['many'] = _case(seeds=SPARSE, sizes=_sizes_row([2, 3], MANY_PER_SEED), max_steps=8)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition's answer to case ``name``: computed once, shared by the tests (treat as read-only)."""
    rowptr, col = graph()
    return sample(rowptr, col, seed=SEED, stream=STREAM, **CASES[name])


def n_items(name):
    c = CASES[name]
    return len(c['seeds']) * c['per_seed']


def connected(rowptr, col_sorted, members):
    """Do ``members`` induce a connected subgraph?  Union-find over their rows."""
    members = [int(v) for v in members]
    parent = {v: v for v in members}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for v in members:
        for w in col_sorted[rowptr[v]:rowptr[v + 1]].tolist():
            if w in parent:
                parent[find(v)] = find(w)
    return len({find(v) for v in members}) <= 1

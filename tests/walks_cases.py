"""Test helpers of the triangular walks' workgroup-per-walk kernels (triangular_walks_lists_kernel and triangular_walks_wg_kernel
in subgnn_amd/csrc/samplers.hip, through ``ops.triangular_walks(kernel=0 / 2)`` and ``ops.triangular_walks_both``): the graphs and
calls tests/test_gpu_walks.py makes,
the oracle's walks for them, and a step-by-step reading of an oracle walk (``steps``) from which tests/test_walks_cases_host.py
says without a GPU which adjacency form and which branch every case reaches.  numpy and the oracle only; nothing here reads the
GPU or imports the package.

The list kernel answers "is candidate w adjacent to prev?" by the length of N(prev): fewer than LIST_MAX entries -- a hash of the
list in LDS; at least LIST_MAX -- one bit of the graph's hub tables, or, where the graph has none (``hub_tables=False`` in the tests, or
rows with repeated ids), a binary search in global memory.  Lists of more than 64 * CHUNKS[variant] entries are classified twice
(the ballots of the count pass are not kept).  The bitmap kernel (``kernel=2``, and what variant 0 takes for small launches) keeps
N(prev) as bits over node ids, WK_CHUNKS chunks of ballots, and takes further items per workgroup beyond BITMAP_GRID walks."""
import functools

import numpy as np

from oracle import graph as OG, integer_half as IH, tape as T

LIST_MAX = 512                          # WKS_LIST_MAX == DS_SEARCH
WK_CHUNKS = 1024                        # WK_CHUNKS: the largest ballot cache of the variants
CHUNKS = (256, 256, 256, 256, 1024)     # ballot-cache chunks of launch variants 0 .. 4 of the list kernel
THREADS = (512, 256, 512, 1024, 512)    # their workgroup sizes (variant 0: what the launch rule takes where it takes this kernel)
LIST_KERNEL = 2                         # the variant that is variant 0's shape WITHOUT the rule: small launches stay on the list kernel
FEW_WALKS = 256                         # WKS_FEW_WALKS: launches up to this size go to the bitmap kernel under variant 0
BITMAP_GRID = 2048                      # workgroups of a bitmap-kernel launch at the most: walk i + BITMAP_GRID follows walk i on its bitmap
HASH_MAX = 96                           # WK_HASH_MAX: patches / in-border sets up to this size are hashed, longer ones scanned
BETA, SEED = 0.5, 31


def make_graph(n, edges, directed=False):
    """Nodes 1 .. n in id order; neighbour lists in the order the edges are given (an edge given twice: two entries; a self loop:
    one entry).  directed: only u -> v is entered -- a CSR no undirected graph gives, which is the only way a walk can reach a
    node none of whose neighbours is valid (its predecessor always is, in an undirected graph)."""
    adj = {v: [] for v in range(1, n + 1)}
    for u, v in edges:
        adj[u].append(v)
        if u != v and not directed:
            adj[v].append(u)
    return OG.OracleGraph(range(1, n + 1), adj)


@functools.lru_cache(maxsize=None)
def hub_graph(deg, self_loops=False):
    """Node 1 with ``deg`` list entries: leaves 2 .. (deg + 1, or deg with the self loop); leaves 2k, 2k + 1 are linked (triangles
    through the hub), every leaf has a pendant of its own (a list of ONE entry, and a non-triangle candidate).  self_loops: 1 - 1
    and a loop on leaf 2 (a short list that holds its own id)."""
    n_leaves = deg - (1 if self_loops else 0)
    leaves = list(range(2, 2 + n_leaves))
    edges = [(1, 1)] if self_loops else []
    edges += [(1, l) for l in leaves]
    edges += [(leaves[i], leaves[i + 1]) for i in range(0, n_leaves - 1, 2)]
    edges += [(l, l + n_leaves) for l in leaves]
    if self_loops:
        edges.append((2, 2))
    return make_graph(1 + 2 * n_leaves, edges)


@functools.lru_cache(maxsize=None)
def two_hubs_graph(duplicates=False):
    """Hubs 1 and 2, linked, over 600 shared leaves (prev a hub AND curr a hub at the steps 1 -> 2 and 2 -> 1); hub 1 has 40 leaves
    of its own; every fifth leaf has a pendant.  duplicates: the edge 1 - 2, thirty hub - leaf edges and a leaf - pendant edge are
    entered twice (repeated ids in long and in short rows: such a graph has no hub tables)."""
    shared = list(range(3, 603))
    own = list(range(603, 643))
    edges = [(1, 2)] + [(1, l) for l in shared] + [(2, l) for l in shared] + [(1, l) for l in own]
    pend = 643
    for l in shared[::5]:
        edges.append((l, pend))
        pend += 1
    if duplicates:
        edges += [(1, 2)] + [(1, l) for l in shared[:30]] + [(shared[0], 643)]
    return make_graph(pend - 1, edges)


@functools.lru_cache(maxsize=None)
def star_graph():
    """A centre (id 1) with 64 * WK_CHUNKS + 1 leaves -- one entry more than the largest ballot cache holds; leaves 2k, 2k + 1 are
    linked, so that a walk leaf -> centre finds both classes among the centre's candidates."""
    n_leaves = 64 * WK_CHUNKS + 1
    edges = [(1, l) for l in range(2, 2 + n_leaves)] + [(2 * k, 2 * k + 1) for k in range(1, n_leaves // 2 + 1)]
    return make_graph(1 + n_leaves, edges)


@functools.lru_cache(maxsize=None)
def random_graph(n=300, seed=5):
    """Every node links to four earlier ones and node 1 to every third node; ids n - 5 .. n - 3 form a component of their own
    (a patch with no in-border node), n - 2 .. n have no edge (walks that end at their first node)."""
    rng = np.random.default_rng(seed)
    m = n - 6
    edges = set()
    for v in range(2, m + 1):
        for u in rng.integers(1, v, size=4):
            edges.add((int(u), v))
    edges |= {(1, v) for v in range(2, m + 1, 3)}
    edges = sorted(edges, key=lambda e: (e[0] * 7919 + e[1] * 104729) % 1000003)      # list order != id order
    edges += [(n - 5, n - 4), (n - 4, n - 3), (n - 3, n - 5)]
    return make_graph(n, edges)


@functools.lru_cache(maxsize=None)
def dead_end_graph():
    """Directed rows: 1 -> 2 -> 3, 3 has no entry: walks from 1 stop at their third node (no candidate), walks from 2 too."""
    return make_graph(3, [(1, 2), (2, 3)], directed=True)


def sparse_ids_csr(max_id=2_000_000, n_used=400, seed=9):
    """ids up to ``max_id`` (beyond any LDS bitmap over ids), ``n_used`` of them with edges (the largest id among them):
    -> rowptr, col (list order != id order), node_order (the used ids)."""
    rng = np.random.default_rng(seed)
    used = np.unique(np.concatenate([rng.integers(1, max_id, size=n_used - 1), [max_id]])).astype(np.int64)
    rng.shuffle(used)
    pairs = set()
    for i in range(1, len(used)):
        for j in rng.integers(0, i, size=3):
            pairs.add((int(used[j]), int(used[i])))
    rows = {}
    for u, v in sorted(pairs, key=lambda e: (e[0] * 31 + e[1] * 17) % 1000003):
        rows.setdefault(u, []).append(v)
        rows.setdefault(v, []).append(u)
    rowptr = np.zeros(max_id + 2, dtype=np.int64)
    for v, a in rows.items():
        rowptr[v + 1] = len(a)
    rowptr = np.cumsum(rowptr)
    col = np.zeros(int(rowptr[-1]), dtype=np.int32)
    for v, a in rows.items():
        col[rowptr[v]:rowptr[v + 1]] = a
    return rowptr, col, np.sort(used).astype(np.int32)


# ---- the oracle's walks ----------------------------------------------------------------------------------------------------------
def graph_walks(G, n, walk_len, beta=BETA, seed=SEED, item_base=0):
    """mode 0: (n, walk_len) int64, PAD filled -- walk i draws as tape item item_base + i."""
    out = np.zeros((n, walk_len), dtype=np.int64)
    for i in range(n):
        w = IH.triangular_walk(G, walk_len, beta, IH._Draws(seed, T.stream_id(T.STREAM_STRUCT_PATCH), item_base + i), 'graph')
        out[i, :min(len(w), walk_len)] = w[:walk_len]
    return out


def patch_walks(G, views, in_borders, n_walks, walk_len, inside, beta=BETA, seed=SEED):
    """modes 1 / 2: (n_patches * n_walks, walk_len) int64."""
    ref = IH.perform_random_walks(G, np.zeros((len(views), 1), dtype=np.int64), n_walks, walk_len, beta, inside, seed,
                                  patch_orders=views, in_borders=in_borders)
    return ref.reshape(len(views) * n_walks, walk_len)


@functools.lru_cache(maxsize=None)
def patches():
    """Node views over random_graph(): 1, HASH_MAX and HASH_MAX + 1 nodes (hash against linear scan), an empty one, a whole
    component (its in-border set is empty), and a mixed one; in-border sets by the oracle."""
    G = random_graph()
    rng = np.random.default_rng(2)
    m = G.n - 6
    views = [[int(rng.integers(1, m))], [int(v) for v in rng.permutation(m)[:HASH_MAX] + 1],
             [int(v) for v in rng.permutation(m)[:HASH_MAX + 1] + 1], [], [G.n - 5, G.n - 4, G.n - 3],
             [1] + [int(v) for v in rng.permutation(m - 1)[:150] + 2]]
    inb = [IH.patch_in_border_nodes(G, v) for v in views]
    return G, views, inb


# ---- reading a walk ----------------------------------------------------------------------------------------------------------------
def steps(G, walk, ok=lambda v: True):
    """Per step t >= 2 of an oracle walk (PAD trimmed): what the kernel's count pass sees -- the lengths of N(prev) and N(curr),
    the triangle / non-triangle counts among curr's valid candidates; a final entry with nt = nn = 0 when the walk stopped for
    want of candidates is NOT included (``stopped_dead`` says it)."""
    w = [int(v) for v in walk if v != 0]
    out = []
    for t in range(2, len(w)):
        prev, curr = w[t - 2], w[t - 1]
        cand = [x for x in G.neighbors(curr) if ok(x)]
        nt = sum(1 for x in cand if G.has_edge(prev, x))
        out.append({'prev': prev, 'curr': curr, 'prev_len': len(G.neighbors(prev)), 'curr_len': len(G.neighbors(curr)), 'nt': nt,
                    'nn': len(cand) - nt})
    return out


def stopped_dead(G, walk, walk_len, ok=lambda v: True):
    """The walk has at least two nodes, fewer than walk_len, and its last node has no valid candidate (nt + nn == 0)."""
    w = [int(v) for v in walk if v != 0]
    return 2 <= len(w) < walk_len and not [x for x in G.neighbors(w[-1]) if ok(x)]


def stopped_at_start(G, walk, ok=lambda v: True):
    """nn == 0 at the first step: one node, none of whose neighbours is valid."""
    w = [int(v) for v in walk if v != 0]
    return len(w) == 1 and not [x for x in G.neighbors(w[0]) if ok(x)]

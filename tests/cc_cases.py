"""Test helpers of the connected-component kernels (the first part of subgnn_amd/csrc/graph_sets.hip: sgnn_cc_labels,
sgnn_cc_labels_huge, sgnn_cc_compact_stats, sgnn_cc_compact, sgnn_cc_compact_huge): one purpose-built graph whose every answer
is known by construction, single sets at every size the kernels branch on, families of sets beyond every grid cap, and a
vectorised reference -- so that the GPU tests can be shown to reach what they name BEFORE a GPU is asked
(test_cc_cases_host.py).

Nothing here loads the library or touches a device: the constants are read out of the kernels' text."""
import math
import os
import re

import numpy as np

from oracle import graph as OG

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'subgnn_amd', 'csrc')


def _parse():
    with open(os.path.join(_CSRC, 'id_table.h')) as f:
        table = f.read()
    with open(os.path.join(_CSRC, 'graph_sets.hip')) as f:
        text = f.read()

    def one(src, pattern, what):
        m = re.search(pattern, src, re.M)
        if m is None:
            raise RuntimeError('cc_cases: cannot find %s' % what)
        n = 1
        for g in m.groups():
            n *= int(g)
        return n

    c = {name: one(table, r'^\s*#define\s+%s\s+(\d+)\b' % name, name)
         for name in ('SGNN_SET_WAVE_MAX', 'SGNN_SET_LDS_MAX', 'SGNN_SET_LDS_HASH_BITS')}
    c['CCH_THREADS'] = one(text, r'^\s*#define\s+CCH_THREADS\s+(\d+)\b', 'CCH_THREADS')
    caps = {
        'labels_wave': one(text, r'grid = \(int\)\(n_subgraphs < (\d+) \* (\d+) \? n_subgraphs', 'the grid of cc_labels_kernel<64>'),
        'labels_lds': one(text, r'cc_labels_kernel<SGNN_SET_LDS_MAX>, dim3\(grid < (\d+) \?', 'the grid of cc_labels_kernel<2048>'),
        'compact_wave': one(text, r'grid = \(int\)\(n_sub < (\d+) \* (\d+) \? n_sub', 'the grid of cc_compact_kernel<false>'),
        'compact_lds': one(text, r'cc_compact_kernel<true, true>\), dim3\(grid < (\d+) \?', 'the grid of cc_compact_kernel<true>'),
        'labels_huge': one(text, r'cc_huge_labels_kernel, dim3\(\(int\)\(n_subgraphs < (\d+) \?', 'the grid of cc_huge_labels_kernel'),
        'compact_huge': one(text, r'grid = \(int\)\(n_subgraphs < (\d+) \? n_subgraphs', 'the grid of cc_huge_compact_kernel'),
    }
    if one(text, r'cc_compact_kernel<true, false>\), dim3\(grid < (\d+) \?', 'the grid of the statistics form') != caps['compact_lds']:
        raise RuntimeError('cc_cases: the two forms of cc_compact_kernel<true> have different grids')
    return c, caps


CONST, CAPS = _parse()
WAVE_MAX, LDS_MAX, LDS_HASH = CONST['SGNN_SET_WAVE_MAX'], CONST['SGNN_SET_LDS_MAX'], 1 << CONST['SGNN_SET_LDS_HASH_BITS']
CCH_THREADS = CONST['CCH_THREADS']
MAX_ENTRIES = 1 << 23                   # S * C * L of the largest component tensor a test asks for
N_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 2303, 2304, 2305, 4095, 4096, 4097, 5000)


# ---- the kernels' arithmetic, restated -------------------------------------------------------------------------------------------

def tier(n):
    """Which kernels own a set of n entries."""
    if n <= 0:
        return 'empty'
    if n <= WAVE_MAX:
        return 'wave'
    return 'lds' if n <= LDS_MAX else 'workspace'


def chunk(n):
    """Positions per step of the rank and position scans of a set of n entries."""
    return CCH_THREADS if tier(n) == 'workspace' else 64


def pair_index(i, j):
    """cc_labels_kernel's pair number of positions i < j."""
    return j * (j - 1) // 2 + i


def decode_pair(p):
    """cc_labels_kernel's way back from a pair number: a square root in double, then two correcting loops."""
    j = int((1.0 + math.sqrt(1.0 + 8.0 * float(p))) * 0.5)
    while j * (j - 1) // 2 > p:
        j -= 1
    while (j + 1) * j // 2 <= p:
        j += 1
    return p - j * (j - 1) // 2, j


def workspace_slots(n):
    """Slots of the id table of a workspace set: 1 << (32 - clz(2 n - 1))."""
    x = 2 * n - 1
    clz = 32 - x.bit_length()
    return 1 << (32 - clz)


def workspace_bytes(total):
    return 44 * max(total, 0) + 64


# ---- the graph ---------------------------------------------------------------------------------------------------------------------

N_PATH_A, N_PATH_B, N_CLIQUE, N_LEAVES, N_LONELY = 6000, 2600, 70, 3000, 5000
PATH_A0 = 1                                          # ids PATH_A0 .. PATH_A0 + N_PATH_A - 1, consecutive ids adjacent
PATH_B0 = PATH_A0 + N_PATH_A
CLIQUE0 = PATH_B0 + N_PATH_B
HUB = CLIQUE0 + N_CLIQUE
LEAF0 = HUB + 1
COMMON = LEAF0 + N_LEAVES                            # the lonely nodes' one neighbour: in no set
LONELY0 = COMMON + 1
MAX_ID = LONELY0 + N_LONELY - 1
LOOPS_PATH = (PATH_A0 + 6, PATH_A0 + 2999, PATH_A0 + 5998, PATH_B0 + 1300)          # no two of them adjacent
LOOPS_LONELY = tuple(LONELY0 + k for k in (0, 11, 999, 2500, 4999))
LOOPS = LOOPS_LONELY[:2] + LOOPS_PATH[:2] + LOOPS_LONELY[2:] + LOOPS_PATH[2:]


class Parts:
    def __init__(self):
        pairs = [(v, v + 1) for v in range(PATH_A0, PATH_A0 + N_PATH_A - 1)]
        pairs += [(v, v + 1) for v in range(PATH_B0, PATH_B0 + N_PATH_B - 1)]
        pairs += [(u, v) for u in range(CLIQUE0, CLIQUE0 + N_CLIQUE) for v in range(u + 1, CLIQUE0 + N_CLIQUE)]
        pairs += [(HUB, LEAF0 + k) for k in range(N_LEAVES)]
        pairs += [(LONELY0 + k, COMMON) for k in range(N_LONELY)]
        pairs += [(v, v) for v in LOOPS]
        self.pairs = pairs
        self.G = OG.from_edge_pairs(pairs, relabel_plus_one=False)
        self.rowptr, self.col = self.G.csr(sort=True)
        self.max_id = self.G.max_id()
        assert self.max_id == MAX_ID


_PARTS = []


def parts():
    if not _PARTS:
        _PARTS.append(Parts())
    return _PARTS[0]


# ---- single sets: the node lists ---------------------------------------------------------------------------------------------------

def _path_reversed(n, start=0):
    return np.arange(PATH_A0 + start + n - 1, PATH_A0 + start - 1, -1, dtype=np.int32)


def _path_shuffled(n, start=0):
    return (PATH_A0 + start + np.random.default_rng(1000 + n).permutation(n)).astype(np.int32)


def _all_lonely(n, start=0):
    return np.arange(LONELY0 + start, LONELY0 + start + n, dtype=np.int32)


def _two_interleaved(n, sa=0, sb=0):
    out = np.empty(n, dtype=np.int32)
    out[0::2] = PATH_A0 + sa + np.arange((n + 1) // 2)
    out[1::2] = PATH_B0 + sb + np.arange(n // 2)
    return out


def _one_id(n, v=PATH_A0 + 41):
    return np.full(n, v, dtype=np.int32)


def _doubled(n, start=0):
    h = (n + 1) // 2
    seg = np.arange(PATH_A0 + start, PATH_A0 + start + h, dtype=np.int32)
    return np.concatenate([seg, seg[:n - h]])


def last_pair_first(n):
    """Where last_pair_only puts the earlier of its two path nodes: position 0 up to 65 entries; beyond, the earliest position
    whose pair with position n - 1 is still among the last 64 pair numbers (pair_index(i, n - 1) = npairs - (n - 1) + i)."""
    return max(0, n - 1 - WAVE_MAX)


def _last_pair_only(n, start=0, a=PATH_A0 + 100):
    assert n >= 2
    out = _all_lonely(n, start)
    out[last_pair_first(n)] = a
    out[n - 1] = a + 1
    return out


def _star_hub_last(n):
    assert n <= N_LEAVES + 1
    return np.concatenate([np.arange(LEAF0, LEAF0 + n - 1), [HUB]]).astype(np.int32)


def _clique(n):
    assert n <= N_CLIQUE
    return (CLIQUE0 + np.random.default_rng(2000 + n).permutation(N_CLIQUE)[:n]).astype(np.int32)


def _self_loops(n, start=0):
    """Lonely nodes with the members that carry a self loop spread among them; from three entries on the first of those is
    listed once more, in the last position."""
    k = min(len(LOOPS), n)
    pool = [v for v in range(LONELY0, LONELY0 + N_LONELY) if v not in LOOPS_LONELY]
    where = [(i * (n - 1)) // max(k - 1, 1) for i in range(k)]
    out = np.zeros(n, dtype=np.int32)
    fill = np.ones(n, dtype=bool)
    fill[where] = False
    out[where] = LOOPS[:k]
    out[fill] = pool[start:start + n - k]
    if n >= 3:
        out[n - 1] = out[where[0]]
    return out


def _n_self_loops_components(n):
    return n - 1 if n >= 3 else n


# builder -> (node list, sizes, claimed (C, L) of n)
BUILDERS = {
    'path_reversed': (_path_reversed, N_EDGES, lambda n: (1, n)),
    'path_shuffled': (_path_shuffled, N_EDGES, lambda n: (1, n)),
    'all_lonely': (_all_lonely, N_EDGES, lambda n: (n, 1)),
    'two_interleaved': (_two_interleaved, N_EDGES, lambda n: (min(n, 2), (n + 1) // 2)),
    'one_id': (_one_id, N_EDGES, lambda n: (1, 1)),
    'doubled': (_doubled, N_EDGES, lambda n: (1, (n + 1) // 2)),
    'last_pair_only': (_last_pair_only, tuple(n for n in N_EDGES if n >= 2), lambda n: (n - 1, 2)),
    'star_hub_last': (_star_hub_last, tuple(n for n in N_EDGES if n <= N_LEAVES + 1), lambda n: (1, n)),
    'clique': (_clique, tuple(n for n in N_EDGES if n <= N_CLIQUE) + (66, N_CLIQUE), lambda n: (1, n)),
    'self_loops': (_self_loops, N_EDGES, lambda n: (_n_self_loops_components(n), 1)),
}


def case(builder, n):
    fn, _, dims = BUILDERS[builder]
    C, L = dims(n)
    return {'name': '%s_%d' % (builder, n), 'builder': builder, 'n': n, 'nodes': fn(n), 'C': C, 'L': L, 'tier': tier(n)}


_CACHE = {}


def single_cases():
    if 'single' not in _CACHE:
        _CACHE['single'] = [case(b, n) for b, (_, sizes, _) in BUILDERS.items() for n in sizes]
    return _CACHE['single']


# ---- many sets: beyond every grid cap ----------------------------------------------------------------------------------------------

def _family_index(k):
    """A workgroup of a capped grid takes sets k, k + cap, k + 2 cap, ... (every cap is a multiple of 1024): with this index the
    shape AND the length of k + cap differ from those of k."""
    return k + k // 1024


def _wave_nodes(shape, n, k):
    if shape == 'path_reversed':
        return _path_reversed(n, (7 * k) % 5900)
    if shape == 'all_lonely':
        return _all_lonely(n, (3 * k) % 4990)
    a, b = PATH_A0 + (5 * k) % 5900, PATH_B0 + k % 2500                   # 'pair_and_repeat': {a, a + 1} and {b}, a listed twice
    return np.array([a, b, a, a + 1][:n], dtype=np.int32)


def many_wave():
    """16 500 sets of 1-4 entries: beyond the grids of cc_labels_kernel<64> and cc_compact_kernel<false, ...>."""
    if 'many_wave' not in _CACHE:
        shapes = ('path_reversed', 'all_lonely', 'pair_and_repeat')
        out = []
        for k in range(16500):
            c = _family_index(k) % 12
            shape, n = shapes[c % 3], 1 + c // 3
            out.append({'name': 'many_wave[%d]:%s_%d' % (k, shape, n), 'shape': shape, 'nodes': _wave_nodes(shape, n, k)})
        _CACHE['many_wave'] = out
    return _CACHE['many_wave']


def many_block():
    """2100 sets of 65-72 entries: beyond the grids of the LDS forms.  (No path shape here: next to all_lonely's 72 components
    its 72-entry component would take the component tensor beyond MAX_ENTRIES; two_interleaved and doubled have the chains.)"""
    if 'many_block' not in _CACHE:
        shapes = ('two_interleaved', 'all_lonely', 'doubled', 'last_pair_only', 'one_id')
        out = []
        for k in range(2100):
            c = _family_index(k) % 40
            shape, n = shapes[c // 8], 65 + c % 8
            if shape == 'two_interleaved':
                nodes = _two_interleaved(n, (13 * k) % 5900, (7 * k) % 2500)
            elif shape == 'all_lonely':
                nodes = _all_lonely(n, (3 * k) % 4900)
            elif shape == 'doubled':
                nodes = _doubled(n, (11 * k) % 5900)
            elif shape == 'last_pair_only':
                nodes = _last_pair_only(n, (3 * k) % 4900, PATH_A0 + (5 * k) % 5900)
            else:
                nodes = _one_id(n, PATH_B0 + k % 2600)
            out.append({'name': 'many_block[%d]:%s_%d' % (k, shape, n), 'shape': shape, 'nodes': nodes})
        _CACHE['many_block'] = out
    return _CACHE['many_block']


def many_huge():
    """1030 sets of 2049-2060 entries with at most two components each: beyond the grids of the workspace forms."""
    if 'many_huge' not in _CACHE:
        shapes = ('path_reversed', 'two_interleaved', 'doubled')
        out = []
        for k in range(1030):
            c = _family_index(k) % 36
            shape, n = shapes[c % 3], 2049 + c // 3
            if shape == 'path_reversed':
                nodes = _path_reversed(n, (13 * k) % 3900)
            elif shape == 'two_interleaved':
                nodes = _two_interleaved(n, (13 * k) % 3900, (7 * k) % 1500)
            else:
                nodes = _doubled(n, (11 * k) % 3900)
            out.append({'name': 'many_huge[%d]:%s_%d' % (k, shape, n), 'shape': shape, 'nodes': nodes})
        _CACHE['many_huge'] = out
    return _CACHE['many_huge']


FAMILIES = {'many_wave': (many_wave, ('labels_wave', 'compact_wave')), 'many_block': (many_block, ('labels_lds', 'compact_lds')),
            'many_huge': (many_huge, ('labels_huge', 'compact_huge'))}


def mixed():
    """One call in which every kernel finds the others' sets and empty sets between its own."""
    if 'mixed' not in _CACHE:
        empty = {'name': 'empty', 'builder': 'empty', 'n': 0, 'nodes': np.zeros(0, dtype=np.int32), 'C': 0, 'L': 0, 'tier': 'empty'}
        plan = [None, ('path_reversed', 1), None, ('two_interleaved', 64), ('doubled', 65), None, ('path_shuffled', 2048),
                ('path_reversed', 2049), None, None, ('two_interleaved', 4096), ('all_lonely', 64), ('last_pair_only', 65),
                ('star_hub_last', 2049), None, ('one_id', 1), ('doubled', 2048), ('clique', 64), ('self_loops', 65), None,
                ('doubled', 4096), ('path_shuffled', 64), None]
        _CACHE['mixed'] = [dict(empty) if p is None else case(*p) for p in plan]
    return _CACHE['mixed']


# ---- the calls the GPU tests make --------------------------------------------------------------------------------------------------

def calls():
    """name -> list of cases.  The single sets go in two calls, by the shape of their component tensor: 'long' holds the cases of
    at most two components (L up to 5000), 'wide' the rest (C up to 5000, L at most 2) -- all_lonely at 5000 next to
    path_reversed at 5000 would ask for 5000 x 5000 entries per set."""
    if 'calls' not in _CACHE:
        singles = single_cases()
        _CACHE['calls'] = {
            'long': [c for c in singles if c['C'] <= 2],
            'wide': [c for c in singles if c['C'] > 2],
            'mixed': mixed(),
            'many_wave': many_wave(),
            'many_block': many_block(),
            'many_huge': many_huge(),
        }
    return _CACHE['calls']


LOOSE_DIMS = ('long', 'wide', 'mixed', 'many_wave', 'many_block')      # the calls that are also made with dims = (C + 3, L + 5)
DIRECT_LABELS = ('long', 'wide', 'mixed')                               # sgnn_cc_labels alone, next to sets beyond the LDS tables
WORKSPACE_CALLS = (('mixed', 'long'), ('long', 'mixed'))                # (the call, the call whose leftovers it finds in the workspace)


def sets_of(name):
    return [c['nodes'] for c in calls()[name]]


# ---- the reference -----------------------------------------------------------------------------------------------------------------

def ragged(sets):
    lens = np.fromiter((len(s) for s in sets), dtype=np.int64, count=len(sets))
    ptr = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in sets]) if ptr[-1] else np.zeros(0, dtype=np.int32)
    return ptr, flat


class Reference:
    """Of a list of sets: ``labels`` (int32, flat: the smallest position of the entry's component), ``n_components`` and
    ``longest`` per set, and the kept entries (the first occurrence of every id) with their component's rank and their
    position inside it."""

    def __init__(self, ptr, flat, labels, ncc, longest, k_set, k_rank, k_within, k_node):
        self.ptr, self.flat, self.labels, self.n_components, self.longest = ptr, flat, labels, ncc, longest
        self.k_set, self.k_rank, self.k_within, self.k_node = k_set, k_rank, k_within, k_node
        self.n_sets = len(ptr) - 1

    def dims(self):
        """The tight (C, L) of the padded tensor (at least 1 each, as the reference pads)."""
        return (max(int(self.n_components.max()), 1), max(int(self.longest.max()), 1)) if self.n_sets else (1, 1)

    def labels_of(self, s):
        return self.labels[self.ptr[s]:self.ptr[s + 1]]

    def lists(self, s):
        """Canonical component lists of set s: components by first position, nodes in set order, first occurrence kept."""
        a, b = np.searchsorted(self.k_set, [s, s + 1])
        out = [[] for _ in range(int(self.n_components[s]))]
        for r, v in zip(self.k_rank[a:b].tolist(), self.k_node[a:b].tolist()):
            out[r].append(v)
        return out


def reference(graph, sets):
    """Connected components of the induced subgraph of every set, all sets at once: the entries of all sets are the vertices
    of one graph (a repeated id is joined to its first occurrence, a kept entry to the kept entries of its set that its
    neighbour list names), scipy labels it, and ranks and positions are prefix sums.  ``graph`` has ``rowptr`` and ``col``."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rowptr, col = np.asarray(graph.rowptr, dtype=np.int64), np.asarray(graph.col, dtype=np.int64)
    ptr, flat = ragged(sets)
    S, total = len(sets), int(ptr[-1])
    if total == 0:
        z32, z64 = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
        return Reference(ptr, flat, z32, np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32), z64, z64, z64, z64)
    M = len(rowptr) - 1
    el = np.arange(total, dtype=np.int64)
    sid = np.repeat(np.arange(S, dtype=np.int64), np.diff(ptr))
    key = sid * M + flat
    order = np.argsort(key, kind='stable')
    ks = key[order]
    new = np.r_[True, ks[1:] != ks[:-1]]
    ukeys, ufirst = ks[new], order[new]                               # (stable: the smallest entry of every (set, id))
    first = np.empty(total, dtype=np.int64)
    first[order] = ufirst[np.cumsum(new) - 1]
    kept = first == el
    ke = el[kept]
    v = flat[ke].astype(np.int64)
    deg = rowptr[v + 1] - rowptr[v]
    rep = np.repeat(ke, deg)
    off = np.arange(int(deg.sum()), dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg)
    want = sid[rep] * M + col[np.repeat(rowptr[v], deg) + off]
    j = np.minimum(np.searchsorted(ukeys, want), len(ukeys) - 1)
    hit = ukeys[j] == want
    src = np.concatenate([el[~kept], rep[hit]])
    dst = np.concatenate([first[~kept], ufirst[j[hit]]])
    adj = coo_matrix((np.ones(len(src), dtype=np.int8), (src, dst)), shape=(total, total)).tocsr()
    _, comp = connected_components(adj, directed=False)
    _, root_of_comp = np.unique(comp, return_index=True)              # the first = smallest entry of every component
    root = root_of_comp[comp].astype(np.int64)
    labels = (root - ptr[sid]).astype(np.int32)
    is_root = root == el
    cr = np.cumsum(is_root)
    rank_of = cr - 1 - np.r_[0, cr][ptr[sid]]                         # of a root: the roots of its set before it
    ncc = np.bincount(sid[is_root], minlength=S).astype(np.int32)
    kroot = root[ke]
    o = np.lexsort((ke, kroot))
    g = kroot[o]
    start = np.r_[True, g[1:] != g[:-1]]
    idx = np.arange(len(o), dtype=np.int64)
    within = np.empty(len(o), dtype=np.int64)
    within[o] = idx - np.maximum.accumulate(np.where(start, idx, 0))
    longest = np.zeros(S, dtype=np.int64)
    np.maximum.at(longest, sid[ke], within + 1)
    return Reference(ptr, flat, labels, ncc, longest.astype(np.int32), sid[ke], rank_of[kroot], within, v)


def padded(ref, C, L):
    """The expected (S, C, L) int64 component tensor."""
    out = np.zeros((ref.n_sets, C, L), dtype=np.int64)
    out[ref.k_set, ref.k_rank, ref.k_within] = ref.k_node
    return out


def reference_of(name):
    """The reference of a call, computed once and never written."""
    key = 'ref_' + name
    if key not in _CACHE:
        _CACHE[key] = reference(parts(), sets_of(name))
    return _CACHE[key]

"""Test helpers of the degree-sequence kernels (subgnn_amd/csrc/degree_sequence.hip through ``ops.degree_sequence`` and the C
ABI): one "ladder" graph with a node of every neighbour-list length the wave kernel branches on, named sets, and a host model
that says which path of the kernel a set takes -- so that the GPU tests can be shown to reach every path BEFORE a GPU is asked.

Nothing here loads the library: the constants are read out of the kernel's text, the table hash is restated on the host.
Only order-independent facts are modelled (the lanes of a wavefront insert concurrently: the value of the probe count P and
which of two colliding ids moves are not fixed; "P > 1" and "one of two members of slot 1023 wraps to slot 0" are)."""
import os
import re

import numpy as np

from oracle import graph as OG

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'subgnn_amd', 'csrc', 'degree_sequence.hip')


def _parse():
    with open(_SRC) as f:
        text = f.read()

    def one(pattern, what):
        m = re.search(pattern, text, re.M)
        if m is None:
            raise RuntimeError('degree_sequence.hip: cannot find %s' % what)
        return m.group(1)

    c = {name: int(one(r'^\s*#define\s+%s\s+(\d+)\b' % name, name))
         for name in ('DS_BIG', 'DS_SEARCH', 'DS_INFLIGHT', 'DS_FLAT_LOADS', 'DS_HASH_BITS', 'DS_TRIES')}
    items = one(r'ds_mult\s*\[\s*DS_TRIES\s*\]\s*=\s*\{([^}]*)\}', 'ds_mult').split(',')
    mult = []
    for it in items:                                            # a term is an OR of literals: "0x9E3779u | 1u"
        lits = re.findall(r'0[xX][0-9A-Fa-f]+|\d+', it)
        if not lits:
            raise RuntimeError('degree_sequence.hip: a multiplier without a literal: %r' % it)
        k = 0
        for l in lits:
            k |= int(l, 0)
        mult.append(k)
    if len(mult) != c['DS_TRIES']:
        raise RuntimeError('degree_sequence.hip: %d multipliers for DS_TRIES = %d' % (len(mult), c['DS_TRIES']))
    c['MULT'] = tuple(mult)
    c['FEW'] = int(one(r'\bfew\s*=\s*n_sets\s*<=\s*(\d+)', 'the bound of the FEW instantiations'))
    c['INFL_SEARCH'] = int(one(r'INFL\s*=\s*SEARCH\s*\?\s*(\d+)\s*:\s*DS_INFLIGHT', 'the loads in flight of the SEARCH instantiations'))
    with open(os.path.join(os.path.dirname(_SRC), 'id_table.h')) as f:
        text = f.read()
    c['WAVE_MAX'] = int(one(r'^\s*#define\s+SGNN_SET_WAVE_MAX\s+(\d+)\b', 'SGNN_SET_WAVE_MAX'))
    c['LDS_MAX'] = int(one(r'^\s*#define\s+SGNN_SET_LDS_MAX\s+(\d+)\b', 'SGNN_SET_LDS_MAX'))
    return c


CONST = _parse()
DS_BIG, DS_SEARCH, DS_INFLIGHT, DS_FLAT_LOADS = CONST['DS_BIG'], CONST['DS_SEARCH'], CONST['DS_INFLIGHT'], CONST['DS_FLAT_LOADS']
DS_HASH_BITS, DS_TRIES, MULT, FEW, INFL_SEARCH = CONST['DS_HASH_BITS'], CONST['DS_TRIES'], CONST['MULT'], CONST['FEW'], CONST['INFL_SEARCH']
HASH = 1 << DS_HASH_BITS
TAIL_LOADS = 8                      # 64-entry loads of one tail block (the kernel's literal 512 = 8 x 64)
WAVE_MAX, LDS_MAX = CONST['WAVE_MAX'], CONST['LDS_MAX']   # csrc/id_table.h: one wavefront per set | the tables in LDS, up to here


# ---- the table, restated ------------------------------------------------------------------------------------------------------

def slot(u, k):
    return ((((u & 0xFFFFFF) * k) & 0xFFFFFFFF) >> (32 - DS_HASH_BITS)) & (HASH - 1)


def first_clean_try(nodes):
    """The first multiplier under which the distinct ids land in distinct slots; DS_TRIES if none does (then P > 1)."""
    ids = sorted(set(int(v) for v in nodes))
    for t, k in enumerate(MULT):
        if len({slot(u, k) for u in ids}) == len(ids):
            return t
    return DS_TRIES


def wraps(nodes):
    """P > 1 and two distinct members share the last slot under the last multiplier: one of them moves to slot 0 (or beyond)."""
    ids = set(int(v) for v in nodes)
    return first_clean_try(ids) == DS_TRIES and sum(slot(u, MULT[-1]) == HASH - 1 for u in ids) >= 2


# ---- the ladder graph ---------------------------------------------------------------------------------------------------------

N_IDS = 6000
HUB_DEGREES_NAMED = (512, 513, 575, 576, 577, 1023, 1024, 2047, 2048, 2049, 2111, 2112, 2560, 2561, 4200)
STREAM_DEGREES_NAMED = (64, 65, 127, 128, 129, 191, 192, 511)
STREAM_DEGREES_MORE = (200, 257, 330, 400, 448)               # tail blocks with 4, 5, 6, 7 live loads
SHORT_DEGREES_NAMED = (1, 2, 63)
ZERO_IDS = (2, 3000, 5990)
SELF_LOOP_SHORT = 4                                            # a short node with a self loop
N_HUBS = 42
EDGE_DEGREES = SHORT_DEGREES_NAMED + STREAM_DEGREES_NAMED + HUB_DEGREES_NAMED


def _wrap_ids():
    """Three ids <= 3000 in slots HASH - 2, HASH - 1 and HASH - 1 under the last multiplier (1643, 1644, 1645 with the multipliers
    this was written against), found by search."""
    k = MULT[-1]
    last = [u for u in range(5, 3001) if slot(u, k) == HASH - 1 and u not in ZERO_IDS]
    before = [u for u in range(5, 3001) if slot(u, k) == HASH - 2 and u not in ZERO_IDS]
    best = None
    for i, b in enumerate(last):
        for c in last[i + 1:]:
            for a in before:
                span = max(a, b, c) - min(a, b, c)
                if best is None or span < best[0]:
                    best = (span, (a, b, c))
    if best is None:
        raise RuntimeError('no two ids share the last slot under the last multiplier')
    return best[1]


WRAP_IDS = _wrap_ids()


class Ladder:
    """ids 1..6000, symmetric, simple (one self loop on a hub, one on a short node).  ``deg`` is the LENGTH of a neighbour list
    (what the kernel branches on; a self loop is one entry)."""

    def __init__(self):
        rng = np.random.default_rng(20260)
        hub_ids = [50 + 140 * i for i in range(N_HUBS)]                      # hub NUMBER = rank by id (DeviceGraph.hub_tables)
        extra = [520 + 7 * i for i in range(N_HUBS - len(HUB_DEGREES_NAMED))]
        hub_deg = list(HUB_DEGREES_NAMED) + extra
        hub_deg = [hub_deg[i] for i in rng.permutation(N_HUBS)]
        stream_deg = STREAM_DEGREES_NAMED + STREAM_DEGREES_MORE
        stream_ids = [95 + 140 * i for i in range(len(stream_deg))]
        short_ids = [20 + 140 * i for i in range(len(SHORT_DEGREES_NAMED))]
        target = dict(zip(hub_ids, hub_deg))
        target.update(zip(stream_ids, stream_deg))
        target.update(zip(short_ids, SHORT_DEGREES_NAMED))
        target[SELF_LOOP_SHORT] = 5
        special = set(target)
        assert len(special) == N_HUBS + len(stream_deg) + len(short_ids) + 1 and not special & set(ZERO_IDS + WRAP_IDS)
        self.hub_ids, self.stream_ids, self.short_ids = hub_ids, stream_ids, short_ids
        self.hub_number = {v: i for i, v in enumerate(hub_ids)}
        by_deg = {d: v for v, d in target.items()}
        self.self_loop_hub = by_deg[2049]
        self.adjacent_hubs = (by_deg[576], by_deg[1024])
        self.late_hub = hub_ids[-2]                                         # hub number 40, adjacent to hubs 0..3
        adj = {v: {} for v in range(1, N_IDS + 1)}
        pairs = []

        def edge(u, v):
            assert v not in adj[u]
            adj[u][v] = adj[v][u] = None
            pairs.append((u, v))

        edge(self.self_loop_hub, self.self_loop_hub)
        edge(SELF_LOOP_SHORT, SELF_LOOP_SHORT)
        edge(*self.adjacent_hubs)
        for h in hub_ids[:4]:
            if h not in adj[self.late_hub] and h != self.late_hub:
                edge(self.late_hub, h)
        a, b, c = WRAP_IDS                                                   # neighbours of each other: inside their set
        edge(a, b); edge(b, c)
        edge(hub_ids[0], N_IDS)                                              # the last id has an edge: max_id = 6000
        pool = np.array([v for v in range(1, N_IDS + 1) if v not in special and v not in ZERO_IDS], dtype=np.int64)
        for v in sorted(target, key=lambda x: (-target[x], x)):              # longest lists first
            need = target[v] - len(adj[v])
            assert need >= 0
            free = pool[~np.isin(pool, list(adj[v]))]
            for u in rng.choice(free, need, replace=False).tolist():
                edge(v, u)
        self.pairs = pairs
        self.G = OG.from_edge_pairs(pairs, relabel_plus_one=False)
        self.rowptr, self.col = self.G.csr()
        self.max_id = self.G.max_id()
        self.deg = np.diff(self.rowptr)[:self.max_id + 1].astype(np.int64)
        self.target = target
        self.pool = [int(v) for v in pool if self.deg[v] > 0]
        self.node_of_degree = {}
        for v in sorted(target):
            self.node_of_degree.setdefault(int(self.deg[v]), v)
        # a degree dict that is NOT the graph's degree at every third id: an ignored dict shows
        nxdeg = self.deg.copy()
        for v in (self.self_loop_hub, SELF_LOOP_SHORT):
            nxdeg[v] += 1
        self.full_degree = (nxdeg + np.where(np.arange(self.max_id + 1) % 3 == 0, 5, 0)).astype(np.int32)

    def row(self, v):
        return self.col[self.rowptr[v]:self.rowptr[v + 1]]

    def multigraph_csr(self):
        """The same graph with the self-loop hub's row carrying one neighbour twice (and that neighbour's row the hub twice) and
        the self loop listed twice: rows with repeated ids, nothing is searched."""
        h = self.self_loop_hub
        y = int(self.row(h)[70])
        assert y != h
        rows = [self.row(v).tolist() for v in range(self.max_id + 1)]
        rows[h] = rows[h][:1000] + [y] + rows[h][1000:] + [h]
        rows[y] = rows[y] + [h]
        rowptr = np.zeros(self.max_id + 2, dtype=np.int64)
        rowptr[1:] = np.cumsum([len(r) for r in rows])
        return rowptr, np.array([u for r in rows for u in r], dtype=np.int32)


_LADDER = []


def ladder():
    if not _LADDER:
        _LADDER.append(Ladder())
    return _LADDER[0]


# ---- the host model of the wave kernel's paths ---------------------------------------------------------------------------------

def list_class(d, infl):
    """How phase A streams a list of d entries with ``infl`` loads in flight: 'flat' (d < DS_BIG: phase B), else
    (full blocks, tail blocks, live loads of the last tail block, the last load is partial)."""
    if d < DS_BIG:
        return 'flat'
    block = 64 * infl
    full, tail = d // block, d % block
    tail_blocks = -(-tail // (64 * TAIL_LOADS))
    live = -(-(tail - 64 * TAIL_LOADS * (tail_blocks - 1)) // 64) if tail else 0
    return (full, tail_blocks, live, d % 64 != 0)


def facts(nodes, deg, hub_number=None):
    """What the kernel does with this set (|set| <= 64), from its members' list lengths alone."""
    nodes = [int(v) for v in nodes]
    n = len(nodes)
    d = [int(deg[v]) for v in nodes]
    G = 64 // n
    long_lanes = [i for i in range(n) if d[i] >= DS_SEARCH]                 # taken by A0 in lane order, G at a time
    rounds = [long_lanes[i:i + G] for i in range(0, len(long_lanes), G)]
    seen, dup = set(), []
    for v in nodes:
        if v in seen:
            dup.append(v)
        seen.add(v)
    f = {
        'n': n, 'G': G, 'nodes': nodes, 'degrees': d,
        'streamed': [list_class(x, DS_INFLIGHT) for x in d],                # every list streamed (search_long_lists=False, multigraph)
        'streamed_search': [list_class(x, INFL_SEARCH) for x in d],          # a long list without bitmap and without sorted rows
        'long': len(long_lanes),
        'a0_taken': [len(r) for r in rounds],
        'a0_lists': [[nodes[i] for i in r] for r in rounds],
        'first_clean_try': first_clean_try(nodes),
        'wrap': wraps(nodes),
        'flat_total': sum(x for x in d if x < DS_BIG),
        'zero_lanes': [i for i in range(n) if d[i] == 0],
        'dups': dup,
    }
    if hub_number is not None:
        f['a0_parities'] = [sorted({hub_number[nodes[i]] & 1 for i in r}) for r in rounds]
        f['hub_numbers'] = sorted({hub_number[v] for v in nodes if v in hub_number})
    return f


# ---- named cases ---------------------------------------------------------------------------------------------------------------

def _fillers(rng, L, k, exclude, near=()):
    """k distinct short ids not in ``exclude``: half of them neighbours of ``near`` (hits), the rest anywhere (mostly misses)."""
    out, ex = [], set(exclude)
    cand = [int(u) for v in near for u in L.row(v) if L.deg[u] < DS_BIG]
    cand = [cand[i] for i in rng.permutation(len(cand))] if cand else []
    for u in cand:
        if len(out) >= (k + 1) // 2:
            break
        if u not in ex:
            out.append(u); ex.add(u)
    pool = [L.pool[i] for i in rng.permutation(len(L.pool))]
    for u in pool:
        if len(out) >= k:
            break
        if u not in ex:
            out.append(u); ex.add(u)
    assert len(out) == k
    return out


def _flat_set(rng, L, total, extra):
    """Short members whose list lengths add up to ``total`` exactly, plus ``extra`` (zero-degree ids, long lists) in front,
    in the middle and at the end."""
    by = {}
    for v in L.pool:
        by.setdefault(int(L.deg[v]), []).append(v)
    hi = max(d for d in by if d < 40)
    out, left = [], total
    while left:
        want = min(left, hi)
        d = want if (left <= hi and want in by and by[want]) else int(rng.integers(max(hi - 6, 1), hi + 1))
        if d > left or not by.get(d):
            d = max(x for x in by if x <= left and by[x])
        out.append(by[d].pop())
        left -= d
    mid = len(out) // 2
    return [extra[0]] + out[:mid] + [extra[1]] + out[mid:] + [extra[2]]


def _search_table_form(rng, L, n, want, fixed=()):
    """A set of n members holding ``fixed`` whose first_clean_try is ``want``, by seeded search over the fillers."""
    for _ in range(20000):
        s = list(fixed) + _fillers(rng, L, n - len(fixed), fixed, near=fixed or L.hub_ids[:2])
        if first_clean_try(s) == want:
            return s
    raise RuntimeError('no set of %d with first_clean_try %d found' % (n, want))


def _edge_positions(d):
    pos = {0, d - 1, 63, 64, 64 * TAIL_LOADS - 1, 64 * TAIL_LOADS, 64 * DS_INFLIGHT - 1, 64 * DS_INFLIGHT}
    return sorted(p for p in pos if 0 <= p < d)


def _wave_cases():
    L = ladder()
    rng = np.random.default_rng(7)
    hubs = L.hub_ids
    cases = []

    def add(name, nodes, **expect):
        assert 1 <= len(nodes) <= WAVE_MAX, name
        cases.append({'name': name, 'nodes': [int(v) for v in nodes], 'expect': expect})

    # sizes x number of long lists: G = 64 // n lists are searched per round of phase A0
    for n in (1, 3, 21, 22, 32, 33, 64):
        G = 64 // n
        for h in sorted({0, 1, G, G + 1, 2 * G + 1, n if n <= 3 else 0}):
            if h > n or h > N_HUBS:
                continue
            # hubs of consecutive NUMBERS, starting at the late hub's neighbours for the large sets
            start = int(rng.integers(0, N_HUBS - h + 1))
            hs = hubs[start:start + h]
            s = hs + _fillers(rng, L, n - h, hs, near=hs)
            s = [s[i] for i in rng.permutation(n)]
            taken = [G] * (h // G) + ([h % G] if h % G else [])
            add('n%d_long%d' % (n, h), s, n=n, long=h, a0_taken=taken)
    s = hubs[:40] + _fillers(rng, L, 24, hubs, near=hubs[:40])
    add('n64_forty_hubs', s, n=64, long=40, a0_taken=[1] * 40)
    s = [L.late_hub] + hubs[:4] + _fillers(rng, L, 16, hubs, near=[L.late_hub])
    add('n21_late_hub_and_its_early_neighbours', s, n=21, long=5, a0_taken=[3, 2])

    # both sides of every branch point of phase A: the node, and its neighbours at the ends of the list and of the loads
    for d in EDGE_DEGREES:
        v = L.node_of_degree[d]
        row = L.row(v)
        s = [v] + [int(row[p]) for p in _edge_positions(d)]
        s = list(dict.fromkeys(s))
        s += _fillers(rng, L, 3, s)
        add('deg_%d_edges' % d, s, streamed_first=list_class(d, DS_INFLIGHT), streamed_search_first=list_class(d, INFL_SEARCH))
    for d in STREAM_DEGREES_MORE:
        v = L.node_of_degree[d]
        add('deg_%d_tail_loads' % d, [v] + [int(L.row(v)[p]) for p in (0, d - 1)] + _fillers(rng, L, 9, [v], near=[v]),
            streamed_first=list_class(d, DS_INFLIGHT))

    # the flat range of phase B: 128 entries per step
    z = ZERO_IDS
    add('flat_0_zero_degree_only', list(z), flat_total=0, zero_lanes=[0, 1, 2])
    add('flat_0_with_a_hub', [z[0], hubs[5], z[1], L.node_of_degree[128], z[2]], flat_total=0, zero_lanes=[0, 2, 4])
    for total in (127, 128, 129, 256):
        s = _flat_set(rng, L, total, z)
        add('flat_%d_zero_degree_first_middle_last' % total, s, flat_total=total,
            zero_lanes=[0, s.index(z[1]), len(s) - 1])
    s = _flat_set(rng, L, 129, (L.node_of_degree[65], hubs[7], z[0]))
    add('flat_129_between_long_lists', s, flat_total=129)

    # an id listed twice counts once as a neighbour and gets its own output
    h, leaf = hubs[9], L.node_of_degree[1]
    add('dup_hub', [h] + _fillers(rng, L, 8, [h], near=[h]) + [h], dups=[h], long=2)
    add('dup_leaf', [leaf, int(L.row(leaf)[0])] + _fillers(rng, L, 5, [leaf, int(L.row(leaf)[0])]) + [leaf], dups=[leaf])
    sh = L.self_loop_hub
    add('dup_self_loop_hub', [sh] + _fillers(rng, L, 10, [sh], near=[sh]) + [sh, SELF_LOOP_SHORT], dups=[sh], long=2)
    add('self_loop_short_alone', [SELF_LOOP_SHORT], n=1)
    add('self_loop_hub_alone', [sh], n=1, long=1)

    # the forms of the table
    for t in range(DS_TRIES):
        s = _search_table_form(rng, L, 40 if t else 12, t, fixed=(hubs[3 + t], hubs[20 + t]))
        add('table_try_%d' % t, s, first_clean_try=t)
    for n in (48, 64):
        for i in range(3):
            s = _search_table_form(rng, L, n, DS_TRIES, fixed=(hubs[2 * i], hubs[2 * i + 1], L.node_of_degree[192]))
            add('table_probed_n%d_%d' % (n, i), s, first_clean_try=DS_TRIES, n=n)
    a, b, c = WRAP_IDS
    s = _search_table_form(rng, L, 48, DS_TRIES, fixed=(a, b, c, hubs[11], L.node_of_degree[129]))
    add('table_probed_wrap_past_the_last_slot', s, first_clean_try=DS_TRIES, wrap=True)
    return cases


def _block_cases():
    L = ladder()
    rng = np.random.default_rng(11)
    big = [v for v in L.hub_ids if L.deg[v] >= 64 * DS_INFLIGHT]
    cases = []
    for n in (65, 128, 129, 256, 257, 1024, 2048, 2050):
        fixed = big + list(ZERO_IDS) + [SELF_LOOP_SHORT]
        assert L.self_loop_hub in fixed
        s = fixed + _fillers(rng, L, n - len(fixed) - 1, fixed, near=big[:2])
        s = [s[i] for i in rng.permutation(len(s))]
        s.append(s[3])                                                       # a repeated id
        name = ('block_%d' if n <= LDS_MAX else 'workspace_%d') % n
        cases.append({'name': name, 'nodes': [int(v) for v in s], 'expect': {'n': n}})
    return cases


_CASES = {}


def wave_cases():
    if 'wave' not in _CASES:
        _CASES['wave'] = _wave_cases()
    return _CASES['wave']


def block_cases():
    if 'block' not in _CASES:
        _CASES['block'] = _block_cases()
    return _CASES['block']


def many_sets():
    """The wave-tier sets repeated and shuffled beyond the bound of the FEW instantiations, one empty set among them."""
    if 'many' not in _CASES:
        base = [c['nodes'] for c in wave_cases()]
        reps = -(-(FEW + 100) // len(base))
        sets = base * reps
        rng = np.random.default_rng(3)
        sets = [sets[i] for i in rng.permutation(len(sets))]
        sets.insert(len(sets) // 2, [])
        _CASES['many'] = sets
    return _CASES['many']


def case_facts(case):
    L = ladder()
    f = facts(case['nodes'], L.deg, L.hub_number)
    f['streamed_first'] = f['streamed'][0]
    f['streamed_search_first'] = f['streamed_search'][0]
    return f


# ---- what the wave-tier cases must cover, together ----------------------------------------------------------------------------

def _stream(key, pred):
    return lambda f: any(c != 'flat' and pred(*c) for c in f[key])


def _coverage():
    cov = {}
    for key, tag in (('streamed', 'INFL %d' % DS_INFLIGHT), ('streamed_search', 'INFL %d' % INFL_SEARCH)):
        cov[tag + ': no full block'] = _stream(key, lambda full, tb, live, part: full == 0)
        cov[tag + ': one full block'] = _stream(key, lambda full, tb, live, part: full == 1)
        cov[tag + ': two full blocks or more'] = _stream(key, lambda full, tb, live, part: full >= 2)
        cov[tag + ': full blocks and no tail'] = _stream(key, lambda full, tb, live, part: full >= 1 and tb == 0)
        cov[tag + ': full block and a one-entry tail'] = _stream(key, lambda full, tb, live, part: full >= 1 and tb == 1 and live == 1 and part)
        if (INFL_SEARCH if key == 'streamed_search' else DS_INFLIGHT) > 2 * TAIL_LOADS:      # (a tail is shorter than a full block)
            cov[tag + ': two tail blocks'] = _stream(key, lambda full, tb, live, part: tb == 2)
            cov[tag + ': three tail blocks or more'] = _stream(key, lambda full, tb, live, part: tb >= 3)
        for k in range(1, TAIL_LOADS + 1):
            cov[tag + ': last tail block with %d live loads' % k] = _stream(key, lambda full, tb, live, part, k=k: tb >= 1 and live == k)
        cov[tag + ': last load partial'] = _stream(key, lambda full, tb, live, part: tb >= 1 and part)
        cov[tag + ': last load whole'] = _stream(key, lambda full, tb, live, part: tb >= 1 and not part)
    cov['flat: list of DS_BIG - 1 entries'] = lambda f: DS_BIG - 1 in f['degrees']
    cov['A0: no long list'] = lambda f: f['long'] == 0 and f['n'] > 1
    cov['A0: one round of exactly G lists, G >= 2'] = lambda f: f['G'] >= 2 and f['a0_taken'] == [f['G']]
    cov['A0: a round with taken < G'] = lambda f: any(t < f['G'] for t in f['a0_taken'])
    cov['A0: several rounds with G >= 2'] = lambda f: f['G'] >= 2 and len(f['a0_taken']) >= 2
    cov['A0: three rounds or more'] = lambda f: len(f['a0_taken']) >= 3
    cov['A0: G = 3 with an idle lane and three different lists at once'] = \
        lambda f: f['n'] == 21 and any(len(set(r)) == 3 for r in f['a0_lists'])
    cov['A0: n = 64, one list per round'] = lambda f: f['n'] == 64 and f['long'] >= 2
    cov['A0: the same list in two slots of a round'] = lambda f: any(len(set(r)) < len(r) for r in f['a0_lists'])
    cov['A0: a round with numbered and unnumbered lists when every other hub has a bitmap'] = \
        lambda f: any(p == [0, 1] for p in f['a0_parities'])
    cov['A0: a round of one kind when every other hub has a bitmap'] = lambda f: any(len(p) == 1 for p in f['a0_parities'])
    cov['bitmaps: hub numbers on both sides of 32 in one set'] = \
        lambda f: f['hub_numbers'] and f['hub_numbers'][0] < 32 <= f['hub_numbers'][-1]
    for t in range(DS_TRIES):
        cov['table: clean under multiplier %d' % t] = lambda f, t=t: f['first_clean_try'] == t
    cov['table: probed, n = 48'] = lambda f: f['first_clean_try'] == DS_TRIES and f['n'] == 48 and not f['wrap']
    cov['table: probed, n = 64'] = lambda f: f['first_clean_try'] == DS_TRIES and f['n'] == 64
    cov['table: probed with a long list searched'] = lambda f: f['first_clean_try'] == DS_TRIES and f['long'] >= 1
    cov['table: probe wraps past the last slot'] = lambda f: f['wrap']
    for total in (0, 127, 128, 129, 256):
        cov['flat total %d' % total] = lambda f, total=total: f['flat_total'] == total
    cov['zero-degree member in lane 0'] = lambda f: 0 in f['zero_lanes']
    cov['zero-degree member in the middle'] = lambda f: any(0 < i < f['n'] - 1 for i in f['zero_lanes'])
    cov['zero-degree member in lane n - 1'] = lambda f: f['n'] > 1 and f['n'] - 1 in f['zero_lanes']
    cov['a long list listed twice'] = lambda f: any(d >= DS_SEARCH for v, d in zip(f['nodes'], f['degrees']) if v in f['dups'])
    cov['a short list listed twice'] = lambda f: any(d < DS_BIG for v, d in zip(f['nodes'], f['degrees']) if v in f['dups'])
    for n in (1, 3, 21, 22, 32, 33, 64):
        cov['n = %d' % n] = lambda f, n=n: f['n'] == n
    return cov


COVERAGE = _coverage()


def uncovered(cases, coverage=None):
    """The entries of the coverage table that no case reaches."""
    coverage = COVERAGE if coverage is None else coverage
    fs = [case_facts(c) for c in cases]
    return [name for name, pred in coverage.items() if not any(pred(f) for f in fs)]


# ---- the plain reference of the reference -------------------------------------------------------------------------------------

def degree_sequence_plain(rowptr, col, full_degree, sets, sort):
    """gamma.get_degree_sequence on CSR rows with dict / set: a self loop counts twice, a repeated entry as often as listed."""
    oi, oe = [], []
    for s in sets:
        members = set(s)
        ints, exts = [], []
        for v in s:
            row = col[rowptr[v]:rowptr[v + 1]].tolist()
            loops = row.count(v)
            internal = sum(1 for u in row if u in members) + loops
            full = int(full_degree[v]) if full_degree is not None else len(row) + loops
            ints.append(internal); exts.append(full - internal)
        oi += sorted(ints) if sort else ints
        oe += sorted(exts) if sort else exts
    return np.array(oi, dtype=np.int32), np.array(oe, dtype=np.int32)


# ---- hub tables built on the host (the C ABI with a bitmap for every other long list) -------------------------------------------

def partial_hub_tables(rowptr, col, parity):
    """(hub_index, hub_bits (max_id + 1, W) uint32, node records without/with...) numbering only the long lists whose rank among
    the long lists has this parity."""
    max_id = len(rowptr) - 2
    deg = np.diff(rowptr)
    hubs = np.nonzero(deg[:max_id + 1] >= DS_SEARCH)[0]
    numbered = hubs[parity::2]
    W = (len(numbered) + 31) // 32
    hub_index = np.full(max_id + 1, -1, dtype=np.int32)
    hub_index[numbered] = np.arange(len(numbered), dtype=np.int32)
    bits = np.zeros((max_id + 1, W), dtype=np.uint32)
    for h, v in enumerate(numbered):
        np.bitwise_or.at(bits[:, h >> 5], col[rowptr[v]:rowptr[v + 1]], np.uint32(1 << (h & 31)))
    return hub_index, bits, W, len(hubs), len(numbered)


def node_records(rowptr, col, hub_index, full_degree):
    """int32 (max_id + 1, 4) as subgnn_hip.h documents node_info: {row start, degree, hub number (0xffffff: none) | self-loop
    entries << 24, full degree}."""
    max_id = len(rowptr) - 2
    deg = np.diff(rowptr)[:max_id + 1]
    rows = np.repeat(np.arange(max_id + 1), deg)
    loops = np.bincount(rows[col[:len(rows)] == rows], minlength=max_id + 1)
    z = (loops.astype(np.int64) << 24) | np.where(hub_index >= 0, hub_index, 0xffffff).astype(np.int64)
    full = full_degree if full_degree is not None else deg + loops
    rec = np.stack([rowptr[:max_id + 1], deg, z, np.asarray(full, dtype=np.int64)], 1)
    return (rec & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


# ---- ids at and beyond 2^24: the slot is computed from the low 24 bits only ----------------------------------------------------

BIG = 1 << 24


def big_id_graph():
    """(rowptr, col ascending rows, sets): the ladder's short and stream tier on ids [1, 6000] and again on [2^24 + 1, 2^24 + 6000],
    plus cross edges u -- v + 2^24 for every third edge u -- v."""
    if 'big' in _CASES:
        return _CASES['big']
    L = ladder()
    hub = set(L.hub_ids)
    e = np.array([(u, v) for u, v in L.pairs if u not in hub and v not in hub and u != v], dtype=np.int64)
    cross = e[(e[:, 0] + e[:, 1]) % 3 == 0]
    und = np.concatenate([e, e + BIG, np.stack([cross[:, 0], cross[:, 1] + BIG], 1)])
    src = np.concatenate([und[:, 0], und[:, 1]])
    dst = np.concatenate([und[:, 1], und[:, 0]])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    max_id = BIG + N_IDS
    rowptr = np.zeros(max_id + 2, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=max_id + 1), out=rowptr[1:])
    col = dst.astype(np.int32)
    adj_lo = {}
    for u, v in cross.tolist():
        adj_lo.setdefault(u, []).append(v)
    sets, names = [], []
    rng = np.random.default_rng(5)
    centres = [u for u in L.stream_ids if u in adj_lo][:6] + [L.node_of_degree[511]]      # (with its cross edges the last is searched)
    for s in centres:
        row = [int(x) for x in col[rowptr[s]:rowptr[s + 1]] if x < BIG]
        twins = adj_lo[s][:3]                                                # s -- t + 2^24 are edges
        near = [row[i] for i in rng.permutation(len(row))[:8]]
        near = list(dict.fromkeys(twins + near))
        sets.append([s] + near + [s + BIG] + [t + BIG for t in twins]); names.append('both_%d' % s)       # v and v + 2^24: P > 1
        sets.append([s] + near); names.append('low_only_%d' % s)             # t + 2^24 is a neighbour of s and NOT a member
        sets.append([s + BIG] + [t + BIG for t in near]); names.append('high_only_%d' % s)
    _CASES['big'] = (rowptr, col, sets, names)
    return _CASES['big']

"""The definition of the insertion sets (include/subgnn_hip.h: sgnn_insertion_count / sgnn_insertion_write) in numpy, the cases
the tests send through the kernels, and the kernels' dispatch restated (which path a set length takes).  No GPU, no library.

A set is an ascending array of ids without repeats (it may be empty); a candidate row is the same.  The variants of a set are,
in the order of its candidate row, one per candidate that is no member: the ascending set with the candidate inserted.  With
``shared`` there is ONE candidate row, which every set takes."""
import numpy as np

from subgnn_amd import tape

WAVE_MAX = 64            # csrc/id_table.h SGNN_SET_WAVE_MAX: up to here one wavefront per set
LDS_MAX = 1024           # csrc/insertion.hip SGNN_INS_LDS_MAX: beyond it a set is read from global memory
SET_LENGTHS = (0, 1, 2, 63, 64, 65, 200, LDS_MAX, LDS_MAX + 1)
# the chunk edges of a 64-thread and of a 256-thread workgroup (a chunk is one candidate per thread), and several chunks
CAND_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
SHAPES = ('disjoint', 'all_members', 'mixed', 'below', 'above', 'interleaved')
ID_LO, ID_HI = 2000, 200000              # the sets' ids: room for 1000 candidates below and above
WAVE_GRID_CAP = 256 * 32                 # sgnn_grid_for(n_sets, 1, 256 * 32): the workgroups of the wave tier's launch
MANY = 9000                              # one-entry sets of the grid-stride case: more than one trip of that loop
assert MANY > WAVE_GRID_CAP


def path_of(n):
    return 'wave' if n <= WAVE_MAX else ('lds' if n <= LDS_MAX else 'streamed')


def make_set(n, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(np.arange(ID_LO, ID_HI, dtype=np.int64), size=n, replace=False)).astype(np.int32)


def _outside(ids, lo, hi, m, rng):
    """m ids of [lo, hi) that are no members of ``ids``, ascending."""
    pool = np.setdiff1d(np.arange(lo, hi, dtype=np.int64), np.asarray(ids, dtype=np.int64))
    return np.sort(rng.choice(pool, size=m, replace=False)).astype(np.int32)


def make_candidates(ids, m, shape, seed):
    """A candidate row of (up to) m ids for the set ``ids``:
      'disjoint'     m non-members anywhere in the id range;
      'all_members'  members only, so no variant: min(m, n) of them (a row has no repeats);
      'mixed'        every third candidate a member (as many as the set has), the others not;
      'below'        all smaller than the set's first entry: the insertion rank is 0;
      'above'        all larger than its last: the rank is n;
      'interleaved'  non-members between the set's first and last entry: every rank in between."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, dtype=np.int32)
    n = len(ids)
    if shape == 'disjoint':
        return _outside(ids, 1, ID_HI + 2000, m, rng)
    if shape == 'all_members':
        return np.sort(rng.choice(ids, size=min(m, n), replace=False)).astype(np.int32)
    if shape == 'mixed':
        k = min((m + 2) // 3, n)
        inside = rng.choice(ids, size=k, replace=False).astype(np.int32)
        return np.sort(np.concatenate([inside, _outside(ids, 1, ID_HI + 2000, m - k, rng)])).astype(np.int32)
    if shape == 'below':
        return _outside(ids, 1, int(ids[0]) if n else ID_LO, m, rng)
    if shape == 'above':
        top = int(ids[-1]) + 1 if n else ID_HI
        return _outside(ids, top, top + 2000, m, rng)
    if shape == 'interleaved':
        if n < 2 or int(ids[-1]) - int(ids[0]) + 1 - n < m:
            return _outside(ids, 1, ID_HI + 2000, m, rng)
        return _outside(ids, int(ids[0]), int(ids[-1]), m, rng)
    raise ValueError(shape)


def expand(sets, cands, shared=False):
    """-> dict of what the two entries give: ``variants`` (per set), ``ptr`` / ``nodes`` (the variants), ``parent``, ``cand``
    (int32) and ``keys`` (uint64: tape.set_key_np of every variant)."""
    assert len(cands) == (1 if shared else len(sets))
    variants, out, parent, inserted = [], [], [], []
    for s, ids in enumerate(sets):
        ids = np.asarray(ids, dtype=np.int32)
        row = np.asarray(cands[0 if shared else s], dtype=np.int32)
        new = row[~np.isin(row, ids)]
        variants.append(len(new))
        for v in new:
            out.append(np.insert(ids, int(np.searchsorted(ids, v)), v))
            parent.append(s)
            inserted.append(int(v))
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in out])]).astype(np.int64)
    nodes = np.concatenate(out).astype(np.int32) if out else np.zeros(0, dtype=np.int32)
    keys = np.array([tape.set_key_np(v) for v in out], dtype=np.uint64)
    return {'variants': np.array(variants, dtype=np.int64), 'ptr': ptr, 'nodes': nodes,
            'parent': np.array(parent, dtype=np.int32), 'cand': np.array(inserted, dtype=np.int32), 'keys': keys}


def incremental_key(ids, v):
    """The key of ``ids`` with ``v`` inserted by the identity the kernel uses: from the parent's sum, in uint64 wrap-around
    arithmetic -> (key, whether the addition wrapped)."""
    mixed = tape.mix64_np(np.asarray(ids).astype(np.uint64) & np.uint64(0xFFFFFFFF))
    with np.errstate(over='ignore'):
        total = mixed.sum(dtype=np.uint64) if len(ids) else np.uint64(0)
        more = tape.mix64_np(np.uint64(int(v) & 0xFFFFFFFF))
        both = np.uint64(total + more)
        key = tape.mix64_np(both + np.uint64(len(ids) + 2) * np.uint64(0x8CB92BA72F3D8DD7))
    return int(key), bool(both < total)


def single_cases(lengths=SET_LENGTHS, shapes=SHAPES):
    """name -> (sets, candidate rows): every set length (of ``lengths``) alone with a row of every length and shape (of
    ``shapes``).  One set, one row: the per-set and the shared form read the same arrays."""
    cases = {}
    for n in lengths:
        ids = make_set(n, 100 + n)
        for m in CAND_LENGTHS:
            for shape in shapes:
                seed = 7 * n + 3 * m + SHAPES.index(shape)
                cases['n=%d, m=%d, %s' % (n, m, shape)] = ([ids], [make_candidates(ids, m, shape, seed)])
    return cases


def mixed_case():
    """(sets, candidate rows): all set lengths in one list, twice (a set's place must not matter), every shape and row length
    among the rows."""
    lengths = SET_LENGTHS + SET_LENGTHS[::-1]
    sets = [make_set(n, 300 + i) for i, n in enumerate(lengths)]
    rows = [make_candidates(ids, CAND_LENGTHS[(2 * i + 1) % len(CAND_LENGTHS)], SHAPES[i % len(SHAPES)], 900 + i)
            for i, ids in enumerate(sets)]
    return sets, rows


def pool_case():
    """(sets, one row): the sets of ``mixed_case`` and ONE pool that holds up to 20 members of every set and 700 other ids
    (several chunks of either workgroup size)."""
    sets, _rows = mixed_case()
    rng = np.random.default_rng(77)
    inside = np.concatenate([rng.choice(ids, size=min(len(ids), 20), replace=False) for ids in sets if len(ids)])
    pool = np.union1d(inside, rng.choice(np.arange(1, ID_HI + 2000, dtype=np.int64), size=700, replace=False))
    return sets, [pool.astype(np.int32)]


def many_case():
    """(sets, candidate rows): MANY one-entry sets with one candidate each -- a member for every seventh set."""
    ids = np.arange(ID_LO, ID_LO + 2 * MANY, 2, dtype=np.int32)
    sets = [ids[i:i + 1] for i in range(MANY)]
    rows = [ids[i:i + 1] if i % 7 == 0 else (ids[i:i + 1] + (1 if i % 2 else -1)).astype(np.int32) for i in range(MANY)]
    return sets, rows

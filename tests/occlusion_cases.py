"""The definition of the occlusion sets (include/subgnn_hip.h: sgnn_occlusion_count / sgnn_occlusion_write) in numpy, the cases
the tests send through the kernels, and the kernels' dispatch restated (which path a set length takes).  No GPU, no library.

A set is an ascending array of ids without repeats.  Node mode: every entry is a unit.  Component mode: ``labels[i]`` is the
smallest position of an entry in i's component (sgnn_cc_labels); every component is a unit, units ordered by their smallest
position.  A set of fewer than two units has no variants; otherwise unit u gives the set without u's entries, order kept."""
import numpy as np

from subgnn_amd import tape

WAVE_MAX = 64            # csrc/id_table.h SGNN_SET_WAVE_MAX: up to here one wavefront per set
LDS_MAX = 1024           # csrc/occlusion.hip SGNN_OCC_LDS_MAX (sgnn_occlusion_lds_max()): beyond it a set is streamed
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 200, LDS_MAX, LDS_MAX + 1)
SHAPES = ('one', 'two', 'singletons', 'long')


def path_of(n):
    return 'wave' if n <= WAVE_MAX else ('lds' if n <= LDS_MAX else 'streamed')


def make_set(n, seed, id_range=200000):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(np.arange(1, id_range, dtype=np.int64), size=n, replace=False)).astype(np.int32)


def make_labels(n, shape):
    """Component labels of n positions: 'one' component; 'two' interleaved ones (roots 0 and 1); all 'singletons'; one 'long'
    component (root 0, two positions of every three) beside singletons."""
    i = np.arange(n, dtype=np.int32)
    if shape == 'one':
        return np.zeros(n, dtype=np.int32)
    if shape == 'two':
        return (i % 2).astype(np.int32)
    if shape == 'singletons':
        return i
    if shape == 'long':
        return np.where(i % 3 == 1, i, 0).astype(np.int32)
    raise ValueError(shape)


def units_of(n, mode, labels=None):
    """The units of a set of n entries: a list of position arrays, in unit order."""
    if mode == 'node':
        return [np.array([i]) for i in range(n)]
    roots = [i for i in range(n) if labels[i] == i]
    return [np.flatnonzero(labels == r) for r in roots]


def expand(sets, mode, labels=None):
    """-> dict of what the two entries give for the list of sets: ``units``, ``variants`` (per set), ``lens`` (one slot per
    input entry: slot ptr[s] + u = the length of unit u's variant, 0 where none), ``ptr`` / ``nodes`` (the variants), ``parent``,
    ``unit`` (int32) and ``keys`` (uint64: tape.set_key_np of every variant)."""
    in_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    units, variants, lens = [], [], np.zeros(int(in_ptr[-1]), dtype=np.int64)
    out, parent, rank = [], [], []
    for s, ids in enumerate(sets):
        us = units_of(len(ids), mode, None if labels is None else labels[s])
        units.append(len(us))
        variants.append(len(us) if len(us) >= 2 else 0)
        if len(us) < 2:
            continue
        for u, gone in enumerate(us):
            keep = np.ones(len(ids), dtype=bool)
            keep[gone] = False
            out.append(np.asarray(ids)[keep])
            parent.append(s)
            rank.append(u)
            lens[in_ptr[s] + u] = int(keep.sum())
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in out])]).astype(np.int64)
    nodes = np.concatenate(out).astype(np.int32) if out else np.zeros(0, dtype=np.int32)
    keys = np.array([tape.set_key_np(v) for v in out], dtype=np.uint64)
    return {'units': np.array(units, dtype=np.int64), 'variants': np.array(variants, dtype=np.int64), 'lens': lens, 'ptr': ptr,
            'nodes': nodes, 'parent': np.array(parent, dtype=np.int32), 'unit': np.array(rank, dtype=np.int32), 'keys': keys}


def incremental_key(ids, gone):
    """The key of ``ids`` without the positions ``gone`` by the identity the kernel uses: from the parent's sum, in uint64
    wrap-around arithmetic -> (key, whether the subtraction wrapped)."""
    mixed = tape.mix64_np(np.asarray(ids).astype(np.uint64) & np.uint64(0xFFFFFFFF))
    with np.errstate(over='ignore'):
        total = mixed.sum(dtype=np.uint64)
        removed = mixed[gone].sum(dtype=np.uint64)
        n_variant = np.uint64(len(ids) - len(gone))
        key = tape.mix64_np(np.uint64(total - removed) + (n_variant + np.uint64(1)) * np.uint64(0x8CB92BA72F3D8DD7))
    return int(key), bool(total < removed)


def node_cases():
    """name -> list of sets: every length alone, and all of them in one list (twice: a set's place must not matter)."""
    cases = {'n=%d' % n: [make_set(n, 100 + n)] for n in LENGTHS}
    cases['mixed'] = [make_set(n, 300 + i) for i, n in enumerate(LENGTHS + LENGTHS[::-1])]
    return cases


def component_cases():
    """name -> (sets, labels): every label shape at every length alone, and one mixed list of all shapes and lengths."""
    cases, mixed_sets, mixed_labels = {}, [], []
    for shape in SHAPES:
        for n in LENGTHS:
            cases['%s, n=%d' % (shape, n)] = ([make_set(n, 500 + n)], [make_labels(n, shape)])
            mixed_sets.append(make_set(n, 700 + n + len(mixed_sets)))
            mixed_labels.append(make_labels(n, shape))
    cases['mixed'] = (mixed_sets, mixed_labels)
    return cases

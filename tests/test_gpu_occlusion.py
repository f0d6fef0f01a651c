"""-m gpu: the occlusion-set kernels (sgnn_occlusion_count / sgnn_occlusion_write, ops.occlusion_sets) against the numpy
definition of tests/occlusion_cases.py, bit for bit: the counts, the variants' nodes, parents, unit ranks and keys, at every set
length the kernels branch on (each alone and all mixed in one call) and, in component mode, at every label shape.  The entries
are called directly with guard words around every output; refused calls write nothing; a call on another stream gives the
same bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import occlusion_cases as OC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 16
NODE_CASES = OC.node_cases()
COMP_CASES = OC.component_cases()


@functools.lru_cache(maxsize=None)
def _want(mode, name):
    if mode == 'node':
        return OC.expand(NODE_CASES[name], 'node')
    sets, labels = COMP_CASES[name]
    return OC.expand(sets, 'component', labels)


def _ragged(sets):
    from subgnn_amd import ops
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    flat = np.concatenate(list(sets) + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    if flat.size == 0:
        flat = np.zeros(1, dtype=np.int32)                            # (a tensor of no elements has no address)
    return ops.Ragged(torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), max_len=max(len(s) for s in sets))


def _labels(labels):
    flat = np.concatenate(list(labels) + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return torch.from_numpy(flat if flat.size else np.zeros(1, dtype=np.int32)).to(DEV)


class Guarded:
    """A device buffer of ``n`` elements with GUARD sentinel words on either side."""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        # (the address is taken from the whole buffer: an empty slice has none)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _run_entries(sets, mode, labels):
    """The two entries called as ops.occlusion_sets calls them, on guarded outputs -> dict of numpy arrays."""
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    r = _ragged(sets)
    lab = _labels(labels) if labels is not None else None
    code = ops.OCCLUSION_MODES[mode]
    slots = int(sum(len(s) for s in sets))
    wsb = int(lib.sgnn_occlusion_workspace_bytes(slots))
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=DEV)
    units, variants = Guarded(r.n, torch.int64, -7), Guarded(r.n, torch.int64, -7)
    lens = Guarded(slots, torch.int64, -7)
    lens.t.zero_()
    head = (ops._ptr(r.ptr), ops._ptr(r.nodes), r.n, r.max_len, code, ops._ptr(lab))
    assert lib.sgnn_occlusion_count(*head, units.ptr, variants.ptr, lens.ptr, slots, ops._ptr(ws), wsb,
                                    ops._stream()) == 0
    var_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(variants.t, 0)])
    len_scan = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(lens.t, 0)])
    V, T = int(var_ptr[-1]), int(len_scan[-1])
    out_ptr = Guarded(V + 1, torch.int64, -7)
    out_ptr.t.zero_()
    nodes, parent, unit, keys = (Guarded(T, torch.int32, -7), Guarded(V, torch.int32, -7), Guarded(V, torch.int32, -7),
                                 Guarded(V, torch.int64, -7))
    assert lib.sgnn_occlusion_write(*head, ops._ptr(var_ptr), ops._ptr(len_scan), V, out_ptr.ptr, nodes.ptr, parent.ptr, unit.ptr,
                                    keys.ptr, slots, ops._ptr(ws), wsb,
                                    ops._stream()) == 0
    torch.cuda.synchronize()
    bufs = {'units': units, 'variants': variants, 'lens': lens, 'ptr': out_ptr, 'nodes': nodes, 'parent': parent, 'unit': unit,
            'keys': keys}
    for k, b in bufs.items():
        assert b.intact(), 'guard words of ' + k
    got = {k: b.t.cpu().numpy() for k, b in bufs.items()}
    got['keys'] = got['keys'].view(np.uint64)
    return got


def _check(got, want, what):
    for k in ('units', 'variants', 'lens', 'ptr', 'parent', 'unit', 'nodes', 'keys'):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


def _check_ops(sets, mode, labels, want, what):
    """ops.occlusion_sets gives the same, its keys are ops.set_keys of what it wrote, and so does a call on another stream."""
    from subgnn_amd import ops
    r, lab = _ragged(sets), (_labels(labels) if labels is not None else None)
    occ = ops.occlusion_sets(r, mode, lab)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        occ2 = ops.occlusion_sets(r, mode, lab)
    side.synchronize()
    torch.cuda.synchronize()
    for o in (occ, occ2):
        T = int(want['ptr'][-1])
        got = {'units': o.units, 'variants': o.variants, 'ptr': o.sets.ptr, 'nodes': o.sets.nodes[:T], 'parent': o.parent,
               'unit': o.unit, 'keys': o.keys}
        for k, v in got.items():
            v = v.cpu().numpy()
            assert np.array_equal(v.view(np.uint64) if k == 'keys' else v, want[k]), (what, k)
        assert o.sets.max_len >= int(np.diff(want['ptr']).max(initial=0))
    if occ.sets.n:
        assert torch.equal(ops.set_keys(occ.sets), occ.keys), what


@pytest.mark.parametrize('name', list(NODE_CASES))
def test_node_mode(name):
    sets, want = NODE_CASES[name], _want('node', name)
    _check(_run_entries(sets, 'node', None), want, name)
    _check_ops(sets, 'node', None, want, name)


@pytest.mark.parametrize('name', list(COMP_CASES))
def test_component_mode(name):
    (sets, labels), want = COMP_CASES[name], _want('component', name)
    _check(_run_entries(sets, 'component', labels), want, name)
    _check_ops(sets, 'component', labels, want, name)


def test_labels_that_are_no_labels_stay_in_bounds():
    """Labels the kernel cannot take (negative, beyond the position, pointing at an entry that is no root) make the entry a unit
    of its own: nothing is read or written out of bounds, and the outputs are those of the repaired labels."""
    n = 70
    ids = OC.make_set(n, 9)
    bad = OC.make_labels(n, 'long')
    bad[5], bad[6], bad[68] = -3, 40, 2 ** 30                          # negative, behind the entry, beyond the set
    bad[11] = 3                                                        # position 3 labels 0, not itself: no root
    bad[9] = 4                                                         # (position 4 is a root: a label the kernel takes)
    repaired = bad.copy()
    for i in range(n):
        l = int(bad[i])
        repaired[i] = l if (0 <= l < i and bad[l] == l) else i
    want = OC.expand([ids], 'component', [repaired])
    _check(_run_entries([ids], 'component', [bad]), want, 'bad labels')


def test_refused_calls_write_nothing():
    from subgnn_amd import ops, _lib
    lib = _lib.load()
    sets = [OC.make_set(5, 1), OC.make_set(70, 2)]
    r = _ragged(sets)
    lab = _labels([OC.make_labels(5, 'two'), OC.make_labels(70, 'two')])
    outs = [Guarded(8, torch.int64, -7) for _ in range(3)]
    o = [b.ptr for b in outs]
    P, N, st = ops._ptr(r.ptr), ops._ptr(r.nodes), ops._stream()
    refused = [
        lib.sgnn_occlusion_count(P, N, r.n, 70, 2, ops._ptr(lab), o[0], o[1], o[2], 75, None, 0, st),          # unknown mode
        lib.sgnn_occlusion_count(P, N, r.n, 70, -1, ops._ptr(lab), o[0], o[1], o[2], 75, None, 0, st),
        lib.sgnn_occlusion_count(P, N, -2, 70, 0, None, o[0], o[1], o[2], 75, None, 0, st),                    # negative sizes
        lib.sgnn_occlusion_count(P, N, r.n, -1, 0, None, o[0], o[1], o[2], 75, None, 0, st),
        lib.sgnn_occlusion_count(None, N, r.n, 70, 0, None, o[0], o[1], o[2], 75, None, 0, st),                # null pointers
        lib.sgnn_occlusion_count(P, None, r.n, 70, 0, None, o[0], o[1], o[2], 75, None, 0, st),
        lib.sgnn_occlusion_count(P, N, r.n, 70, 1, None, o[0], o[1], o[2], 75, None, 0, st),                   # component mode, no labels
        lib.sgnn_occlusion_count(P, N, r.n, 70, 0, None, None, o[1], o[2], 75, None, 0, st),
        lib.sgnn_occlusion_count(P, N, r.n, 5000, 1, ops._ptr(lab), o[0], o[1], o[2], 75, None, 0, st),        # streamed, no workspace
        lib.sgnn_occlusion_count(P, N, r.n, 0, 1, ops._ptr(lab), o[0], o[1], o[2], 75, o[0], 8, st),           # ... too small a one
    ]
    w = [Guarded(8, torch.int64, -7) for _ in range(2)] + [Guarded(8, torch.int32, -7) for _ in range(3)]
    q = [b.ptr for b in w]
    vp, ls = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(76, dtype=torch.int64, device=DEV)
    VP, LS = ops._ptr(vp), ops._ptr(ls)
    refused += [
        lib.sgnn_occlusion_write(P, N, r.n, 70, 3, None, VP, LS, 4, q[0], q[2], q[3], q[4], q[1], 75, None, 0, st),
        lib.sgnn_occlusion_write(P, N, r.n, 70, 0, None, VP, LS, -4, q[0], q[2], q[3], q[4], q[1], 75, None, 0, st),
        lib.sgnn_occlusion_write(P, N, r.n, 70, 0, None, None, LS, 4, q[0], q[2], q[3], q[4], q[1], 75, None, 0, st),
        lib.sgnn_occlusion_write(P, N, r.n, 70, 0, None, VP, None, 4, q[0], q[2], q[3], q[4], q[1], 75, None, 0, st),
        lib.sgnn_occlusion_write(P, N, r.n, 70, 0, None, VP, LS, 4, None, q[2], q[3], q[4], q[1], 75, None, 0, st),
        lib.sgnn_occlusion_write(P, N, r.n, 70, 0, None, VP, LS, 4, q[0], None, q[3], q[4], q[1], 75, None, 0, st),
        lib.sgnn_occlusion_write(P, N, r.n, 70, 0, None, VP, LS, 4, q[0], q[2], q[3], q[4], None, 75, None, 0, st),
        lib.sgnn_occlusion_write(P, N, r.n, 70, 1, None, VP, LS, 4, q[0], q[2], q[3], q[4], q[1], 75, None, 0, st),
    ]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert all(b.untouched() for b in outs + w)
    with pytest.raises(ValueError):
        ops.occlusion_sets(r, 'edge')
    with pytest.raises(ValueError):
        ops.occlusion_sets(r, 'component')

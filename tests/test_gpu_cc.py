"""-m gpu: the connected-component kernels (the first part of csrc/graph_sets.hip) on the calls of cc_cases.py -- single sets at
every tier boundary, chunk seam and table load, families of sets beyond every grid cap, one call that mixes all tiers with
empty sets -- against the vectorised reference.  Everything is exact.  test_cc_cases_host.py shows, without a GPU, that the
cases reach what they are named after, that the reference agrees with two independent routes, and that no call here asks
for more than 2^23 entries of component tensor.

The compaction kernels are given the REFERENCE's labels (a wrong label shows in the label tests, not as a wrong tensor), no
call passes a shape, a length hint or a workspace smaller than the true one, and every buffer a kernel writes is followed by
guard words."""
import numpy as np
import pytest
import torch

import cc_cases as K
from test_gpu_integer import DEV, _ops

pytestmark = pytest.mark.gpu
_SETUP = {}
CALLS = list(K.calls())
GUARD = 4096                                # words behind every buffer a kernel writes
UNWRITTEN = -7                              # no label, count or length is negative (-1 is sgnn_cc_labels' flag)
GUARD_WORD = 0x5a5a5a5a


def shared():
    """The graph on the device, and per call its sets as Ragged, its reference and the reference's labels on the device: built
    once, never written."""
    if not _SETUP:
        P = K.parts()
        _SETUP['dg'] = _ops().DeviceGraph(P.rowptr, P.col, P.G.node_order, DEV)
        _SETUP['calls'] = {}
    return _SETUP


def call(name):
    S = shared()
    if name not in S['calls']:
        ref = K.reference_of(name)
        lens = np.diff(ref.ptr)
        r = _ops().Ragged(torch.from_numpy(ref.ptr).to(DEV), torch.from_numpy(ref.flat).to(DEV), max_len=int(lens.max()))
        S['calls'][name] = (r, ref, torch.from_numpy(ref.labels).to(DEV), lens > K.LDS_MAX)
    return S['calls'][name]


def _lib():
    from subgnn_amd import _lib as L
    return L.load(), L.check


def _same_flat(got, want, name, ref, what):
    """Arrays aligned with the entries of the call: a difference is reported with the name of its set."""
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        s = int(np.searchsorted(ref.ptr, bad[0], side='right')) - 1
        raise AssertionError('%s, %s: %d of %d entries differ, first in set %d (%s) at position %d: got %d, want %d'
                             % (what, name, len(bad), len(want), s, K.calls()[name][s]['name'], bad[0] - ref.ptr[s],
                                got[bad[0]], want[bad[0]]))


def _same_per_set(got, want, name, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError('%s, %s: %d of %d sets differ, first %d (%s): got %d, want %d'
                             % (what, name, len(bad), len(want), bad[0], K.calls()[name][bad[0]]['name'], got[bad[0]], want[bad[0]]))


def _same_tensor(got, want, name, what):
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        s, c, l = bad[0]
        raise AssertionError('%s, %s: %d entries differ, first at set %d (%s) component %d position %d: got %d, want %d'
                             % (what, name, len(bad), s, K.calls()[name][s]['name'], c, l, got[s, c, l], want[s, c, l]))


def _guarded(n, dtype, fill=UNWRITTEN):
    return torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)


def _guard_intact(t, n, what, fill=UNWRITTEN):
    assert bool((t[n:] == fill).all()), 'written behind its end: ' + what


# ---- labels ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', CALLS)
def test_labels(name):
    ops = _ops()
    r, ref, _, _ = call(name)
    lab = ops.cc_labels(shared()['dg'], r)
    _same_flat(lab.cpu().numpy(), ref.labels, name, ref, 'ops.cc_labels')
    again = ops.cc_labels(shared()['dg'], r)                          # lock-free, and still one answer
    assert torch.equal(lab, again), name


@pytest.mark.parametrize('name', K.DIRECT_LABELS)
def test_sgnn_cc_labels_alone_flags_the_sets_it_does_not_own(name):
    """Next to sets beyond the LDS tables: those hold -1 at every position, every other set is complete, nothing behind the
    last entry is written, and the length hint changes nothing."""
    ops = _ops()
    lib, check = _lib()
    dg = shared()['dg']
    r, ref, _, huge = call(name)
    total = int(ref.ptr[-1])
    assert huge.any() and not huge.all()
    want = ref.labels.copy()
    for s in np.nonzero(huge)[0]:
        want[ref.ptr[s]:ref.ptr[s + 1]] = -1
    for hint in (0, r.max_len):
        out = _guarded(total, torch.int32)
        check(lib.sgnn_cc_labels(ops._ptr(dg.rowptr), ops._ptr(dg.col_sorted), dg.nnz, ops._ptr(r.ptr), ops._ptr(r.nodes), r.n,
                                 hint, ops._ptr(out), ops._stream()), 'sgnn_cc_labels')
        _same_flat(out[:total].cpu().numpy(), want, name, ref, 'sgnn_cc_labels alone, max_sub_len=%d' % hint)
        _guard_intact(out, total, 'labels')


# ---- statistics per subgraph -------------------------------------------------------------------------------------------------------

def _stats(lib, check, ops, r, labels, hint, huge, ws=None, wsb=0):
    """sgnn_cc_compact_stats, then (with sets beyond the LDS tables) sgnn_cc_compact_huge's statistics form -> the two guarded
    arrays after the first and after the second call."""
    ncc, longest = _guarded(r.n, torch.int32), _guarded(r.n, torch.int32)
    check(lib.sgnn_cc_compact_stats(ops._ptr(r.ptr), ops._ptr(r.nodes), ops._ptr(labels), r.n, hint, ops._ptr(ncc), ops._ptr(longest),
                                    ops._stream()), 'sgnn_cc_compact_stats')
    first = (ncc.cpu().numpy(), longest.cpu().numpy())
    if huge.any():
        total = int(r.ptr[-1].item())
        if ws is None:
            wsb = lib.sgnn_cc_huge_workspace_bytes(total)
            ws = torch.empty(wsb // 4 + 1, dtype=torch.int32, device=DEV)
        check(lib.sgnn_cc_compact_huge(ops._ptr(r.ptr), ops._ptr(r.nodes), ops._ptr(labels), r.n, total, 0, 0, 0, ops._ptr(ncc),
                                       ops._ptr(longest), None, ops._ptr(ws), wsb, ops._stream()), 'sgnn_cc_compact_huge')
    return first, (ncc.cpu().numpy(), longest.cpu().numpy())


def _check_stats(first, second, ref, huge, name, what):
    own = ~huge
    for k, (a, b, want) in enumerate(zip(first, second, (ref.n_components, ref.longest))):
        field = ('n_components', 'longest')[k] + ' ' + what
        # the LDS forms write their own sets and the empty ones, and leave the others to the workspace form
        _same_per_set(a[:ref.n_sets], np.where(own, want, UNWRITTEN), name, field + ' (sgnn_cc_compact_stats)')
        _same_per_set(b[:ref.n_sets], want, name, field)
        assert np.all(a[ref.n_sets:] == UNWRITTEN) and np.all(b[ref.n_sets:] == UNWRITTEN), field
    empty = np.diff(ref.ptr) == 0
    assert np.all(second[0][:ref.n_sets][empty] == 0) and np.all(second[1][:ref.n_sets][empty] == 0)


@pytest.mark.parametrize('name', CALLS)
def test_statistics_of_every_subgraph(name):
    """n_components[s] and longest[s] for every s -- through the product only their maxima are ever seen."""
    ops = _ops()
    lib, check = _lib()
    r, ref, labels, huge = call(name)
    for hint in (0, r.max_len):
        first, second = _stats(lib, check, ops, r, labels, hint, huge)
        _check_stats(first, second, ref, huge, name, 'max_sub_len=%d' % hint)


# ---- the component tensor ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', CALLS)
def test_component_tensor(name):
    _ops()
    from subgnn_amd.subgraph_utils import components_from_labels
    r, ref, labels, _ = call(name)
    C, L = ref.dims()
    want = K.padded(ref, C, L)
    out = components_from_labels(r.ptr, r.nodes, labels, r.max_len).cpu().numpy()
    assert out.shape == (ref.n_sets, C, L) and out.dtype == np.int64, (name, out.shape, (C, L))      # the tight shape
    _same_tensor(out, want, name, 'components_from_labels')
    out = components_from_labels(r.ptr, r.nodes, labels, 0).cpu().numpy()            # length unknown: every launch
    _same_tensor(out, want, name, 'components_from_labels, max_sub_len=0')
    out = components_from_labels(r.ptr, r.nodes, labels, r.max_len, dims=(C, L)).cpu().numpy()
    _same_tensor(out, want, name, 'components_from_labels, dims kept')
    if name in K.LOOSE_DIMS:
        # a shape that other ranks' subgraphs made larger: the same block, zeros around it
        want = K.padded(ref, C + 3, L + 5)
        for hint in (r.max_len, 0):
            out = components_from_labels(r.ptr, r.nodes, labels, hint, dims=(C + 3, L + 5)).cpu().numpy()
            _same_tensor(out, want, name, 'components_from_labels, dims larger than needed, max_sub_len=%d' % hint)
        out = components_from_labels(r.ptr, r.nodes, labels, r.max_len, dims_reduce=lambda d: d + torch.tensor([3, 5], device=d.device, dtype=d.dtype))
        _same_tensor(out.cpu().numpy(), want, name, 'components_from_labels, dims_reduce')


# ---- the workspace of the huge forms -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,other', K.WORKSPACE_CALLS)
def test_huge_forms_clear_what_they_use_and_stay_inside_the_workspace(name, other):
    """The workspace is torch.empty memory in the product.  Here it holds zeros, ones in every bit, 0x7f7f7f7f, or what the same
    kernels left there after a call over other subgraphs (another total: every array of the layout starts elsewhere) -- before
    EACH of the three huge launches.  Labels, statistics and tensor are the reference every time; the words behind the declared
    size, behind the labels and behind the tensor are untouched."""
    ops = _ops()
    lib, check = _lib()
    dg = shared()['dg']
    r, ref, labels, huge = call(name)
    ro, refo, labels_o, _ = call(other)
    total, total_o = int(ref.ptr[-1]), int(refo.ptr[-1])
    wsb, wsb_o = lib.sgnn_cc_huge_workspace_bytes(total), lib.sgnn_cc_huge_workspace_bytes(total_o)
    assert wsb == 44 * total + 64 and wsb % 4 == 0 and wsb != wsb_o
    ws = torch.empty(max(wsb, wsb_o) // 4 + GUARD, dtype=torch.int32, device=DEV)
    scratch = torch.empty(total_o, dtype=torch.int32, device=DEV)
    stats_o = torch.empty((2, refo.n_sets), dtype=torch.int32, device=DEV)
    C, L = ref.dims()
    n_out = ref.n_sets * C * L
    want = K.padded(ref, C, L)
    graph = (ops._ptr(dg.rowptr), ops._ptr(dg.col_sorted), dg.nnz)
    sets = (ops._ptr(r.ptr), ops._ptr(r.nodes))

    def poison(fill):
        if fill == 'leftover':
            ws.fill_(0)
            check(lib.sgnn_cc_labels_huge(*graph, ops._ptr(ro.ptr), ops._ptr(ro.nodes), ro.n, total_o, ops._ptr(scratch), ops._ptr(ws),
                                          wsb_o, ops._stream()), 'sgnn_cc_labels_huge')
            check(lib.sgnn_cc_compact_huge(ops._ptr(ro.ptr), ops._ptr(ro.nodes), ops._ptr(labels_o), ro.n, total_o, 0, 0, 0,
                                           ops._ptr(stats_o[0]), ops._ptr(stats_o[1]), None, ops._ptr(ws), wsb_o, ops._stream()),
                  'sgnn_cc_compact_huge')
        else:
            ws.fill_(fill)
        ws[wsb // 4:] = GUARD_WORD

    for fill in (0, -1, 0x7f7f7f7f, 'leftover'):
        what = 'workspace filled with %s' % (fill if isinstance(fill, str) else hex(fill & 0xffffffff))
        # labels
        lab = _guarded(total, torch.int32)
        check(lib.sgnn_cc_labels(*graph, *sets, r.n, r.max_len, ops._ptr(lab), ops._stream()), 'sgnn_cc_labels')
        poison(fill)
        check(lib.sgnn_cc_labels_huge(*graph, *sets, r.n, total, ops._ptr(lab), ops._ptr(ws), wsb, ops._stream()), 'sgnn_cc_labels_huge')
        _same_flat(lab[:total].cpu().numpy(), ref.labels, name, ref, 'labels, ' + what)
        _guard_intact(lab, total, 'labels, ' + what)
        _guard_intact(ws, wsb // 4, 'workspace of sgnn_cc_labels_huge, ' + what, GUARD_WORD)
        # statistics
        poison(fill)
        first, second = _stats(lib, check, ops, r, labels, r.max_len, huge, ws, wsb)
        _check_stats(first, second, ref, huge, name, what)
        _guard_intact(ws, wsb // 4, 'workspace of sgnn_cc_compact_huge (statistics), ' + what, GUARD_WORD)
        # the tensor
        out = torch.zeros(n_out + GUARD, dtype=torch.int64, device=DEV)
        out[n_out:] = UNWRITTEN
        check(lib.sgnn_cc_compact(*sets, ops._ptr(labels), r.n, r.max_len, C, L, ops._ptr(out), ops._stream()), 'sgnn_cc_compact')
        poison(fill)
        check(lib.sgnn_cc_compact_huge(*sets, ops._ptr(labels), r.n, total, 1, C, L, None, None, ops._ptr(out), ops._ptr(ws), wsb,
                                       ops._stream()), 'sgnn_cc_compact_huge')
        _same_tensor(out[:n_out].view(ref.n_sets, C, L).cpu().numpy(), want, name, 'tensor, ' + what)
        _guard_intact(out, n_out, 'tensor, ' + what)
        _guard_intact(ws, wsb // 4, 'workspace of sgnn_cc_compact_huge (write), ' + what, GUARD_WORD)


# ---- another stream ----------------------------------------------------------------------------------------------------------------

def test_on_a_stream_of_its_own():
    ops = _ops()
    from subgnn_amd.subgraph_utils import components_from_labels
    r, ref, labels, _ = call('mixed')
    C, L = ref.dims()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert ops._stream().value == st.cuda_stream != torch.cuda.default_stream().cuda_stream
        lab = ops.cc_labels(shared()['dg'], r)
        out = components_from_labels(r.ptr, r.nodes, labels, r.max_len)
        out0 = components_from_labels(r.ptr, r.nodes, labels, 0, dims=(C, L))
    st.synchronize()
    _same_flat(lab.cpu().numpy(), ref.labels, 'mixed', ref, 'ops.cc_labels on a side stream')
    _same_tensor(out.cpu().numpy(), K.padded(ref, C, L), 'mixed', 'components_from_labels on a side stream')
    _same_tensor(out0.cpu().numpy(), K.padded(ref, C, L), 'mixed', 'components_from_labels on a side stream, dims kept')

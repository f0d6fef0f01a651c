"""CPU: the exact-DTW structure similarity (structure_similarity_fn = 'dtw_exact') -- the float64 restatement the GPU tests
compare large sets against, the C ABI of the three new entries, and the argument checks that need no device."""
import os
import re

import numpy as np
import pytest

from dtw_exact_ref import exact_dtw_distances, exact_dtw_similarities, seeded_set
from oracle import fastdtw_restate as FD

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ENTRIES = ('sgnn_dtw_exact_workspace_bytes', 'sgnn_dtw_exact_similarity', 'sgnn_dtw_exact_similarity_live')


@pytest.mark.parametrize('sort', [True, False])
def test_vectorised_restatement_equals_the_oracle_bit_for_bit(sort):
    """The min-of-predecessors DP, vectorised over the pairs, against oracle.fastdtw_restate.exact_dtw (a first minimum over
    the three SUMS) on the seeded set: equal on all 2928 pairs, bit for bit -- rounding is monotone, so the minimum of the
    sums is the minimum of the predecessors plus the cost.  Also what the set is made of: 3 empty x rows, and fastdtw
    (rule 2) above the exact distance on 10 sorted / 1161 unsorted pairs, so a kernel that computed fastdtw under the new
    name would not pass the GPU test."""
    xs, ys = seeded_set(sort)
    assert len(xs) == 64 and len(ys) == 48 and sum(len(x) == 0 for x in xs) == 3
    got = exact_dtw_distances(xs, ys)
    pairs = above = 0
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            if not x:
                assert np.isnan(got[i, j])
                continue
            want = FD.exact_dtw(x, y, FD.calc_dist)
            assert got[i, j] == want and np.float64(got[i, j]).tobytes() == np.float64(want).tobytes(), (i, j)
            fast = FD.fastdtw(x, y, radius=1, dist=FD.calc_dist, tie_order=2)[0]
            assert fast >= want
            above += fast > want
            pairs += 1
    assert pairs == 2928
    assert above == (10 if sort else 1161)
    sims = exact_dtw_similarities(xs, ys)
    assert sims.dtype == np.float32 and (sims[[len(x) == 0 for x in xs]] == 0).all()
    assert (sims[[len(x) > 0 for x in xs]] > 0).all() and (sims <= 1).all()


def test_restatement_handles_empty_rows_and_single_entries():
    d = exact_dtw_distances([[3], [], [1, 2]], [[3], [], [0, 7, 7]])
    assert d[0, 0] == 0.0 and np.isnan(d[1]).all() and np.isnan(d[:, 1]).all()
    assert d[2, 2] == FD.exact_dtw([1, 2], [0, 7, 7], FD.calc_dist)
    s = exact_dtw_similarities([[3], []], [[3], []])
    assert s.tolist() == [[1.0, 0.0], [0.0, 0.0]]


def _declarations():
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return {m.group(2): (m.group(1).strip(), [a.strip() for a in m.group(3).split(',')])
            for m in re.finditer(r'\b(int64_t|int)\s+(sgnn_dtw_exact_[a-z_]+)\s*\(([^)]*)\)\s*;', txt)}


def test_header_declares_the_entries_and_the_ctypes_table_mirrors_them():
    import ctypes
    from subgnn_amd import _lib
    decl = _declarations()
    assert sorted(decl) == sorted(ENTRIES)

    def ctype(arg):
        if '*' in arg:
            return ctypes.c_void_p
        return ctypes.c_int64 if arg.startswith('int64_t') else ctypes.c_int
    for name in ENTRIES:
        res, args = decl[name]
        want_res, want_args = _lib.SIGNATURES[name]
        assert want_res is (ctypes.c_int64 if res == 'int64_t' else ctypes.c_int), name
        assert [ctype(a) for a in args] == want_args, name
        assert not any('tie_order' in a for a in args), name                 # the exact distance has no predecessor rule
    # the fastdtw entries minus tie_order
    for new, old in (('sgnn_dtw_exact_similarity', 'sgnn_dtw_similarity'), ('sgnn_dtw_exact_similarity_live', 'sgnn_dtw_similarity_live')):
        assert len(_lib.SIGNATURES[new][1]) == len(_lib.SIGNATURES[old][1]) - 1


def test_workspace_query_answers_on_the_host_and_null_arguments_are_errors():
    from subgnn_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    small, large = lib.sgnn_dtw_exact_workspace_bytes(100, 20, 10, 50), lib.sgnn_dtw_exact_workspace_bytes(100, 200, 10, 50)
    # value + 1 and reciprocal of both sides, the lengths; the general kernel's columns grow with the longest x row
    assert small >= 2 * 8 * (100 * 20 + 10 * 50) + 4 * (100 + 10) and large > small
    assert lib.sgnn_dtw_exact_workspace_bytes(0, 0, 0, 0) > 0
    assert lib.sgnn_dtw_exact_similarity(None, None, 1, 1, None, None, 1, 1, 0, None, None, None, 0, None) == -1
    assert lib.sgnn_dtw_exact_similarity_live(None, None, 1, 1, None, None, 1, 1, 0, None, None, None, None, 0, None) == -1
    assert lib.sgnn_abi_version() == 14


def test_unknown_similarity_function_is_rejected_before_the_library_is_touched(monkeypatch):
    from subgnn_amd import _lib, gamma, ops

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(ValueError):
        ops.dtw_similarity(None, None, 1, None, None, 1, fn='nope')
    with pytest.raises(ValueError):
        gamma.calc_dtw('cpu', [1], [1], fn='nope')
    assert ops.DTW_FNS == ('dtw', 'dtw_exact')


def test_dtw_similarity_takes_no_live_range_and_the_blocking_row_count_is_gone():
    """The live range is the grouping's own business (ops.DtwRowPrep), not an argument; the distinct-row count has the
    non-blocking form only."""
    import inspect
    from subgnn_amd import ops
    params = list(inspect.signature(ops.dtw_similarity).parameters)
    assert '_live' not in params
    assert params[:9] == ['x_ptr', 'x_val', 'max_x', 'y_ptr', 'y_val', 'max_y', 'tie_order', 'order_rows', 'dedupe']
    assert [n for n in dir(ops) if n.startswith('distinct_row')] == ['distinct_rows_async', 'distinct_rows_ready']


@pytest.mark.parametrize('pattern,max_vgprs', [
    ('dtw_exact_reg_kernel<12, 4, true>', 128),               # 4 wavefronts per SIMD
    ('dtw_exact_reg_kernel<20, 2, true>', 256),               # 2: column, kept costs, x + 1 and reciprocals = 160 registers
    ('dtw_exact_reg_kernel<32, 2, false>', 256),              # 2
    ('dtw_exact_kernel', 64), ('dtw_exact_prepare_kernel', 64),
])
def test_new_kernels_fit_their_register_budget_without_spills_or_scratch(pattern, max_vgprs):
    import sys
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_resources as KR
    from subgnn_amd import build
    build.build(verbose=False)
    hits = [k for k in KR.kernels(os.path.join(REPO, 'subgnn_amd', 'lib', 'dtw_exact.o')) if pattern in k['demangled']]
    assert len(hits) == 1, pattern
    k = hits[0]
    assert k['vgpr_count'] <= max_vgprs and k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k

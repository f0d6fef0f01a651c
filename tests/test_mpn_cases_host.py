"""Without a GPU: the calls of tests/test_gpu_mpn.py reach every branch of the message-passing layer body that
mpn_cases.branches names, the constants of that restated dispatch are the ones in mpn.hip, common.h and ops.py, and the
inputs make the results independent of the order of every sum: the float32 CPU evaluation, forwards and with the anchors
reversed, equals the float64 one bit for bit."""
import os
import re

import pytest
import torch

import mpn_cases as MC

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
_ids = lambda c: c.name


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def test_case_names_are_unique():
    names = [c.name for c in MC.CASES]
    assert len(set(names)) == len(names)


def test_cases_reach_every_branch():
    reached = {}
    for c in MC.CASES:
        for b in MC.branches(c):
            assert b in MC.BRANCHES, '%s: %s' % (c.name, b)
            reached.setdefault(b, []).append(c.name)
    assert set(reached) == set(MC.BRANCHES), 'not reached: %s' % sorted(set(MC.BRANCHES) - set(reached))


def test_cases_hold_what_the_kernels_branch_on():
    """The shapes and pairings the cases were chosen for, stated once more so that an edit of CASES cannot drop one silently."""
    by = lambda src, **kw: {(c.R, c.A, c.D) for c in MC.CASES if c.src == src and all(getattr(c, k) == v for k, v in kw.items())}
    assert by('gather', det=True) >= {(96, 15, 64), (96, 16, 64), (96, 70, 8), (1200, 130, 256), (2048, 17, 256), (16400, 5, 256),
                                      (33, 1, 4), (33, 5, 4), (7, 3, 256), (96, 0, 64), (0, 5, 64), (16400, 128, 4)}
    assert by('gather', det=False) >= {(96, 70, 64), (8200, 3, 256)}
    assert by('gather', id_div=3, det=True) and by('gather', id_div=3, det=False) and by('gather', id_div=3, plan=True, sel='edge')
    assert by('gather', tap='half', det=True) and by('gather', tap='half', det=False)
    assert by('gather', tap='tap', plan=False) >= {(96, 70, 64), (1200, 130, 256)}
    assert 96 * 70 < MC.SCATTER_TOGETHER_BELOW <= 1200 * 130
    assert by('dense', det=True) >= {(90, 70, 32), (8200, 3, 256)} and by('dense', det=False) >= {(90, 70, 32), (8200, 3, 256)}
    assert by('dense', ids=False, sel='col')
    small = {(150, 13, 8), (4095, 13, 64), (4095, 33, 256), (150, 300, 4)}
    assert by('shared', det=True, knobs=()) >= small and by('shared', det=False, knobs=()) >= small
    off = (('SHARED_GEMM_MIN_ROWS', MC.NEVER),)
    assert (65600, 4, 4) in by('shared', det=True, knobs=off, sel='edge') and (65600, 4, 4) in by('shared', det=False, knobs=off, sel='edge')
    assert (262400, 4, 4) in by('shared', det=False, knobs=off)
    assert {c.sel for c in MC.CASES if c.src == 'gather'} == {'col', 'edge', 'id'}
    # the gate at bp > 0, = 0, < 0, in the kernels and materialised
    for where in ('gate.in_kernel', 'gate.materialised'):
        signs = {(c.bp > 0) - (c.bp < 0) for c in MC.CASES if where in MC.branches(c)}
        assert signs == {-1, 0, 1}, where
    # which gradients exist
    assert {c.grads for c in MC.CASES} >= {(True, False, False), (False, True, False), (False, False, True), (True, True, True)}
    assert {c.outs for c in MC.CASES} == {(True, True), (True, False), (False, True)}
    # the chunk lengths and tilings DESIGN names for these shapes (two of 8; eight of 8 and one of 6; 33, 33, 33, 31; unsplit)
    assert MC.split_chunks(MC.grid_for(96 * 16, 256), 16) == (2, 'anchors')
    assert MC.chunk_lengths(70, MC.split_chunks(MC.grid_for(96 * 2, 256), 70)[0]) == [8] * 8 + [6]
    assert MC.grid_for(1200 * 64, 256) == 300 and MC.chunk_lengths(130, MC.split_chunks(300, 130)[0]) == [33, 33, 33, 31]
    assert MC.split_chunks(MC.grid_for(2048 * 64, 256), 17) == (1, None)
    assert MC.shared_det_tiling(150, 13, 2)[1:] == (4, 38, 1)
    assert MC.shared_det_tiling(4095, 13, 16)[1:] == (8, 512, 1)
    assert MC.shared_det_tiling(4095, 33, 64) == (72, 64, 64, 9)
    assert MC.shared_atomic_tiling(65600, 4, 1) == (64, 1025, 1, 1025)
    assert MC.shared_atomic_tiling(262400, 4, 1) == (64, 4100, 1, 4096)
    ten = next(c for c in MC.CASES if c.bodies)
    assert len(ten.bodies) == 10 and len(set(ten.bodies)) == 10 and all(R * A < MC.SCATTER_TOGETHER_BELOW for R, A in ten.bodies)


def test_inputs_hold_the_edges_the_kernels_skip():
    """PAD ids, weights exactly 0, whole masked rows, a row whose every edge is masked, and -- with bp = 0 under the relu --
    read-out entries that are exactly 0 with a non-zero gradient arriving."""
    for c in MC.CASES:
        inp = MC.inputs(c)
        for k, b in enumerate(inp['bodies']):
            if b['R'] * b['A'] < 20:
                continue
            assert (b['sims'] == 0).any(), c.name
            edge, w, _ = MC._weights(c, b, torch.float64)
            assert (~edge).any() and edge.any(), c.name
            assert (edge & (w == 0)).any() or b['R'] * b['A'] < 200, c.name
            assert (~edge).all(1).any(), c.name
            if c.src == 'gather':
                assert (b['ids'] == 0).any() and inp['x'][0].abs().max() > 0
            if c.relu and c.bp == 0 and c.outs[1]:
                z = MC.reference(c)[0][k][1]
                assert ((z == 0) & ~edge & (b['gz'] != 0)).any(), c.name
        if inp['half'] is not None:
            assert not torch.equal(inp['half'], inp['x']) and torch.equal(inp['half'].half().float(), inp['half'])


def test_constants_are_the_sources():
    src = _read('subgnn_amd', 'csrc', 'mpn.hip')
    defines = {k: int(v) for k, v in re.findall(r'^#define (MPN_\w+) (\d+)\b', src, re.M)}
    mine = {'MPN_U': MC.MPN_U, 'MPN_MAX_BODIES': MC.MAX_BODIES, 'MPN_SH_TILE': MC.SH_TILE, 'MPN_SPLIT_BELOW_GX': MC.SPLIT_BELOW_GX,
            'MPN_SPLIT_MIN_A': MC.SPLIT_MIN_A, 'MPN_SPLIT_WANT': MC.SPLIT_WANT, 'MPN_CHUNK_MIN_A': MC.CHUNK_MIN_A,
            'MPN_DENSE_BWD_GRID_CAP': MC.DENSE_BWD_GRID_CAP, 'MPN_WIDE_GRID_CAP': MC.WIDE_GRID_CAP, 'MPN_SH_FULL_TILES': MC.SH_FULL_TILES,
            'MPN_SH_WANT': MC.SH_WANT, 'MPN_SH_GRID_CAP': MC.SH_GRID_CAP, 'MPN_SH_DET_WANT': MC.SH_DET_WANT}
    assert {k: defines.get(k) for k in mine} == mine
    # the conditions as the source writes them
    for line in ('if (gx < MPN_SPLIT_BELOW_GX && args->A >= MPN_SPLIT_MIN_A) {',
                 'chunks = (MPN_SPLIT_WANT + gx - 1) / gx;',
                 'const int64_t most = (args->A + MPN_CHUNK_MIN_A - 1) / MPN_CHUNK_MIN_A;'):
        assert src.count(line) == 2, line                          # the forward and the atomic GATHER backward
    for line in ('if (n_tiles < MPN_SH_FULL_TILES) {',
                 'const int64_t want = (MPN_SH_WANT + chunks - 1) / chunks;',
                 'const int grid = (int)(n_tiles < MPN_SH_GRID_CAP ? n_tiles : MPN_SH_GRID_CAP);',
                 'const int64_t want = (MPN_SH_DET_WANT + *chunks - 1) / *chunks;',
                 'const int grid = sgnn_grid_for(args->R * D4, 256, MPN_DENSE_BWD_GRID_CAP);',
                 'const int gx = sgnn_grid_for(args->R * args->D, 256, MPN_WIDE_GRID_CAP);',
                 'const int gx = sgnn_grid_for(args->R * D4, 256);'):
        assert src.count(line) == 1, line
    assert src.count('tile_rows < %d ? %d' % (MC.SH_MIN_TILE, MC.SH_MIN_TILE)) == 1 and src.count('tr < %d ? %d' % (MC.SH_MIN_TILE, MC.SH_MIN_TILE)) == 1
    assert src.count('256, MPN_WIDE_GRID_CAP)') == 4               # atomic GATHER backward, edge lists (two entries), wp partials
    assert src.count('__launch_bounds__(%d)' % MC.THREADS) == src.count('__launch_bounds__(') and 'dim3(%d)' % MC.THREADS in src
    common = _read('subgnn_amd', 'csrc', 'common.h')
    m = re.search(r'sgnn_grid_for\(int64_t work_items, int items_per_block, int max_blocks = (\d+) \* (\d+)\)', common)
    assert m and int(m.group(1)) * int(m.group(2)) == MC.GRID_CAP
    from subgnn_amd import ops
    assert ops.SHARED_GEMM_MIN_ROWS == MC.SHARED_GEMM_MIN_ROWS and ops.SCATTER_TOGETHER_BELOW == MC.SCATTER_TOGETHER_BELOW
    assert (ops.SRC_DENSE, ops.SRC_GATHER, ops.SRC_SHARED) == (0, 1, 2)


def test_every_case_is_exact():
    """exact(): sum of |terms| x 2^(their fraction bits) < 2^24 for every output element of EVERY case, the largest ones on
    their coarser grid included: tests/test_gpu_mpn.py compares with torch.equal throughout and has no tolerance."""
    for c in MC.CASES:
        print('%-28s %s' % (c.name, {k: '%.3g' % (v / (1 << 24)) for k, v in MC.exactness(c).items()}))
    assert [c.name for c in MC.CASES if not MC.exact(c)] == []


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(a.double(), b), what


@pytest.mark.parametrize('case', MC.CASES, ids=_ids)
def test_float32_in_either_anchor_order_equals_float64(case):
    """The order-independence the GPU test relies on, shown on the CPU for every case."""
    out64, g64 = MC.reference(case)
    want = dict(MC.leaf_names(case))
    for reverse in (False, True):
        out32, g32 = MC.reference(case, torch.float32, reverse)
        for k, ((a32, z32), (a64, z64)) in enumerate(zip(out32, out64)):
            _same(a32, a64, '%s agg of body %d' % (case.name, k))
            _same(z32, z64, '%s z of body %d' % (case.name, k))
        for name in g64:
            _same(g32[name], g64[name], '%s gradient of %s' % (case.name, name))
    # a gradient arrives exactly where one is wanted and the loss depends on the leaf; none is all zero
    for name, wanted in want.items():
        reaches = case.outs[1] or name == 'x'
        assert (g64[name] is not None) == (wanted and reaches), name
        if g64[name] is not None and any(R * A for R, A in MC.bodies(case)):
            assert g64[name].abs().max() > 0, 'the gradient of %s is all zero: nothing could be wrong with it' % name
    if case.src == 'gather' and g64['x'] is not None:
        assert float(g64['x'][0].abs().max()) == 0.0

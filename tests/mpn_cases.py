"""Test helpers of the message-passing layer body (subgnn_amd/csrc/mpn.hip through ``ops.mpn``): the seeded calls
tests/test_gpu_mpn.py makes, the operation written out in float64 torch on the CPU, a restatement of the dispatch of
mpn.hip / ops._MPN so that tests/test_mpn_cases_host.py can say without a GPU which branches those calls reach, and the
condition under which a call's results do not depend on the order of any sum.  torch-CPU only; nothing here reads the GPU
or imports the package.

The operation, per component row r and anchor slot a (x_ra the anchor's row: E[ids] | X[r, a] | X[a]):
    edge[r, a] = ids != 0 and row_mask[r]                 (DENSE: the given mask)
    w[r, a]    = sims[r, sim_col[a]] | sims[r, a] | sims[r, id - 1]
    agg[r, :]  = sum_a edge * w * x_ra
    z[r, a]    = edge * w * <wp, x_ra> + bp               (relu'd under ``relu``)

Every input lies on a small dyadic grid (``GRIDS``): table and anchor rows k/8 in [-1, 1], wp k/8 in [-1/2, 1/2],
similarities k/8 in [0, 2] (a tenth of them exactly 0), incoming gradients k/8 in [-1, 1], bp a multiple of 1/64.  Every
term of every output is then a multiple of 2^-bits (bits = the fraction bits of the factors' product), and where the sum
of a term's absolute values times 2^bits stays below 2^24 (``exact``) every partial sum in any order is a float32: the
kernels' results, the float32 CPU evaluation and the float64 one agree bit for bit, whatever fma contraction, anchor
chunks, row tiles or atomics do to the order, and the relu gate is decided from the same value on both sides."""
import functools
from collections import namedtuple

import torch

# ---- the constants the dispatch depends on (tests/test_mpn_cases_host.py reads them out of the sources and compares) ---------
THREADS = 256                           # __launch_bounds__(256), dim3(256) of every launch
MPN_U = 4                               # anchors whose loads are in flight together
MAX_BODIES = 8                          # MPN_MAX_BODIES: layer bodies per sgnn_mpn_fwd_many / sgnn_mpn_bwd_edges_many launch
SH_TILE = 64                            # MPN_SH_TILE: most rows of a row tile of the SHARED backward
SPLIT_BELOW_GX = 512                    # MPN_SPLIT_BELOW_GX: anchors are split over grid.y below this many row workgroups ...
SPLIT_MIN_A = 16                        # MPN_SPLIT_MIN_A: ... from this many anchors,
SPLIT_WANT = 1024                       # MPN_SPLIT_WANT: towards this many workgroups,
CHUNK_MIN_A = 8                         # MPN_CHUNK_MIN_A: at least this many anchors per chunk
GRID_CAP = 256 * 16                     # sgnn_grid_for's default max_blocks (common.h): the forward's cap
DENSE_BWD_GRID_CAP = 2048               # MPN_DENSE_BWD_GRID_CAP
WIDE_GRID_CAP = 8192                    # MPN_WIDE_GRID_CAP: atomic GATHER backward, edge lists, wp partials
SH_FULL_TILES = 1024                    # MPN_SH_FULL_TILES: 64-row tiles from this many of them
SH_WANT = 1024                          # MPN_SH_WANT: workgroups the short tiles of the atomic SHARED backward aim at
SH_GRID_CAP = 4096                      # MPN_SH_GRID_CAP: row-tile workgroups of the atomic SHARED backward
SH_DET_WANT = 512                       # MPN_SH_DET_WANT: workgroups the deterministic SHARED backward aims at
SH_MIN_TILE = 4                         # the lower clamp of both tilings
SHARED_GEMM_MIN_ROWS = 4096             # ops.SHARED_GEMM_MIN_ROWS: SHARED calls from here go to the library
SCATTER_TOGETHER_BELOW = 1 << 16        # ops.SCATTER_TOGETHER_BELOW: shorter edge lists into a tapped table wait
NEVER = 1 << 60                         # the value the SHARED_GEMM_MIN_ROWS knob is patched to

BRANCHES = (
    # forward
    'fwd.unsplit.few_anchors', 'fwd.split.by_anchors', 'fwd.split.by_rows', 'fwd.unsplit.many_rows', 'fwd.ragged_chunk',
    'fwd.second_trip', 'fwd.lanes=1', 'fwd.lanes=64', 'fwd.partial_block', 'fwd.A=0', 'fwd.R=0', 'fwd.gather', 'fwd.dense',
    'fwd.shared', 'fwd.half_table', 'fwd.relu', 'fwd.id_div', 'fwd.shared.no_ids', 'fwd.shared.id=0', 'fwd.dense.no_ids',
    'fwd.many', 'fwd.many.second_launch',
    # deterministic GATHER backward
    'edges.own', 'edges.own.tapped', 'edges.planned', 'edges.wait', 'edges.wait.second_launch', 'edges.second_trip',
    'edges.id_div', 'edges.gate', 'edges.no_g_z', 'edges.no_g_agg',
    'wp_partial', 'wp_partial.bias', 'wp_partial.no_bias', 'wp_partial.second_trip', 'wp_partial.half', 'wp_partial.id_div',
    'wp_partial.gate',
    # GATHER backward with float atomics
    'gather_atomic.unsplit', 'gather_atomic.split', 'gather_atomic.second_trip', 'gather_atomic.half', 'gather_atomic.id_div',
    # DENSE backward
    'dense.partial', 'dense.atomic', 'dense.second_trip', 'dense.no_ids',
    # SHARED backward, deterministic
    'shared_det.tile=4', 'shared_det.tile_between', 'shared_det.tile=64', 'shared_det.ragged_tile', 'shared_det.item_chunks>1',
    'shared_det.reduce_one_block', 'shared_det.reduce_blocks>1', 'shared_det.reduce_anchors>256', 'shared_det.bias',
    'shared_det.no_bias', 'shared_det.gate', 'shared_det.id=0', 'shared_det.no_ids',
    # SHARED backward with float atomics
    'shared_atomic.short_tiles', 'shared_atomic.tile=64', 'shared_atomic.tile_loop', 'shared_atomic.id=0',
    # which gradients exist, and where the relu gate is applied
    'g_z=None', 'g_agg=None', 'only_x', 'only_wp', 'only_bp', 'gate.in_kernel', 'gate.materialised', 'bp.summed_outside',
)

# ---- a case -------------------------------------------------------------------------------------------------------------------
# src 'gather' | 'dense' | 'shared'; sel: the weight column 'col' (sim_col) | 'edge' (sims_per_edge) | 'id' (id - 1); ids: DENSE /
# SHARED calls with an id array; rows: a row mask; relu + bp: the fused gate and the bias it is tested at; grads: which of
# (x, wp, bp) require a gradient; outs: which of (agg, z) receive one; det: sorted sums / tile partials (True) or float
# atomics; plan: ops.mpn_edge_plan; tap: None | 'tap' (ops.tap_table) | 'half' (with an fp16 copy that holds OTHER values);
# knobs: ((name in ops, value), ...); grid: a key of GRIDS; bodies: ((R, A), ...) of a call with several lazy bodies.
Case = namedtuple('Case', 'name src R A D N sel ids id_div rows relu bp grads outs det plan tap knobs grid bodies seed',
                  defaults=(300, 'id', True, 1, True, False, 5 / 64, (True, True, True), (True, True), True, False, None, (), 'fine',
                            None, 0))

# grid name -> (fraction bits of each factor, rows' |k| <=, wp's |k| <=, similarities' k <=, gradients' |k| <=)
GRIDS = {'fine': (3, 8, 4, 16, 8), 'coarse': (1, 2, 1, 4, 2)}
_GEMM_OFF = (('SHARED_GEMM_MIN_ROWS', NEVER),)


def _named(cases):
    return [c._replace(seed=i + 1) for i, c in enumerate(cases)]


def _both(c):
    return [c._replace(name=c.name + '-det'), c._replace(name=c.name + '-atomics', det=False)]


_TEN = ((96, 70), (33, 5), (7, 3), (96, 16), (150, 13), (96, 15), (33, 1), (90, 9), (64, 40), (17, 21))

CASES = _named([
    # ---- forward lanes and chunking, GATHER (each with its deterministic backward) ----
    Case('g-96-15-64', 'gather', 96, 15, 64),                                       # no split: A < 16
    Case('g-96-16-64', 'gather', 96, 16, 64, sel='col'),                            # two chunks of 8
    Case('g-96-70-8-relu+', 'gather', 96, 70, 8, sel='edge', relu=True, bp=9 / 64),  # 9 chunks, the last of 6 anchors
    Case('g-1200-130-256-relu0-tap', 'gather', 1200, 130, 256, relu=True, bp=0.0, tap='tap'),   # gx = 300: chunks of 33, 33, 33, 31
    Case('g-2048-17-256-relu-', 'gather', 2048, 17, 256, sel='col', relu=True, bp=-7 / 64),     # gx = 512: unsplit with A >= 16
    Case('g-16400-5-256-relu', 'gather', 16400, 5, 256, relu=True, bp=3 / 64),      # second trip: forward, wp partials, bias items
    Case('g-33-1-4', 'gather', 33, 1, 4),
    Case('g-33-5-4', 'gather', 33, 5, 4, sel='edge'),
    Case('g-7-3-256', 'gather', 7, 3, 256, sel='col'),
    Case('g-96-0-64', 'gather', 96, 0, 64),
    Case('g-0-5-64', 'gather', 0, 5, 64),
    # ---- selection, id_div, which gradients exist ----
    Case('g-96-70-64-div3', 'gather', 96, 70, 64, id_div=3, relu=True, bp=0.0),
    Case('g-97-16-64-div3-edge', 'gather', 97, 16, 64, sel='edge', id_div=3),
    Case('g-96-16-64-no-gz', 'gather', 96, 16, 64, outs=(True, False)),
    Case('g-96-16-64-no-gz-tap', 'gather', 96, 16, 64, outs=(True, False), tap='tap', sel='col'),
    Case('g-96-16-64-no-gagg', 'gather', 96, 16, 64, outs=(False, True), relu=True, bp=0.0),
    Case('g-96-16-64-only-x', 'gather', 96, 16, 64, grads=(True, False, False), relu=True, bp=0.0),
    Case('g-96-16-64-only-wp', 'gather', 96, 16, 64, grads=(False, True, False), relu=True, bp=0.0),
    Case('g-96-16-64-only-bp', 'gather', 96, 16, 64, grads=(False, False, True), relu=True, bp=0.0),
    Case('g-96-16-64-x-wp', 'gather', 96, 16, 64, grads=(True, True, False), relu=True, bp=2 / 64),
    # ---- GATHER backward forms ----
    Case('g-96-70-64-plan', 'gather', 96, 70, 64, sel='edge', id_div=3, plan=True, relu=True, bp=0.0),
    Case('g-96-70-64-plan-tap', 'gather', 96, 70, 64, plan=True, tap='tap', relu=True, bp=-3 / 64),
    Case('g-96-70-64-tap', 'gather', 96, 70, 64, tap='tap', relu=True, bp=0.0),        # R A < SCATTER_TOGETHER_BELOW: the list waits
    Case('g-ten-bodies', 'gather', 0, 0, 64, tap='tap', relu=True, bp=0.0, bodies=_TEN),
    Case('g-16400-128-4-edge', 'gather', 16400, 128, 4, sel='edge', grid='coarse', relu=True, bp=0.0),  # R A > 8192 * 256
    Case('g-96-70-64-atomics', 'gather', 96, 70, 64, det=False, relu=True, bp=0.0),    # the anchor-split form
    Case('g-96-70-64-div3-atomics', 'gather', 96, 70, 64, det=False, id_div=3, sel='col'),
    Case('g-8200-3-256-atomics', 'gather', 8200, 3, 256, det=False, relu=True, bp=4 / 64),       # gx = 8200 > 8192
    # ---- the fp16-stored table ----
    Case('g-96-70-64-half', 'gather', 96, 70, 64, tap='half', relu=True, bp=0.0),
    Case('g-96-16-64-half-div3', 'gather', 96, 16, 64, tap='half', id_div=3, sel='col'),
    Case('g-96-70-64-half-atomics', 'gather', 96, 70, 64, tap='half', det=False, sel='edge'),
    Case('g-33-5-4-half-fwd', 'gather', 33, 5, 4, tap='half', grads=(False, True, True)),   # a table without a gradient: the detached tap
    # ---- DENSE ----
    *_both(Case('d-90-70-32', 'dense', 90, 70, 32, relu=True, bp=0.0)),
    *_both(Case('d-8200-3-256', 'dense', 8200, 3, 256, sel='edge')),                    # R D4 > 2048 * 256
    Case('d-90-9-32-no-ids', 'dense', 90, 9, 32, sel='col', ids=False),
    Case('d-33-5-4', 'dense', 33, 5, 4, sel='edge', ids=False, relu=True, bp=-1 / 64),
    Case('d-7-3-256', 'dense', 7, 3, 256, det=False),
    Case('d-16400-5-256', 'dense', 16400, 5, 256, sel='col', ids=False, relu=True, bp=1 / 64),   # the forward's second trip
    # ---- SHARED through ops.mpn's own kernels (R < SHARED_GEMM_MIN_ROWS) ----
    *_both(Case('s-150-13-8', 'shared', 150, 13, 8, sel='col', ids=False, relu=True, bp=0.0)),
    *_both(Case('s-4095-13-64', 'shared', 4095, 13, 64, sel='id', relu=True, bp=6 / 64)),
    *_both(Case('s-4095-33-256', 'shared', 4095, 33, 256, sel='edge', ids=True, grads=(True, True, False), relu=True, bp=-2 / 64)),
    *_both(Case('s-150-300-4', 'shared', 150, 300, 4, sel='edge', ids=False)),
    Case('s-150-13-8-id-only-x', 'shared', 150, 13, 8, sel='id', grads=(True, False, False), relu=True, bp=0.0),
    Case('s-33-5-4-no-gz', 'shared', 33, 5, 4, sel='col', outs=(True, False)),
    Case('s-7-3-256-no-gagg', 'shared', 7, 3, 256, sel='edge', ids=False, outs=(False, True)),
    Case('s-96-16-64', 'shared', 96, 16, 64, sel='col', ids=True),
    # ---- SHARED past the library threshold, the knob set ----
    *_both(Case('s-65600-4-4', 'shared', 65600, 4, 4, sel='edge', ids=False, grid='coarse', knobs=_GEMM_OFF, relu=True, bp=0.0)),
    Case('s-262400-4-4-atomics', 'shared', 262400, 4, 4, sel='edge', ids=True, grid='coarse', knobs=_GEMM_OFF, det=False, bp=1 / 4),
    Case('s-16400-5-256-atomics', 'shared', 16400, 5, 256, sel='col', ids=False, knobs=_GEMM_OFF, det=False),
])

def bodies(case):
    return tuple(case.bodies) if case.bodies else ((case.R, case.A),)


def knob(case, name, default):
    return dict(case.knobs).get(name, default)


def tapped(case):
    """Whether the call's table carries a gradient accumulator (ops.tap_table makes one only for a table that wants a gradient)."""
    return case.src == 'gather' and case.tap is not None and case.grads[0]


def half(case):
    return case.src == 'gather' and case.tap == 'half'


# ---- the dispatch of mpn.hip and of ops._MPN, restated ---------------------------------------------------------------------------
def grid_for(items, per_block, cap=GRID_CAP):
    """sgnn_grid_for (common.h)."""
    return max(1, min(cap, (items + per_block - 1) // per_block))


def split_chunks(gx, A):
    """The anchor chunks of mpn_fwd_chunks and of the atomic GATHER backward -> (chunks, what clipped them)."""
    if not (gx < SPLIT_BELOW_GX and A >= SPLIT_MIN_A):
        return 1, None
    want = (SPLIT_WANT + gx - 1) // gx
    most = (A + CHUNK_MIN_A - 1) // CHUNK_MIN_A
    return (most, 'anchors') if want > most else (max(want, 1), 'rows')


def chunk_lengths(A, chunks):
    per = (A + chunks - 1) // chunks
    return [max(0, min(per, A - k * per)) for k in range(chunks)]


def shared_atomic_tiling(R, A, D4):
    """sgnn_mpn_bwd, SHARED -> (tile_rows, n_tiles, item chunks, grid.x)."""
    tile, chunks = SH_TILE, 1
    n_tiles = (R + tile - 1) // tile
    if n_tiles < SH_FULL_TILES:
        chunks = (A * D4 + THREADS - 1) // THREADS
        want = (SH_WANT + chunks - 1) // chunks
        tile = min(SH_TILE, max(SH_MIN_TILE, (R + want - 1) // want))
        n_tiles = (R + tile - 1) // tile
    return tile, n_tiles, chunks, min(n_tiles, SH_GRID_CAP)


def shared_det_tiling(R, A, D4):
    """mpn_shared_det_tiling -> (tile_rows before the clamps, tile_rows, n_tiles, item chunks)."""
    chunks = (A * D4 + THREADS - 1) // THREADS
    want = (SH_DET_WANT + chunks - 1) // chunks
    raw = (R + want - 1) // want
    tile = min(SH_TILE, max(SH_MIN_TILE, raw))
    return raw, tile, (R + tile - 1) // tile, chunks


def _fwd_branches(case, R, A, got):
    D4 = case.D // 4
    if A == 0:
        got.add('fwd.A=0')                                            # ops._MPN.forward: no launch, agg = 0
        return
    if R == 0:
        got.add('fwd.R=0')                                            # ops._MPN.forward: ``elif R == 0``, no launch, empty outputs
        return
    got.add('fwd.' + case.src)
    gx = grid_for(R * D4, THREADS)
    chunks, clipped = split_chunks(gx, A)
    if chunks > 1:
        got.add('fwd.split.by_' + clipped)
        if any(n % MPN_U for n in chunk_lengths(A, chunks)):
            got.add('fwd.ragged_chunk')
    elif A < SPLIT_MIN_A and gx < SPLIT_BELOW_GX:
        got.add('fwd.unsplit.few_anchors')
    elif A >= SPLIT_MIN_A and gx >= SPLIT_BELOW_GX:
        got.add('fwd.unsplit.many_rows')
    if R * D4 > gx * THREADS:
        got.add('fwd.second_trip')                                    # t += gx * blockDim.x taken
    if D4 == 1:
        got.add('fwd.lanes=1')
    if D4 == 64:
        got.add('fwd.lanes=64')
    if R * D4 < THREADS:
        got.add('fwd.partial_block')
    if half(case):
        got.add('fwd.half_table')
    if case.relu:
        got.add('fwd.relu')
    if case.src == 'gather' and case.id_div > 1:
        got.add('fwd.id_div')
    if case.src == 'shared' and (case.ids or case.sel != 'id'):
        got.add('fwd.shared.id=0' if case.ids else 'fwd.shared.no_ids')
    if case.src == 'dense' and not case.ids:
        got.add('fwd.dense.no_ids')


def branches(case):
    """The names in BRANCHES that one forward + backward of the case reaches."""
    got = set()
    need_x, need_wp, need_bp = case.grads
    D, D4 = case.D, case.D // 4
    if case.src == 'shared' and any(R >= knob(case, 'SHARED_GEMM_MIN_ROWS', SHARED_GEMM_MIN_ROWS) and A > 0 for R, A in bodies(case)):
        # ops.mpn -> _mpn_shared_gemm: none of mpn.hip would run
        raise ValueError('%s: a SHARED call with R >= SHARED_GEMM_MIN_ROWS goes to the library GEMMs; patch the knob '
                         '(knobs=_GEMM_OFF) to reach the kernels of mpn.hip' % case.name)
    live = [(R, A) for R, A in bodies(case) if R > 0 and A > 0]
    if case.bodies:                                                   # lazy=True, keep_chunks=True: ops.flush_lazy_mpn
        groups = [live[lo:lo + MAX_BODIES] for lo in range(0, len(live), MAX_BODIES)]
        many = [g for g in groups if len(g) > 1]                      # (a group of one goes through sgnn_mpn_fwd)
        if many:
            got.add('fwd.many')
        if len(many) > 1:
            got.add('fwd.many.second_launch')
    waiting = 0
    for R, A in bodies(case):
        _fwd_branches(case, R, A, got)
        g_agg, g_z = case.outs
        if not any(case.grads) or not any(case.outs):
            continue
        if not g_z:
            got.add('g_z=None')
            need_wp_, need_bp_ = False, False                         # ``if g_z is None: need_wp = need_bp = False``
        else:
            need_wp_, need_bp_ = need_wp, need_bp
        if not g_agg:
            got.add('g_agg=None')
        if case.grads == (True, False, False):
            got.add('only_x')
        if case.grads == (False, True, False):
            got.add('only_wp')
        if case.grads == (False, False, True):
            got.add('only_bp')
        gather_det = A > 0 and case.src == 'gather' and case.det and D <= 256
        shared_det = A > 0 and case.src == 'shared' and case.det
        planned = gather_det and case.plan
        in_kernel = case.relu and g_z and (need_x or need_wp_) and ((gather_det and not planned) or shared_det)
        if case.relu and g_z:
            got.add('gate.in_kernel' if in_kernel else 'gate.materialised')
        gbp_made = False
        if not ((need_x or need_wp_) and A > 0):
            pass
        elif gather_det:
            if need_x:
                if planned:
                    got.add('edges.planned')
                elif tapped(case) and 0 < R * A < knob(case, 'SCATTER_TOGETHER_BELOW', SCATTER_TOGETHER_BELOW):
                    got.add('edges.wait')
                    waiting += 1
                else:
                    got.add('edges.own.tapped' if tapped(case) else 'edges.own')
                if R * A > WIDE_GRID_CAP * THREADS:
                    got.add('edges.second_trip')
                if case.id_div > 1:
                    got.add('edges.id_div')                           # (a plan's list is made by the same kernel)
                if in_kernel:
                    got.add('edges.gate')
                if not g_z:
                    got.add('edges.no_g_z')
                if not g_agg:
                    got.add('edges.no_g_agg')
            if need_wp_:
                got.add('wp_partial')
                got.add('wp_partial.bias' if need_bp_ else 'wp_partial.no_bias')
                gbp_made = need_bp_
                if R * (D + (1 if need_bp_ else 0)) > WIDE_GRID_CAP * THREADS:
                    got.add('wp_partial.second_trip')
                if half(case):
                    got.add('wp_partial.half')
                if case.id_div > 1:
                    got.add('wp_partial.id_div')
                if in_kernel:
                    got.add('wp_partial.gate')
        elif shared_det:
            raw, tile, n_tiles, chunks = shared_det_tiling(R, A, D4)
            got.add('shared_det.tile=4' if raw < SH_MIN_TILE else 'shared_det.tile=64' if raw > SH_TILE else 'shared_det.tile_between')
            if R % tile:
                got.add('shared_det.ragged_tile')
            if chunks > 1:
                got.add('shared_det.item_chunks>1')
            got.add('shared_det.reduce_one_block' if (A * D + THREADS - 1) // THREADS == 1 else 'shared_det.reduce_blocks>1')
            if A > THREADS and need_wp_:
                got.add('shared_det.reduce_anchors>256')
            gbp_made = need_bp_ and g_z
            got.add('shared_det.bias' if gbp_made else 'shared_det.no_bias')
            if in_kernel:
                got.add('shared_det.gate')
            if case.ids or case.sel != 'id':
                got.add('shared_det.id=0' if case.ids else 'shared_det.no_ids')
        elif case.src == 'shared':
            tile, n_tiles, chunks, gx = shared_atomic_tiling(R, A, D4)
            got.add('shared_atomic.tile=64' if (R + SH_TILE - 1) // SH_TILE >= SH_FULL_TILES else 'shared_atomic.short_tiles')
            if n_tiles > gx:
                got.add('shared_atomic.tile_loop')
            if case.ids:
                got.add('shared_atomic.id=0')
        elif case.src == 'dense':
            if need_wp_:
                got.add('dense.partial' if case.det else 'dense.atomic')
            if R * D4 > DENSE_BWD_GRID_CAP * THREADS:
                got.add('dense.second_trip')
            if not case.ids:
                got.add('dense.no_ids')
        else:
            gx = grid_for(R * D, THREADS, WIDE_GRID_CAP)
            got.add('gather_atomic.split' if split_chunks(gx, A)[0] > 1 else 'gather_atomic.unsplit')
            if R * D > gx * THREADS:
                got.add('gather_atomic.second_trip')
            if half(case) and need_wp_:
                got.add('gather_atomic.half')
            if case.id_div > 1:
                got.add('gather_atomic.id_div')
        if need_bp_ and not gbp_made:
            got.add('bp.summed_outside')
    if waiting > MAX_BODIES:
        got.add('edges.wait.second_launch')                           # _GradAcc.flush: eight bodies per sgnn_mpn_bwd_edges_many
    return got


def entries(case):
    """{library entry: calls} that one forward + backward of the case makes, of the entries of mpn.hip that launch."""
    from collections import Counter
    n = Counter()
    if case.src == 'shared' and any(R >= knob(case, 'SHARED_GEMM_MIN_ROWS', SHARED_GEMM_MIN_ROWS) and A > 0 for R, A in bodies(case)):
        return n
    live = [(R, A) for R, A in bodies(case) if R > 0 and A > 0]
    if case.bodies:
        for lo in range(0, len(live), MAX_BODIES):
            n['sgnn_mpn_fwd' if len(live[lo:lo + MAX_BODIES]) == 1 else 'sgnn_mpn_fwd_many'] += 1
    else:
        n['sgnn_mpn_fwd'] += len(live)
    if case.plan:
        n['sgnn_mpn_bwd_edges'] += len(live)                          # ops.mpn_edge_plan
    need_x, need_wp, need_bp = case.grads
    g_agg, g_z = case.outs
    need_wp = need_wp and g_z
    waiting = 0
    for R, A in live:
        if not (need_x or need_wp) or not any(case.outs):
            continue
        if case.src == 'gather' and case.det and case.D <= 256:
            if need_x and not case.plan:
                if tapped(case) and R * A < knob(case, 'SCATTER_TOGETHER_BELOW', SCATTER_TOGETHER_BELOW):
                    waiting += 1
                else:
                    n['sgnn_mpn_bwd_edges'] += 1
            if need_wp:
                n['sgnn_mpn_bwd_wp_partial'] += 1
        elif case.src == 'shared' and case.det:
            n['sgnn_mpn_bwd_shared_det'] += 1
        else:
            n['sgnn_mpn_bwd'] += 1
    n['sgnn_mpn_bwd_edges_many'] += (waiting + MAX_BODIES - 1) // MAX_BODIES
    return +n


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _signed(shape, k, bits, g):
    return torch.randint(-k, k + 1, shape, generator=g).to(torch.float32) / (1 << bits)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The float32 / integer CPU inputs of a case: {'x', 'half' (values of the fp16 copy, or None), 'bodies': one dict per
    layer body with R, A, ids, edge_mask, row_mask, sims, sim_col, wp, bp, gagg, gz}.  Never modified."""
    g = torch.Generator().manual_seed(7000 + case.seed)
    bits, kx, kwp, kw, kg = GRIDS[case.grid]
    D, N = case.D, case.N
    out = {'half': None, 'bodies': []}
    if case.src == 'gather':
        out['x'] = _signed((N + 1, D), kx, bits, g)                  # row 0, the PAD row, holds values: nothing may read them
        if half(case):
            out['half'] = _signed((N + 1, D), kx, bits, g)
    for R, A in bodies(case):
        b = {'R': R, 'A': A, 'ids': None, 'edge_mask': None, 'row_mask': None, 'sim_col': None}
        if case.src == 'gather':
            n_id = (R + case.id_div - 1) // case.id_div
            ids = torch.randint(1, N + 1, (n_id, A), generator=g)
            ids[torch.rand(n_id, A, generator=g) < 0.15] = 0
            if n_id > 1:
                ids[1] = 0                                            # every edge of a row masked
            b['ids'] = ids
        elif case.src == 'dense':
            out['x'] = _signed((R, A, D), kx, bits, g)
            ids = torch.randint(1, N + 1, (R, A), generator=g)
            ids[torch.rand(R, A, generator=g) < 0.15] = 0
            live = (ids != 0) & (torch.rand(R, A, generator=g) > 0.1) & (torch.rand(R, 1, generator=g) > 0.2)
            if R > 1:
                live[1] = False
            b['edge_mask'] = live.to(torch.uint8)
            if case.ids or case.sel == 'id':
                b['ids'] = ids
        else:
            out['x'] = _signed((A, D), kx, bits, g)
            if case.ids or case.sel == 'id':
                ids = torch.randint(1, N + 1, (A,), generator=g)
                if case.ids:
                    ids[torch.rand(A, generator=g) < 0.15] = 0
                    ids[0] = ids[-1] = 0
                b['ids'] = ids
        if case.rows and case.src != 'dense':
            rm = torch.rand(R, generator=g) > 0.2
            if R > 2:
                rm[2] = False
            b['row_mask'] = rm.to(torch.uint8)
        ld = {'id': N, 'col': A + 7, 'edge': A + 3}[case.sel]
        sims = torch.randint(0, kw + 1, (R, ld), generator=g).to(torch.float32) / (1 << bits)
        sims[torch.rand(R, ld, generator=g) < 0.1] = 0                # the weight of an anchor inside its own component
        b['sims'] = sims
        if case.sel == 'col':
            b['sim_col'] = torch.randperm(ld, generator=g)[:A]
        wp = _signed((D,), kwp, bits, g)
        wp[0] = kwp / (1 << bits)
        b['wp'] = wp
        b['bp'] = torch.tensor([case.bp], dtype=torch.float32)
        b['gagg'] = _signed((R, D), kg, bits, g)
        b['gz'] = _signed((R, A), kg, bits, g)
        out['bodies'].append(b)
    return out


def leaf_names(case):
    """(name, wants a gradient) of every differentiable input: 'x', then 'wp<k>', 'bp<k>' per body."""
    out = [('x', case.grads[0])]
    for k in range(len(bodies(case))):
        out += [('wp%d' % k, case.grads[1]), ('bp%d' % k, case.grads[2])]
    return out


# ---- the operation ------------------------------------------------------------------------------------------------------------
def _weights(case, b, dtype):
    """(edge (R, A) bool, w (R, A)) of a body."""
    R, A = b['R'], b['A']
    ids, rm = b['ids'], b['row_mask']
    if case.src == 'gather':
        ids = ids.repeat_interleave(case.id_div, 0)[:R] if case.id_div > 1 else ids
        edge = ids != 0
    elif case.src == 'dense':
        edge = b['edge_mask'] != 0
    else:
        edge = (ids != 0).view(1, A).expand(R, A) if (ids is not None and case.ids) else torch.ones(R, A, dtype=torch.bool)
        ids = ids.view(1, A).expand(R, A) if ids is not None else None
    if rm is not None:
        edge = edge & (rm != 0).view(R, 1)
    if case.sel == 'col':
        w = b['sims'][:, b['sim_col']]
    elif case.sel == 'edge':
        w = b['sims'][:, :A]
    else:
        w = torch.gather(b['sims'], 1, (ids - 1).clamp(min=0))
    return edge, w.to(dtype), ids


def _evaluate(case, inp, dtype, reverse=False, gates=None):
    """One forward + backward in ``dtype``.  reverse: the anchors of every row are taken in the opposite order.  gates: the
    (R, A) bool masks that stand in for the relu (``exact`` evaluates the absolute values under the real gates).
    -> ([(agg, z) per body], {leaf: gradient or None}, [gate per body])"""
    want = dict(leaf_names(case))
    leaves = {'x': inp['x'].to(dtype).clone().requires_grad_(want['x'])}
    x = leaves['x']
    outs, made_gates, loss = [], [], None
    for k, b in enumerate(inp['bodies']):
        R, A, D = b['R'], b['A'], case.D
        wp = leaves['wp%d' % k] = b['wp'].to(dtype).clone().requires_grad_(want['wp%d' % k])
        bp = leaves['bp%d' % k] = b['bp'].to(dtype).clone().requires_grad_(want['bp%d' % k])
        edge, w, ids = _weights(case, b, dtype)
        c = w * edge.to(dtype)
        order = torch.arange(A - 1, -1, -1) if reverse else torch.arange(A)
        c_o = c[:, order]
        if case.src == 'shared':
            xo = x[order]
            agg = c_o @ xo
            z_o = c_o * (xo @ wp).view(1, A) + bp
        else:
            if case.src == 'gather':
                rows = x[ids[:, order]]
                if inp['half'] is not None:                            # the fp16 copy's values, the fp32 table's gradient
                    rows = inp['half'].to(dtype)[ids[:, order]] + (rows - rows.detach())
            else:
                rows = x[:, order]
            agg = torch.bmm(c_o.unsqueeze(1), rows).squeeze(1) if A else torch.zeros(R, D, dtype=dtype)
            z_o = c_o * (rows @ wp) + bp
        z = torch.empty_like(z_o)
        z[:, order] = z_o
        if gates is not None:
            gate = gates[k]
            z = z * gate.to(dtype)
        elif case.relu:
            gate = z.detach() > 0
            z = torch.relu(z)
        else:
            gate = torch.ones(R, A, dtype=torch.bool)
        made_gates.append(gate)
        outs.append((agg.detach(), z.detach()))
        for t, go, used in ((agg, b['gagg'], case.outs[0]), (z, b['gz'], case.outs[1])):
            if used and t.requires_grad:
                term = (t * go.to(dtype)).sum()
                loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
    return outs, {n: t.grad for n, t in leaves.items()}, made_gates


@functools.lru_cache(maxsize=None)
def reference(case, dtype=torch.float64, reverse=False):
    """([(agg, z) per body], {leaf name: gradient, None where none arrives}) of loss = sum agg * gagg + sum z * gz over the
    outputs that receive a gradient, evaluated in ``dtype`` on the CPU."""
    outs, grads, _ = _evaluate(case, inputs(case), dtype, reverse)
    return outs, grads


def _abs_inputs(inp):
    out = {'x': inp['x'].abs(), 'half': None if inp['half'] is None else inp['half'].abs(), 'bodies': []}
    for b in inp['bodies']:
        out['bodies'].append({k: (v.abs() if k in ('sims', 'wp', 'bp', 'gagg', 'gz') else v) for k, v in b.items()})
    return out


@functools.lru_cache(maxsize=None)
def exactness(case):
    """{output: largest (sum of the absolute values of an element's terms) * 2^(fraction bits of those terms)}: the
    evaluation of the absolute values of the inputs under the real relu gates (float64).  Below 2^24 every partial sum of
    that output, in any order and with or without fma contraction, is a float32 -- an order-independent condition."""
    inp = inputs(case)
    bits = GRIDS[case.grid][0]
    gates = _evaluate(case, inp, torch.float64)[2]
    outs, grads, _ = _evaluate(case, _abs_inputs(inp), torch.float64, gates=gates)
    top = lambda ts: max([float(t.max()) for t in ts if t is not None and t.numel()] or [0.0])
    frac = {'agg': 2 * bits, 'z': 3 * bits, 'x': 3 * bits, 'wp': 3 * bits, 'bp': bits}
    worst = {'agg': top([o[0] for o in outs]), 'z': top([o[1] for o in outs]), 'x': top([grads['x']]),
             'wp': top([v for n, v in grads.items() if n.startswith('wp')]), 'bp': top([v for n, v in grads.items() if n.startswith('bp')])}
    assert case.bp * (1 << 2 * bits) == int(case.bp * (1 << 2 * bits))
    return {k: worst[k] * (1 << frac[k]) for k in worst}


def exact(case):
    return all(v < (1 << 24) for v in exactness(case).values())

"""Test helpers of the walk aggregator's kernels (subgnn_amd/csrc/lstm.hip: sgnn_lstm_fwd / _bwd, sgnn_rows_gemm,
sgnn_rows_gemm_nt, sgnn_lstm_tail_fwd / _bwd): the seeded calls tests/test_gpu_lstm.py makes, every operation written out in
float64 torch on the CPU, and a restatement of the launch forms of lstm.hip so that tests/test_lstm_cases_host.py can say without
a GPU which kernel form each call reaches.  torch-CPU only; nothing here reads the GPU or imports the package.

The recurrence, per direction d (0 forward, 1 reverse: it walks t = T-1 ... 0), from the projected inputs pre_x (2, B, T, 4H):
    pre = pre_x[d, :, t] + b_hh[d] + h W_hh[d]^T,   (i, f, o) = sigmoid, g = tanh   (gate order i, f, g, o),
    c = f c + i g,   h = o tanh(c);   y[:, t, d H:(d+1) H] = h;   gates, cell and hprev (= h BEFORE the step, 0 at the direction's
    first step) are kept, direction-major (2, B, T, .).   dgates is the gradient of sum(y * dy) with respect to pre_x.

Two kinds of inputs for the GEMMs and the tails:
    float   normal inputs, weights / sqrt(K): compared within helpers.REL_TOL and a norm bound.
    grid    every entry of every operand, biases included, is an integer in [-2, 2] held in float32.  Every product and every
            partial sum of every output is then an integer far below 2^24 (at most 4 * 2 * 512 + 2 for the GEMMs; for the tails
            at most 2 * 5 * 10 = 100 in s, 100 * 2 * 260 + 10 in X), so a float32 evaluation in ANY order equals the float64 one
            bit for bit (tests/test_lstm_cases_host.py shows it for every case) and the device results are compared with
            torch.equal: a wrong lane, row or k-slice of the MFMA layout cannot hide in a tolerance."""
import functools
import math
from collections import namedtuple

import torch

# ---- the constants the launch forms depend on (tests/test_lstm_cases_host.py reads them out of lstm.hip / ops.py and compares) ----
TILE4_FROM = 768                        # lstm_tile: sequences from which a workgroup takes 4 ...
TILE8_FROM = 2048                       # ... and 8 of them; 2 below
HIDDEN = (32, 64, 128)                  # sgnn_lstm_supported
KC = 16                                 # LSTM_KC: k positions per chunk of the GEMM kernels' load loops
KSPLIT_FROM, KSPLIT_MULTIPLE = 128, 32  # sgnn_rows_gemm: K >= 128 && K % 32 == 0 takes the four-wavefront k-split kernel
OWN_GEMM_MAX_H = 64                     # ops.LSTM_OWN_GEMM_MAX_H
TAIL_MAX = 8192                         # the tails' H2 (forward) and D (backward) limit: what their LDS holds
TAIL_STRIDE = 256                       # lanes of a tail workgroup: the stride of its loops over H2 and D
GRID_MAX = 2
PAD_VALUE = 1000.0                      # what the columns K .. ldx of a padded X hold: never an operand


def tile(B):
    """lstm_tile: sequences per workgroup."""
    return 8 if B >= TILE8_FROM else 4 if B >= TILE4_FROM else 2


def own(H, BT):
    """OWN = ceil(BT H / 4 H): (sequence, unit) pairs, i.e. cell states, per owner lane.  The H cancels: 1 at heights 2 (where
    half of the lanes own nothing) and 4, 2 at height 8 -- slot 0 holds sequences 0-3 of the tile, slot 1 sequences 4-7."""
    return (BT * H + 4 * H - 1) // (4 * H)


def gemm_form(K):
    """('single' | 'ksplit', k positions per (wavefront, k-half), whether the last chunk of LSTM_KC positions is partial)."""
    if K >= KSPLIT_FROM and K % KSPLIT_MULTIPLE == 0:
        return 'ksplit', K // 8, (K // 8) % KC != 0
    return 'single', K // 2, (K // 2) % KC != 0


def gemm_nt_form(K):
    """rows_gemm_nt: (k positions per (wavefront, k-half), whether the last chunk is partial)."""
    return K // 4, (K // 4) % KC != 0


# ---- the recurrence ------------------------------------------------------------------------------------------------------------
# bias: 'both' | 'none' (bhh_f and bhh_r null) | 'fwd' (only bhh_r null)
RCase = namedtuple('RCase', 'name B T H bias seed', defaults=('both', 0))
RECURRENCE_SHAPES = ((1, 1), (2, 2), (3, 4), (767, 2), (768, 3), (769, 3), (771, 2), (2047, 2), (2048, 2), (2049, 3), (2053, 3), (5, 20))
BIAS_VARIANT_B = ((3, 4), (769, 3), (2053, 3))                       # one B per tile height
TILE_PAIRS = (2053, 769)                # the launches whose first TILE_SMALL sequences must equal a launch of those alone
TILE_SMALL = 5


def _rcases():
    out = []
    for H in HIDDEN:
        for B, T in RECURRENCE_SHAPES:
            out.append(RCase('rec-%d-%d-%d' % (B, T, H), B, T, H))
        for B, T in BIAS_VARIANT_B:
            for bias in ('none', 'fwd'):
                out.append(RCase('rec-%d-%d-%d-bias-%s' % (B, T, H, bias), B, T, H, bias))
    return tuple(c._replace(seed=i + 1) for i, c in enumerate(out))


RCASES = _rcases()


def rcase(name):
    return next(c for c in RCASES if c.name == name)


@functools.lru_cache(maxsize=4)
def rinputs(case):
    """{'pre_x' (2, B, T, 4H) ~ N(0, 1), 'whh' (2, 4H, H) and 'bhh' [(4H) or None] * 2 uniform in +-1/sqrt(H), 'dy' (B, T, 2H)
    ~ N(0, 1)}, float32, CPU.  Never modified."""
    g = torch.Generator().manual_seed(7000 + case.seed)
    B, T, H = case.B, case.T, case.H
    k = 1.0 / math.sqrt(H)
    pre_x = torch.randn(2, B, T, 4 * H, generator=g)
    whh = (torch.rand(2, 4 * H, H, generator=g) * 2 - 1) * k
    b = (torch.rand(2, 4 * H, generator=g) * 2 - 1) * k
    dy = torch.randn(B, T, 2 * H, generator=g)
    bhh = [None if case.bias == 'none' else b[0], b[1] if case.bias == 'both' else None]
    return {'pre_x': pre_x, 'whh': whh, 'bhh': bhh, 'dy': dy}


def lstm_bwd_ref(whh, gates, cell, dy, dtype=torch.float64):
    """dgates (2, B, T, 4H) from the kept activations AS GIVEN (so that the backward kernel can be fed the float32-rounded
    reference activations and be judged on its own), evaluated in ``dtype``."""
    whh, gates, cell, dy = (t.to(dtype) for t in (whh, gates, cell, dy))
    _, B, T, G = gates.shape
    H = G // 4
    dgates = torch.zeros(2, B, T, G, dtype=dtype)
    for d in (0, 1):
        dh_next = torch.zeros(B, H, dtype=dtype)                     # the recurrent part of dh, from the step after
        dc_next = torch.zeros(B, H, dtype=dtype)
        for step in range(T):                                        # the direction's steps, last first
            t = step if d else T - 1 - step
            first = step == T - 1                                    # the direction's first step: c before it is 0
            i, f, g, o = gates[d, :, t].split(H, dim=1)
            c = cell[d, :, t]
            c_prev = torch.zeros_like(c) if first else cell[d, :, t + 1 if d else t - 1]
            dh = dy[:, t, d * H:(d + 1) * H] + dh_next
            tc = torch.tanh(c)
            dc = dh * o * (1 - tc * tc) + dc_next
            dc_next = dc * f
            dg = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            dgates[d, :, t] = dg
            dh_next = dg @ whh[d]
    return dgates


def lstm_ref(pre_x, whh, bhh, dy=None, dtype=torch.float64):
    """The explicit recurrence in ``dtype`` -> {'y' (B, T, 2H), 'gates' (2, B, T, 4H), 'cell', 'hprev' (2, B, T, H) and, when dy
    is given, 'dgates' (2, B, T, 4H)}.  whh (2, 4H, H); bhh: two (4H) vectors, each of which may be None."""
    pre_x, whh = pre_x.to(dtype), whh.to(dtype)
    _, B, T, G = pre_x.shape
    H = G // 4
    y = torch.zeros(B, T, 2 * H, dtype=dtype)
    gates = torch.zeros(2, B, T, G, dtype=dtype)
    cell, hprev = torch.zeros(2, B, T, H, dtype=dtype), torch.zeros(2, B, T, H, dtype=dtype)
    for d in (0, 1):
        h, c = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype)
        for step in range(T):
            t = T - 1 - step if d else step
            hprev[d, :, t] = h
            pre = pre_x[d, :, t] + h @ whh[d].t()
            if bhh[d] is not None:
                pre = pre + bhh[d].to(dtype)
            i, f, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
            g = torch.tanh(pre[:, 2 * H:3 * H])
            c = f * c + i * g
            h = o * torch.tanh(c)
            gates[d, :, t] = torch.cat([i, f, g, o], 1)
            cell[d, :, t] = c
            y[:, t, d * H:(d + 1) * H] = h
    out = {'y': y, 'gates': gates, 'cell': cell, 'hprev': hprev}
    if dy is not None:
        out['dgates'] = lstm_bwd_ref(whh, gates, cell, dy, dtype)
    return out


@functools.lru_cache(maxsize=4)
def rreference(case):
    inp = rinputs(case)
    return lstm_ref(inp['pre_x'], inp['whh'], inp['bhh'], inp['dy'])


# ---- the row GEMMs -------------------------------------------------------------------------------------------------------------
# op 'gemm': out[z] (R, N) = X[row(r)][:K] W_z^T + b_z, z < dirs; ids: rows gathered from a table of TABLE_ROWS rows; pad: ldx =
# K + pad; copy: x_copy is asked for.   op 'nt': out (R, N) = A[0] W_0 + A[1] W_1, A (2, R, K), W_z (K, N).
GCase = namedtuple('GCase', 'name op kind R K N dirs bias ids pad copy seed', defaults=(2, True, False, 0, False, 0))
TABLE_ROWS = 50


def _g(kind, R, K, N, dirs=2, bias=True, ids=False, pad=0, copy=False):
    name = 'gemm-%s-%d-%d-%d-%dd%s%s%s%s' % (kind, R, K, N, dirs, '' if bias else '-nobias', '-ids' if ids else '',
                                             '-ldx+%d' % pad if pad else '', '-copy' if copy else '')
    return GCase(name, 'gemm', kind, R, K, N, dirs, bias, ids, pad, copy)


def _gcases():
    G, F = 'grid', 'float'
    out = [
        #   kind R   K    N   dirs bias   ids    pad copy
        _g(G, 1, 8, 1, 1, False, False, 0, False),           # the smallest call there is
        _g(G, 31, 8, 31, 2, True, True, 0, True),
        _g(G, 32, 24, 32, 2, True, False, 4, False),
        _g(G, 33, 24, 33, 1, False, True, 4, True),
        _g(G, 65, 40, 40, 2, True, True, 0, True),
        _g(G, 33, 40, 128, 2, True, True, 0, True),          # K = 40: the product's odd input width
        _g(G, 65, 64, 128, 2, True, False, 0, False),        # single wavefront, whole chunks
        _g(G, 31, 64, 32, 1, True, False, 0, True),          # x_copy without ids
        _g(G, 31, 72, 33, 2, False, False, 4, True),
        _g(G, 33, 120, 40, 2, True, True, 0, True),          # the switch, other things equal: single, chunk tail
        _g(G, 33, 128, 40, 2, True, True, 0, True),          # k-split, whole chunks
        _g(G, 33, 136, 40, 2, True, True, 0, True),          # single (136 % 32 != 0), chunk tail
        _g(G, 33, 160, 40, 2, True, True, 0, True),          # k-split, chunk tail
        _g(G, 1, 128, 1, 1, False, False, 4, False),
        _g(G, 32, 160, 31, 1, True, True, 4, True),
        _g(G, 65, 256, 33, 2, False, True, 4, False),        # ids without x_copy
        _g(G, 65, 256, 512, 2, True, False, 0, False),       # the second layer's projection at H = 128
        _g(F, 1, 8, 1, 1, True, False, 0, False),
        _g(F, 65, 24, 33, 2, True, False, 0, True),
        _g(F, 65, 40, 128, 2, True, True, 0, True),
        _g(F, 33, 64, 128, 2, True, True, 0, True),
        _g(F, 32, 72, 32, 1, True, True, 0, False),
        _g(F, 33, 120, 40, 2, True, False, 4, False),
        _g(F, 33, 128, 40, 2, True, False, 4, False),
        _g(F, 33, 136, 33, 2, True, True, 0, True),
        _g(F, 31, 160, 31, 2, False, True, 4, True),
        _g(F, 65, 256, 512, 2, True, False, 0, False),
    ]
    for kind, R, K, N in ((G, 1, 16, 1), (G, 31, 48, 31), (G, 32, 80, 32), (G, 33, 128, 33), (G, 65, 256, 40), (G, 33, 512, 128),
                          (G, 65, 80, 40), (F, 33, 16, 40), (F, 65, 48, 33), (F, 32, 80, 1), (F, 31, 128, 32), (F, 65, 256, 40),
                          (F, 33, 512, 128)):
        out.append(GCase('nt-%s-%d-%d-%d' % (kind, R, K, N), 'nt', kind, R, K, N))
    return tuple(c._replace(seed=i + 1) for i, c in enumerate(out))


GCASES = _gcases()


def _rnd(kind, g):
    if kind == 'grid':
        return lambda *s: torch.randint(-GRID_MAX, GRID_MAX + 1, s, generator=g).to(torch.float32)
    return lambda *s: torch.randn(*s, generator=g)


@functools.lru_cache(maxsize=4)
def ginputs(case):
    """'gemm': {'X' (rows, K + pad) with PAD_VALUE in the columns from K on, 'ids' (R) int64 or None, 'W' [dirs x (N, K)],
    'b' [dirs x (N)] or None}; rows = TABLE_ROWS with ids, R else.  ids name the table's last row first, then row 0, then the last
    row again.   'nt': {'A' (2, R, K), 'W' [2 x (K, N)]}.  float32, CPU.  Never modified."""
    g = torch.Generator().manual_seed(8000 + case.seed)
    rnd = _rnd(case.kind, g)
    R, K, N = case.R, case.K, case.N
    scale = 1.0 if case.kind == 'grid' else 1.0 / math.sqrt(K)
    if case.op == 'nt':
        return {'A': rnd(2, R, K), 'W': [rnd(K, N) * scale for _ in range(2)]}
    rows = TABLE_ROWS if case.ids else R
    X = torch.full((rows, K + case.pad), PAD_VALUE)
    X[:, :K] = rnd(rows, K)
    ids = None
    if case.ids:
        ids = torch.randint(0, rows, (R,), generator=g)
        ids[:3] = torch.tensor([rows - 1, 0, rows - 1])[:R]
    return {'X': X, 'ids': ids, 'W': [rnd(N, K) * scale for _ in range(case.dirs)],
            'b': [rnd(N) for _ in range(case.dirs)] if case.bias else None}


def gathered(case, inp):
    """The (R, K) operand rows of a 'gemm' case: what x_copy must hold, bit for bit."""
    X = inp['X'][:, :case.K]
    return (X if inp['ids'] is None else X[inp['ids']]).contiguous()


def gemm_ref(case, inp, dtype=torch.float64):
    """'gemm' -> (dirs, R, N); 'nt' -> (R, N); in ``dtype``."""
    if case.op == 'nt':
        A = inp['A'].to(dtype)
        return A[0] @ inp['W'][0].to(dtype) + A[1] @ inp['W'][1].to(dtype)
    x = gathered(case, inp).to(dtype)
    outs = []
    for z in range(case.dirs):
        o = x @ inp['W'][z].to(dtype).t()
        outs.append(o if inp['b'] is None else o + inp['b'][z].to(dtype))
    return torch.stack(outs)


# ---- the tails -----------------------------------------------------------------------------------------------------------------
# bias: b_lin given; dW, db: the backward is asked for dW_lin, db_lin
TCase = namedtuple('TCase', 'name kind P n_walks T H2 D last_only bias dW db seed', defaults=(True, True, True, 0))
TAIL_SHAPES = ((1, 1, 1, 2, 1), (5, 3, 4, 64, 64), (7, 5, 10, 256, 128), (3, 2, 3, 260, 300), (4, 2, 2, 10, 3))


def _tcases():
    out = []
    for shape in TAIL_SHAPES:
        for last in (0, 1):
            for kind in ('grid', 'float'):
                out.append(TCase('tail-%s-%s-%s' % (kind, '-'.join(map(str, shape)), 'last' if last else 'sum'), kind, *shape, last))
    for shape, last in ((TAIL_SHAPES[3], 1), (TAIL_SHAPES[4], 0)):
        for what, kw in (('nobias', {'bias': False}), ('nodW', {'dW': False}), ('nodb', {'db': False})):
            out.append(TCase('tail-grid-%s-%s-%s' % ('-'.join(map(str, shape)), 'last' if last else 'sum', what), 'grid', *shape, last)
                       ._replace(**kw))
    return tuple(c._replace(seed=i + 1) for i, c in enumerate(out))


TCASES = _tcases()


@functools.lru_cache(maxsize=4)
def tinputs(case):
    """{'y' (P n_walks, T, H2), 'W' (D, H2), 'b' (D) or None, 'dX' (P, D)}, float32, CPU.  Never modified."""
    g = torch.Generator().manual_seed(9000 + case.seed)
    rnd = _rnd(case.kind, g)
    scale = 1.0 if case.kind == 'grid' else 1.0 / math.sqrt(case.H2)
    y = rnd(case.P * case.n_walks, case.T, case.H2)
    W, b, dX = rnd(case.D, case.H2) * scale, rnd(case.D), rnd(case.P, case.D)
    return {'y': y, 'W': W, 'b': b if case.bias else None, 'dX': dX}


def tail_ref(case, inp, dtype=torch.float64):
    """{'s' (P, H2), 'X' (P, D), 'dy' (P n_walks, T, H2), 'dW' (D, H2), 'db' (D)} in ``dtype`` (dW and db whether or not the
    case asks the kernel for them)."""
    y, W, dX = inp['y'].to(dtype), inp['W'].to(dtype), inp['dX'].to(dtype)
    yw = y.view(case.P, case.n_walks, case.T, case.H2)
    s = yw[:, :, -1].sum(1) if case.last_only else yw.sum((1, 2))
    X = s @ W.t()
    if inp['b'] is not None:
        X = X + case.n_walks * inp['b'].to(dtype)
    g = (dX @ W).repeat_interleave(case.n_walks, dim=0)             # (P n_walks, H2): every walk of a patch receives the patch's row
    dy = torch.zeros_like(y)
    if case.last_only:
        dy[:, -1] = g
    else:
        dy[:] = g.unsqueeze(1)
    return {'s': s, 'X': X, 'dy': dy, 'dW': dX.t() @ s, 'db': case.n_walks * dX.sum(0)}

"""Test helpers of the fused read-out (subgnn_amd/csrc/readout.hip through ``ops.subgraph_embedding``): the seeded calls
tests/test_gpu_readout.py makes, the operation written out in float64 torch on the CPU, and a restatement of the
dispatch predicates of readout.hip / ops._SubgraphEmbedding, so that tests/test_readout_cases_host.py can say without a
GPU which branches those calls reach.  torch-CPU only; nothing here reads the GPU or imports the package.

The operation, per subgraph b and column slot:
    out[b, slot] = sum_c mask[b, c] * relu(W[b, c, a] * s[a] + bp)
W = the similarity columns chosen by ``sim_col`` (the first A columns without one; all zero without similarities),
s = X wp rounded to float32, zero where ids == 0 and for a piece without X; tensor pieces are masked sums; everything is
concatenated in piece order.

The inputs make the relu gates of the kernel and of the reference agree EXACTLY, so that a tolerance has to cover
summation error only: X and wp are integers in [-512, 512] / 256, every product is a multiple of 2^-16 of magnitude <= 4
and every partial sum of <= 1024 of them is exact in double -- the float32 score is the same in any summation order
(``score_orders`` shows it per case).  ``fmaf(w, s, bp) > 0`` in the kernel is then the sign of the exact value of
w * s + bp, and so is the reference's gate: the float32 factors' product has 48 significant bits, exact in double, and a
correctly rounded sum has the sign of the exact one."""
import functools
from collections import namedtuple

import torch

# ---- the constants the dispatch depends on ------------------------------------------------------------------------------------
# (tests/test_readout_cases_host.py reads the #defines out of readout.hip and compares)
ROWS_PER_BLOCK = 64                     # #define RO_ROWS_PER_BLOCK 64: component rows per workgroup of the backward partials
COMP_STEP = 4                           # #define RO_COMP_STEP 4: components per trip of the forward kernels' loop
GS_CHUNK = 1024                         # #define RO_GS_CHUNK 1024: anchors of d s staged in LDS at a time (d wp)
THREADS = 256                           # #define RO_THREADS 256: d wp: 256 / D anchor ranges, or columns d, d + 256, ...
MAX_SLOTS = 96                          # #define RO_MAX_SLOTS 96: tensor pieces per launch of masked_sum_slots_*
MAX_PIECES = 8                          # #define RO_MAX_PIECES 8: in-kernel read-out pieces per launch group
MAX_D = 1024                            # ro_fill_pieces: ``if (D < 1 || D > 1024) return -1``
FINISH_LANES, FINISH_LOADS = 64, 4      # the finish kernels: a lane adds every 64th block partial, four loads in flight
SLOTS_TOGETHER_BELOW = 1 << 22          # ops.SLOTS_TOGETHER_BELOW (the host test compares)

BRANCHES = ('comp_loop_trips>1', 'comp_loop_ragged', 'nblk>256', 'dwp_first', 'dwp_second_q1', 'dwp_second_q2',
            'dwp_second_q3', 'dwp_second_q4', 'anchor_chunks>1', 'vec4_slot', 'scalar_slot', 'slots_launches>1',
            'null_grad_slot', 'pad_ids', 'no_X_piece', 'groups>1')

# ---- the pieces of a call ------------------------------------------------------------------------------------------------------
# Tensor: a (B, C, w) tensor piece.  InKernel: a read-out piece whose scores X wp are made inside the launches (D None: no
# X, all scores zero, no similarities); col 'perm': sim_col is a permutation into a row 7 wider, 'ld': no sim_col, the row is
# 3 wider than A; grad: which of (X, wp, bp) want a gradient.  Scores: the s-given form; grad: which of (s, bp).
Tensor = namedtuple('Tensor', 'w grad', defaults=(True,))
InKernel = namedtuple('InKernel', 'A D ids col grad', defaults=(False, 'perm', (True, True, True)))
Scores = namedtuple('Scores', 'A col grad', defaults=('perm', (True, True)))
Case = namedtuple('Case', 'name B C pieces together_below dead_block seed', defaults=(None, False, 0))


def _variants(base, which):
    out = []
    for tag, grad in which:
        pieces = tuple(p._replace(grad=grad) if isinstance(p, InKernel) and p.D is not None else p for p in base.pieces)
        out.append(base._replace(name='%s-%s' % (base.name, tag), pieces=pieces))
    return out


_D48 = Case('three-trips-D48', 33, 9, (Tensor(5), InKernel(1025, 48, ids=True), InKernel(64, 48, col='ld'), InKernel(4, None)), seed=3)

CASES = [
    # (B, C) = (7, 5): a ragged second trip of the component loop; D = 8: first d wp form, 32 anchor ranges re-split in 2 chunks
    Case('ragged-trip-D8', 7, 5, (Tensor(3), InKernel(1025, 8, ids=True), InKernel(3, None), InKernel(4, 8, col='ld')), seed=1),
    # two full trips; D = 128: first form with nq = 2, three chunks of anchors
    Case('two-trips-D128', 13, 8, (InKernel(2100, 128, ids=True), InKernel(1, 128, col='ld'), InKernel(5, None), Tensor(5)), seed=2),
    # three trips, R = 297 = 4 blocks of 64 rows + 41; D = 48: second form, one column per thread, two chunks
    _D48,
    # exactly one full block; D = 300: second form, two columns per thread, three chunks
    Case('one-block-D300', 64, 1, (InKernel(2100, 300, ids=True), Tensor(2), InKernel(65, 300, col='ld')), seed=4),
    # D = 1024: the widest the library takes, four columns per thread
    Case('two-trips-D1024', 13, 8, (InKernel(65, 1024, ids=True), InKernel(3, 1024, col='ld'), InKernel(3, None)), seed=5),
    # D = 600: three columns per thread, the third for threads 0..87 only
    Case('ragged-trip-D600', 7, 5, (InKernel(64, 600, ids=True), InKernel(5, 600, col='ld'), Tensor(4)), seed=13),
    # D = 256 divides 256 but exceeds 128: second form; A = 1024 is exactly one chunk
    Case('three-trips-D256', 33, 9, (InKernel(1024, 256), InKernel(5, 256, ids=True, col='ld'), Tensor(1)), seed=6),
    # nine pieces of one width (two launches: 8 + 2 with the piece without X); D = 1: first form, 256 ranges
    Case('nine-pieces-D1', 7, 5, tuple(InKernel(A, 1, ids=(i % 2 == 1), col=('ld' if i % 3 == 0 else 'perm'))
                                       for i, A in enumerate((1, 3, 4, 5, 64, 65, 1024, 5, 3))) + (InKernel(4, None),), seed=7),
    # R = 16800 = 262 blocks + 32 rows: 263 block partials -- every lane of the finish takes one four-load iteration, lanes
    # 0..6 a tail iteration as well; one block of 64 rows wholly dead
    Case('many-rows-D64', 4200, 4, (InKernel(5, 64, ids=True, col='ld'), Tensor(2), InKernel(70, 64), InKernel(3, None)),
         dead_block=True, seed=8),
    # the s-given form (ReadoutPiece turns the scores into anchors X = s of width 1 with wp = 1; one launch group of three
    # per case): gradient of bp only, of s only, of both
    Case('scores-three-trips', 33, 9, (Scores(65, grad=(False, True)), Tensor(3), Scores(5, 'ld', (True, False)), Scores(64)), seed=9),
    Case('scores-many-rows', 4200, 4, (Scores(5), Scores(3, 'ld', (False, True)), Scores(4, 'perm', (True, False))),
         dead_block=True, seed=10),
    # one vectorised launch per tensor piece: widths, slot offsets and H multiples of 4 (and two pieces that are not)
    Case('vec4-slots', 13, 8, (Tensor(8), InKernel(4, 8), Tensor(64), InKernel(8, 8, ids=True), Tensor(6), Tensor(2)),
         together_below=0, seed=11),
    # its twin: one width changed, H odd -- every piece takes the scalar form
    Case('vec4-slots-odd-H', 13, 8, (Tensor(8), InKernel(4, 8), Tensor(63), InKernel(8, 8, ids=True), Tensor(6), Tensor(2)),
         together_below=0, seed=11),
    # 100 tensor pieces in the launches that take RO_MAX_SLOTS: two each way; three pieces want no gradient
    Case('many-slots', 5, 3, tuple(Tensor(1 + i % 3, grad=i not in (5, 50, 99)) for i in range(50)) + (InKernel(4, 8),)
         + tuple(Tensor(1 + i % 3, grad=i not in (5, 50, 99)) for i in range(50, 100)), together_below=1 << 30, seed=12),
] + _variants(_D48, (('X-only', (True, False, False)), ('wp-only', (False, True, False)), ('bp-only', (False, False, True))))


def widths(case):
    return [p.w if isinstance(p, Tensor) else p.A for p in case.pieces]


# ---- the dispatch of readout.hip and of ops._SubgraphEmbedding, restated -------------------------------------------------------
def row_blocks(case):
    """ro_blocks: ``(R + RO_ROWS_PER_BLOCK - 1) / RO_ROWS_PER_BLOCK``."""
    return (case.B * case.C + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK


def launch_groups(case):
    """ops._readout_groups: the read-out pieces by anchor width (those without X ride with the smallest; given scores are
    anchors of width 1), each width in launches of RO_MAX_PIECES -> the group sizes."""
    many = [p for p in case.pieces if not isinstance(p, Tensor)]
    if not many:
        return []
    by_d = {}
    for p in many:
        d = 1 if isinstance(p, Scores) else p.D
        by_d[d] = by_d.get(d, 0) + 1
    free = by_d.pop(None, 0)
    ds = sorted(by_d) or [1]
    by_d[ds[0]] = by_d.get(ds[0], 0) + free
    return [min(MAX_PIECES, by_d[d] - lo) for d in ds for lo in range(0, by_d[d], MAX_PIECES)]


def slots_together(case):
    """_SubgraphEmbedding.forward: ``together = n_x >= 2 and B * C * H <= SLOTS_TOGETHER_BELOW``."""
    below = SLOTS_TOGETHER_BELOW if case.together_below is None else case.together_below
    n_x = sum(isinstance(p, Tensor) for p in case.pieces)
    return n_x >= 2 and case.B * case.C * sum(widths(case)) <= below


def branches(case):
    """The names in BRANCHES that one forward + backward of the case reaches."""
    got = set()
    ws, H = widths(case), sum(widths(case))
    readouts = [p for p in case.pieces if not isinstance(p, Tensor)]
    if readouts:
        if case.C > COMP_STEP:                                        # for (c0 = 0; c0 < C; c0 += RO_COMP_STEP): a second trip
            got.add('comp_loop_trips>1')
        if case.C % COMP_STEP:                                        # c0 + u < C fails inside the last trip
            got.add('comp_loop_ragged')
    if any(any(p.grad) for p in readouts) and row_blocks(case) > FINISH_LANES * FINISH_LOADS:
        got.add('nblk>256')                                           # for (; k + 192 < nblk; k += 256) taken by every lane
    for p in readouts:
        if not isinstance(p, InKernel):
            continue
        if p.D is None:
            got.add('no_X_piece')                                     # if (X && ...) in readout_scores_kernel; P.gX / P.gwp null
            continue
        if p.ids:
            got.add('pad_ids')                                        # ids && ids[a] == 0
        if p.grad[1]:                                                 # if (P.gwp[p] && P.X[p] && P.gs[p])
            if p.D <= THREADS // 2 and THREADS % p.D == 0:            # if (D <= RO_THREADS / 2 && RO_THREADS % D == 0)
                got.add('dwp_first')
            else:                                                     # columns d, d + RO_THREADS, ... of a thread
                got.add('dwp_second_q%d' % ((p.D + THREADS - 1) // THREADS))
            if p.A > GS_CHUNK:                                        # for (a0 = 0; a0 < A; a0 += RO_GS_CHUNK)
                got.add('anchor_chunks>1')
    if len(launch_groups(case)) > 1:
        got.add('groups>1')
    together = slots_together(case)
    n_x = sum(isinstance(p, Tensor) for p in case.pieces)
    if together:
        if n_x > MAX_SLOTS:                                           # for (from = 0; from < n_pieces; from += RO_MAX_SLOTS)
            got.add('slots_launches>1')
        wanted = sum(p.grad for p in case.pieces if isinstance(p, Tensor))
        if 0 < wanted < n_x:
            # a piece whose gradient nobody wants: ops leaves it out of the backward launch's list.  (The kernel's own
            # ``if (gx)`` for a null pointer INSIDE the list is reached by a direct library call in test_gpu_readout.py.)
            got.add('null_grad_slot')
    else:
        off = 0
        for p, w in zip(case.pieces, ws):
            if isinstance(p, Tensor):
                # ro_vec4_ok: W % 4 == 0 && ld % 4 == 0 && both pointers 16-byte aligned (the slot's: its offset, in floats)
                got.add('vec4_slot' if w % 4 == 0 and H % 4 == 0 and off % 4 == 0 else 'scalar_slot')
            off += w
    return got


# ---- inputs and reference ------------------------------------------------------------------------------------------------------
def _grid(shape, g):
    return torch.randint(-512, 513, shape, generator=g).to(torch.float32) / 256


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The float32 CPU inputs of a case: {'mask' (B, C) bool, 'go' (B, H), 'pieces': one dict per piece}.  Never modified."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    B, C = case.B, case.C
    R = B * C
    mask = torch.rand(B, C, generator=g) > 0.3
    mask[B // 2] = False                                              # a subgraph without a live component
    if case.dead_block:
        assert R > 6 * ROWS_PER_BLOCK
        mask.view(-1)[5 * ROWS_PER_BLOCK:6 * ROWS_PER_BLOCK] = False  # a block of the backward partials without a live row
    pieces = []
    for i, p in enumerate(case.pieces):
        if isinstance(p, Tensor):
            pieces.append({'x': torch.randn(B, C, p.w, generator=g)})
            continue
        d = {'bp': (torch.rand(1, generator=g) * 0.2 + 0.2) * (1 if i % 2 else -1), 'sims': None, 'col': None, 'ids': None}
        if not (isinstance(p, InKernel) and p.D is None):
            ld = p.A + (7 if p.col == 'perm' else 3)
            d['sims'] = torch.rand(R, ld, generator=g)
            if p.col == 'perm':
                d['col'] = torch.randperm(ld, generator=g)[:p.A]
        if isinstance(p, Scores):
            d['s'] = torch.randn(p.A, generator=g)
        elif p.D is not None:
            d['X'], d['wp'] = _grid((p.A, p.D), g), _grid((p.D,), g)
            if p.ids:
                ids = torch.randint(1, 9, (p.A,), generator=g) * (torch.rand(p.A, generator=g) > 0.25)
                ids[1:4] = 2
                ids[0] = ids[-1] = 0                                  # PAD at both ends of the anchors
                d['ids'] = ids
        if not gates(p, d).expand(R, p.A)[mask.reshape(-1)].any():                   # no live gate: nothing would depend on this piece
            d['bp'] = -d['bp']
        pieces.append(d)
    return {'mask': mask, 'go': torch.randn(B, sum(widths(case)), generator=g), 'pieces': pieces}


def scores32(p, d):
    """The float32 scores of a read-out piece: given, all zero without X, or X wp rounded once."""
    if isinstance(p, Scores):
        return d['s']
    return torch.zeros(p.A) if p.D is None else exact_scores(d)


def similarity_columns(p, d, R):
    """W (R, A) float32: the columns ``sim_col`` picks, the first A without one, zeros without similarities."""
    if d['sims'] is None:
        return torch.zeros(R, p.A)
    return d['sims'][:, d['col']] if d['col'] is not None else d['sims'][:, :p.A]


def gates(p, d):
    """(R, A) bool: w * s + bp > 0, exactly -- the float32 factors' product and the sum's sign are exact in double."""
    R = d['sims'].shape[0] if d['sims'] is not None else 1
    return similarity_columns(p, d, R).double() * scores32(p, d).double() + d['bp'].double() > 0


def leaf_names(case):
    """(name, wants a gradient) of every differentiable input, in piece order: 'p<i>.x' | 'p<i>.X', '.wp', '.bp' | '.s', '.bp'."""
    out = []
    for i, p in enumerate(case.pieces):
        if isinstance(p, Tensor):
            out.append(('p%d.x' % i, p.grad))
        elif isinstance(p, Scores):
            out += [('p%d.s' % i, p.grad[0]), ('p%d.bp' % i, p.grad[1])]
        elif p.D is None:
            out.append(('p%d.bp' % i, p.grad[2]))
        else:
            out += [('p%d.X' % i, p.grad[0]), ('p%d.wp' % i, p.grad[1]), ('p%d.bp' % i, p.grad[2])]
    return out


def exact_scores(d):
    """s = X wp of an in-kernel piece with anchors: exact in double, rounded once to float32, zero where ids == 0."""
    s = (d['X'].double() @ d['wp'].double()).float()
    return s * (d['ids'] != 0).float() if d['ids'] is not None else s


def score_orders(d):
    """The scores of a piece summed in three orders in double (the library's, a permuted sequential one, a reversed
    sequential one) -> three (A,) float64 tensors; equal bits are the gate-exactness condition."""
    X, wp = d['X'].double(), d['wp'].double()
    perm = torch.randperm(X.shape[1], generator=torch.Generator().manual_seed(X.shape[1]))
    seq = lambda idx: (X[:, idx] * wp[idx]).cumsum(1)[:, -1]
    return X @ wp, seq(perm), seq(torch.arange(X.shape[1] - 1, -1, -1))


@functools.lru_cache(maxsize=None)
def reference(case, dtype=torch.float64):
    """(out (B, H), {leaf name: gradient, None where none is wanted}) of loss = (out * go).sum(), evaluated in ``dtype`` on
    the CPU.  The score is the exactly rounded float32 value in either dtype (its gradient passes through the rounding as
    the identity) and the gate is the sign of the exact w * s + bp: what is left to ``dtype`` is every sum."""
    inp = inputs(case)
    B, C = case.B, case.C
    m = inp['mask'].to(dtype).view(B, C, 1)
    leaves, cols = {}, []
    want = dict(leaf_names(case))

    def leaf(name, t):
        leaves[name] = t.to(dtype).clone().requires_grad_(want[name])
        return leaves[name]
    for i, (p, d) in enumerate(zip(case.pieces, inp['pieces'])):
        if isinstance(p, Tensor):
            cols.append(leaf('p%d.x' % i, d['x']))
            continue
        s32 = scores32(p, d)
        if isinstance(p, Scores):
            s = leaf('p%d.s' % i, d['s'])
        elif p.D is None:
            s = s32.to(dtype)
        else:
            X, wp = leaf('p%d.X' % i, d['X']), leaf('p%d.wp' % i, d['wp'])
            lin = X @ wp
            if d['ids'] is not None:
                lin = lin * (d['ids'] != 0).to(dtype)
            s = (lin - lin.detach()) + s32.to(dtype)                  # the value of s32, the gradient of X wp
        bp = leaf('p%d.bp' % i, d['bp'])
        W = similarity_columns(p, d, B * C)
        gate = gates(p, d).expand(B * C, p.A)
        cols.append(((W.to(dtype) * s + bp) * gate.to(dtype)).view(B, C, p.A))
    out = (torch.cat(cols, dim=-1) * m).sum(1)
    if any(t.requires_grad for t in leaves.values()):
        (out * inp['go'].to(dtype)).sum().backward()
    return out.detach(), {k: t.grad for k, t in leaves.items()}

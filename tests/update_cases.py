"""Test helpers of the update layer (subgnn_amd/csrc/update.hip through ``ops.update_layer`` / ``ops.update_layers``): the
seeded calls tests/test_gpu_update.py makes, the operation written out in float64 torch on the CPU, and a restatement of the
launch forms of update.hip / ops.py so that tests/test_update_cases_host.py can say without a GPU which kernel form each call
reaches.  torch-CPU only; nothing here reads the GPU or imports the package.

The operation, per body:  out = relu([x | sum_k aggr_k] W^T + b),  loss = sum over the bodies that receive a gradient of
(out * grad_out).sum(),  gradients for exactly the leaves the case asks for (a chunked aggregate's gradient is (chunks, R, D)).

Two kinds of inputs:
    float   randn, W / sqrt(2 D) (tests/test_gpu_float.py's): compared within helpers.REL_TOL and a norm bound.
    grid    every entry of x, the aggregate chunks, W, b and grad_out is an integer in [-2, 2] held in float32.  Every product
            and every partial sum of every output is then an integer below 2^24 (the forward at most 4 D (1 + chunks), dx at
            most 4 D, dW at most 4 R chunks), so a float32 evaluation in ANY order equals the float64 one bit for bit
            (tests/test_update_cases_host.py shows it for every case) and the device results are compared with torch.equal.
            About half of the outputs are exactly 0; ``inputs`` takes the first seed at which at least one PRE-activation is
            exactly 0 too (the relu mask's edge: its gradient is 0) and at least one output is positive."""
import functools
import math
from collections import namedtuple

import torch

# ---- the constants the launch forms depend on (tests/test_update_cases_host.py reads them out of update.hip and compares) ----
KSPLIT_BELOW = 4096                     # UPD_KSPLIT_BELOW: rows below which a tile's contraction is split over four wavefronts
SPLIT_BELOW = 16384                     # UPD_SPLIT_BELOW: rows below which the output tiles go to separate wavefronts
WAVE_ROWS = 64                          # UPD_WAVE_ROWS: rows per wavefront of the weight-gradient kernel ...
WAVE_ROWS_SMALL = 16                    # UPD_WAVE_ROWS_SMALL: ... and for calls below UPD_KSPLIT_BELOW rows
MAX_BODIES = 8                          # UPD_MAX_BODIES: bodies per sgnn_update_fwd_many / sgnn_update_bwd_many launch
DIMS = (32, 64, 128)
GRID_MAX = 2                            # grid inputs: integers in [-GRID_MAX, GRID_MAX]
DEAD_BIAS = -2000.0                     # the all-dead layer: below every pre-activation's bias-free part (|.| <= 4 * 2 D = 1024)

ALL, NONE = (True, True, True, True), (False, False, False, False)

# chunks: 0 = aggr is (R, D); k >= 1 = aggr is (k, R, D).  grads: which of (x, aggr, W, b) require a gradient.  go: whether the
# body's output receives a gradient.  bias: 'rand' | None (no bias) | 'dead' (DEAD_BIAS, but column 0 has b = 0 and a zero row
# of W: a pre-activation of exactly 0 in every row) | 'half0' (0 in the even columns).
Body = namedtuple('Body', 'chunks grads go bias', defaults=(0, ALL, True, 'rand'))
# kind 'float' | 'grid'; via 'layer' (ops.update_layer, one body) | 'layers' (ops.update_layers); zero_row: one row of x and of
# every aggregate chunk is all 0 (with bias 'half0' its pre-activation is exactly 0 in half the columns).
Case = namedtuple('Case', 'name kind R D bodies via zero_row seed', defaults=((Body(),), 'layer', False, 0))

ROW_EDGES_64 = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 193, 255, 256, 257, 4095, 4096, 4097, 4351, 4352,
                16383, 16384, 16385, 16415)
ROW_EDGES_OTHER = (1, 33, 65, 4095, 4096, 16383, 16384, 16385)
CHUNK_COUNTS = (1, 2, 3, 70)
CHUNK_ROWS = (1, 33, 96, 4095)
BODY_ROWS = (1, 33, 4095)
GRAD_SHAPES = ((33, 64), (4097, 64), (16385, 64))


def _cases():
    out = []
    # ---- row edges: one body, one chunk, all gradients, both kinds ----
    for D in DIMS:
        for R in (ROW_EDGES_64 if D == 64 else ROW_EDGES_OTHER):
            for kind in ('float', 'grid'):
                out.append(Case('rows-%s-%d-%d' % (kind, R, D), kind, R, D))
    # ---- chunks: one body ----
    for D in DIMS:
        for R in CHUNK_ROWS:
            for k in CHUNK_COUNTS:
                out.append(Case('chunks-%d-%d-%d' % (k, R, D), 'grid', R, D, (Body(chunks=k),)))
    out.append(Case('chunks-3-4096-64-torch-sum', 'grid', 4096, 64, (Body(chunks=3),)))       # ops adds the chunks in torch
    out.append(Case('chunks-3-96-64-float', 'float', 96, 64, (Body(chunks=3),)))
    out.append(Case('chunks-70-33-128-float', 'float', 33, 128, (Body(chunks=70),)))
    # ---- bodies ----
    for D in DIMS:
        for R in BODY_ROWS:
            for n in (2, 8, 9):
                out.append(Case('bodies-%d-%d-%d' % (n, R, D), 'grid', R, D, (Body(),) * n, 'layers'))
            out.append(Case('bodies-chunks-1-3-70-%d-%d' % (R, D), 'grid', R, D, (Body(chunks=1), Body(chunks=3), Body(chunks=70)), 'layers'))
            out.append(Case('bodies-no-gradient-for-1-%d-%d' % (R, D), 'grid', R, D, (Body(chunks=2), Body(go=False), Body()), 'layers'))
            out.append(Case('bodies-split-gradients-%d-%d' % (R, D), 'grid', R, D,
                            (Body(grads=(False, True, False, False)), Body(chunks=2, grads=(False, False, True, True))), 'layers'))
    out.append(Case('bodies-3-4096-64-one-by-one', 'grid', 4096, 64, (Body(), Body(chunks=3), Body()), 'layers'))
    out.append(Case('bodies-3-33-64-float', 'float', 33, 64, (Body(), Body(chunks=3), Body()), 'layers'))
    # ---- gradient subsets ----
    for R, D in GRAD_SHAPES:
        for m in range(16):
            grads = tuple(bool(m >> i & 1) for i in range(4))
            out.append(Case('grads-%s-%d-%d' % (''.join(n for n, w in zip('xaWb', grads) if w) or 'none', R, D), 'grid', R, D,
                            (Body(grads=grads),)))
    # ---- edges of the values ----
    for R in (33, 4097):
        for kind in ('float', 'grid'):
            out.append(Case('no-bias-%s-%d-64' % (kind, R), kind, R, 64, (Body(bias=None),)))
    out.append(Case('no-rows-64', 'float', 0, 64))
    for R in (33, 4097, 16385):                                      # (one per forward kernel)
        out.append(Case('all-dead-%d-64' % R, 'grid', R, 64, (Body(bias='dead'),)))
        out.append(Case('zero-row-%d-64' % R, 'grid', R, 64, (Body(bias='half0'),), zero_row=True))
    return tuple(c._replace(seed=i + 1) for i, c in enumerate(out))


CASES = _cases()


def dead(case):
    return any(b.bias == 'dead' for b in case.bodies)


def n_chunks(body):
    return max(1, body.chunks)


# ---- the launch forms of update.hip and ops.py, restated --------------------------------------------------------------------------
def partial_blocks(R):
    """Row blocks of the weight-gradient kernel (sgnn_update_bwd_workspace_bytes, upd_block_rows)."""
    rows = 4 * (WAVE_ROWS_SMALL if R < KSPLIT_BELOW else WAVE_ROWS)
    return (R + rows - 1) // rows


def workspace_bytes(R, D):
    return partial_blocks(R) * (D * 2 * D + D) * 4 + 64


def forms(case):
    """{'fwd': 'ksplit' | 'split' | 'wide' | None, 'dx': 'split' | 'wide' | None, 'dw': 'small' | 'large' | None,
    'blocks': partial blocks of dW, 'many': launches of sgnn_update_fwd_many (= of sgnn_update_bwd_many when a gradient
    arrives), 'chunk_adding': the kernel adds a body's chunks while loading, 'torch_sum': ops adds them}."""
    R = case.R
    f = {'fwd': None, 'dx': None, 'dw': None, 'blocks': 0, 'many': 0, 'chunk_adding': False, 'torch_sum': False}
    if R == 0:
        return f
    f['fwd'] = 'ksplit' if R < KSPLIT_BELOW else 'split' if R < SPLIT_BELOW else 'wide'
    back = [b for b in case.bodies if b.go and any(b.grads)]
    many = case.via == 'layers' and len(case.bodies) >= 2 and R < KSPLIT_BELOW and all(b.bias is not None for b in case.bodies)
    if many:
        f['many'] = (len(case.bodies) + MAX_BODIES - 1) // MAX_BODIES
    if any(b.grads[0] or b.grads[1] for b in back):
        f['dx'] = 'split' if R < SPLIT_BELOW else 'wide'
    if any(b.grads[2] or b.grads[3] for b in back) or (many and back):     # (the _many backward always makes grad_W and grad_b)
        f['dw'] = 'small' if R < KSPLIT_BELOW else 'large'
        f['blocks'] = partial_blocks(R)
    f['chunk_adding'] = any(b.chunks > 1 for b in case.bodies) and R < KSPLIT_BELOW
    f['torch_sum'] = any(b.chunks > 1 for b in case.bodies) and R >= KSPLIT_BELOW
    return f


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _draw(case, seed):
    g = torch.Generator().manual_seed(seed)
    R, D = case.R, case.D
    if case.kind == 'grid':
        rnd = lambda *s: torch.randint(-GRID_MAX, GRID_MAX + 1, s, generator=g).to(torch.float32)
        w_scale = 1.0
    else:
        rnd = lambda *s: torch.randn(*s, generator=g)
        w_scale = 1.0 / math.sqrt(2 * D)
    zero = R // 2
    bodies = []
    for body in case.bodies:
        x = rnd(R, D)
        aggr = rnd(body.chunks, R, D) if body.chunks else rnd(R, D)
        W = rnd(D, 2 * D) * w_scale
        b = rnd(D)
        go = rnd(R, D)
        if case.zero_row:
            x[zero] = 0
            aggr[..., zero, :] = 0
        if body.bias == 'half0':
            b[0::2] = 0
        elif body.bias == 'dead':
            b[:] = DEAD_BIAS
            b[0] = 0
            W[0] = 0
        elif body.bias is None:
            b = None
        bodies.append({'x': x, 'aggr': aggr, 'W': W, 'b': b, 'go': go if body.go else None})
    return {'bodies': bodies, 'zero_row': zero if case.zero_row else None}


def pre_activation(b, dtype=torch.float64):
    a = b['aggr'].to(dtype)
    a = a.sum(0) if a.dim() == 3 else a
    pre = torch.cat([b['x'].to(dtype), a], 1) @ b['W'].to(dtype).t()
    return pre if b['b'] is None else pre + b['b'].to(dtype)


@functools.lru_cache(maxsize=2)
def inputs(case):
    """The float32 CPU inputs of a case: {'bodies': [{'x', 'aggr' (R, D) or (chunks, R, D), 'W', 'b' or None, 'go' or None}],
    'zero_row'}.  Never modified.  grid: the first of the seeds 1000 seed, 1000 seed + 1, ... at which every body holds a
    pre-activation that is exactly 0 and (unless the layer is dead) a positive one."""
    for t in range(1000):
        inp = _draw(case, 1000 * case.seed + t)
        if case.kind != 'grid' or case.R == 0:
            return inp
        pres = [pre_activation(b) for b in inp['bodies']]
        if all((p == 0).any() and ((p > 0).any() or dead(case)) for p in pres):
            return inp
    raise ValueError('%s: no seed gives a pre-activation of exactly 0' % case.name)


# ---- the operation ------------------------------------------------------------------------------------------------------------
def evaluate(case, inp, dtype):
    """One forward + backward in ``dtype`` on the CPU -> [{'out', 'x', 'aggr', 'W', 'b': gradient or None} per body]."""
    res, loss, leaves = [], None, []
    for body, b in zip(case.bodies, inp['bodies']):
        lv = {n: (None if b[n] is None else b[n].to(dtype).clone().requires_grad_(w))
              for n, w in zip(('x', 'aggr', 'W', 'b'), body.grads)}
        a = lv['aggr'].sum(0) if lv['aggr'].dim() == 3 else lv['aggr']
        pre = torch.cat([lv['x'], a], 1) @ lv['W'].t()
        out = torch.relu(pre if lv['b'] is None else pre + lv['b'])
        leaves.append(lv)
        res.append({'out': out.detach()})
        if b['go'] is not None and out.requires_grad:
            term = (out * b['go'].to(dtype)).sum()
            loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
    for r, lv in zip(res, leaves):
        for n, t in lv.items():
            r[n] = None if t is None else t.grad
    return res


@functools.lru_cache(maxsize=2)
def reference(case):
    """``evaluate`` in float64."""
    return evaluate(case, inputs(case), torch.float64)

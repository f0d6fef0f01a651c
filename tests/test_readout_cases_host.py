"""Without a GPU: the calls of tests/test_gpu_readout.py reach every branch of the fused read-out that readout_cases.branches
names, its constants are the kernel's, its inputs make the relu gates exact, and the tolerances of the GPU test are
reachable by a correct float32 evaluation of the same operation."""
import os
import re

import pytest
import torch

import readout_cases as RC
from helpers import assert_close

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
_ids = lambda c: c.name


def test_cases_reach_every_branch():
    reached = {}
    for c in RC.CASES:
        for b in RC.branches(c):
            assert b in RC.BRANCHES, b
            reached.setdefault(b, []).append(c.name)
    assert set(reached) == set(RC.BRANCHES), 'not reached: %s' % sorted(set(RC.BRANCHES) - set(reached))


def test_cases_hold_what_the_kernels_branch_on():
    """The sizes and pairings the cases were chosen for, stated once more so that an edit of CASES cannot drop one silently."""
    shapes = {(c.B, c.C) for c in RC.CASES}
    assert {(7, 5), (13, 8), (33, 9), (64, 1), (4200, 4)} <= shapes
    pairs = {(p.D, p.A) for c in RC.CASES for p in c.pieces if isinstance(p, RC.InKernel)}
    assert {(8, 1025), (128, 2100), (48, 1025), (300, 2100), (1024, 65)} <= pairs
    assert {d for d, _ in pairs} >= {1, 8, 128, 48, 256, 300, 1024, None}
    assert {a for _, a in pairs} >= {1, 3, 4, 5, 64, 65, 1024, 1025, 2100}
    big = [c for c in RC.CASES if (c.B, c.C) == (4200, 4)]
    assert any({(64, 5), (64, 70)} <= {(p.D, p.A) for p in c.pieces if isinstance(p, RC.InKernel)} for c in big)
    for c in RC.CASES:
        widths = {p.D for p in c.pieces if isinstance(p, RC.InKernel)} - {None}
        assert len(widths) <= 1, c.name                                # one anchor width per call
        assert sum(t.numel() for d in RC.inputs(c)['pieces'] for t in d.values() if t is not None) * 4 < 8 << 20, c.name
    assert any(len(RC.launch_groups(c)) > 1 and sum(RC.launch_groups(c)) >= 9 for c in RC.CASES)
    # the s-given form at both row counts, with each choice of gradients
    for shape in ((33, 9), (4200, 4)):
        grads = {p.grad for c in RC.CASES if (c.B, c.C) == shape for p in c.pieces if isinstance(p, RC.Scores)}
        assert grads >= {(True, False), (False, True), (True, True)}
    # given scores travel as anchors of width 1: the three pieces of each such case share one launch group
    assert all(RC.launch_groups(c) == [3] for c in RC.CASES if c.name in ('scores-three-trips', 'scores-many-rows'))
    grads = {p.grad for c in RC.CASES for p in c.pieces if isinstance(p, RC.InKernel) and p.D is not None}
    assert grads >= {(True, False, False), (False, True, False), (False, False, True), (True, True, True)}
    many = next(c for c in RC.CASES if c.name == 'many-slots')
    assert sum(isinstance(p, RC.Tensor) for p in many.pieces) == 100 and (many.B, many.C) == (5, 3)
    assert sum(isinstance(p, RC.Tensor) and p.grad for p in many.pieces) > RC.MAX_SLOTS     # two launches backward too
    # the masks: a subgraph without a live component everywhere, a dead block of rows where the finish has > 256 partials
    for c in RC.CASES:
        m = RC.inputs(c)['mask']
        assert not m[c.B // 2].any() and m.any(), c.name
        if RC.row_blocks(c) > 256:
            blocks = m.reshape(-1)[:c.B * c.C // RC.ROWS_PER_BLOCK * RC.ROWS_PER_BLOCK].view(-1, RC.ROWS_PER_BLOCK)
            assert (~blocks.any(1)).any(), c.name


def test_constants_are_the_kernels():
    src = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'readout.hip')).read()
    defines = {k: int(v) for k, v in re.findall(r'^#define (RO_\w+) (\d+)\b', src, re.M)}
    mine = {'RO_ROWS_PER_BLOCK': RC.ROWS_PER_BLOCK, 'RO_COMP_STEP': RC.COMP_STEP, 'RO_GS_CHUNK': RC.GS_CHUNK,
            'RO_THREADS': RC.THREADS, 'RO_MAX_SLOTS': RC.MAX_SLOTS, 'RO_MAX_PIECES': RC.MAX_PIECES}
    assert {k: defines.get(k) for k in mine} == mine
    # the conditions that are not #defines, as the kernel writes them
    assert 'if (D < 1 || D > %d) return -1;' % RC.MAX_D in src
    assert 'if (D <= RO_THREADS / 2 && RO_THREADS % D == 0)' in src
    assert src.count('for (; k + %d < nblk; k += %d)' % (RC.FINISH_LANES * (RC.FINISH_LOADS - 1), RC.FINISH_LANES * RC.FINISH_LOADS)) == 2
    from subgnn_amd import ops
    assert ops.SLOTS_TOGETHER_BELOW == RC.SLOTS_TOGETHER_BELOW


@pytest.mark.parametrize('case', RC.CASES, ids=_ids)
def test_scores_do_not_depend_on_the_summation_order(case):
    """The gate-exactness condition: every partial sum of a score is exact in double, so any order gives the same float64
    sum and the same float32 rounding -- the kernel's fma chain in double included."""
    for p, d in zip(case.pieces, RC.inputs(case)['pieces']):
        if not isinstance(p, RC.InKernel) or p.D is None:
            continue
        assert p.D <= RC.MAX_D
        for t in (d['X'], d['wp']):
            assert t.abs().max() <= 2 and torch.equal(t * 256, (t * 256).round())
        a, b, c = RC.score_orders(d)
        assert torch.equal(a, b) and torch.equal(a, c)
        assert torch.equal(a.float(), b.float()) and torch.equal(a.float(), c.float())
        s = RC.exact_scores(d)
        if d['ids'] is not None:
            assert s[0] == 0 and s[-1] == 0 and d['ids'][0] == 0 and d['ids'][-1] == 0


@pytest.mark.parametrize('case', RC.CASES, ids=_ids)
def test_float32_evaluation_meets_the_gpu_tolerances(case):
    """reference() in float32 torch-CPU against reference() in float64 at the tolerances of tests/test_gpu_readout.py: they
    are reachable by a correct float32 evaluation whose sums run in other orders than the kernels'."""
    out64, g64 = RC.reference(case)
    out32, g32 = RC.reference(case, torch.float32)
    assert out32.dtype == torch.float32
    assert_close(out32, out64, case.name + ' embedding', norm_tol=1e-6)
    for (name, wanted) in RC.leaf_names(case):
        assert (g64[name] is not None) == wanted and (g32[name] is not None) == wanted, name
        if wanted:
            assert g64[name].abs().max() > 0, 'the gradient of %s is all zero: nothing could be wrong with it' % name
            assert_close(g32[name], g64[name], '%s gradient of %s' % (case.name, name), norm_tol=1e-5)

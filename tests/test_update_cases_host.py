"""Without a GPU: the calls of tests/test_gpu_update.py reach every launch form of the update layer on both sides of every
threshold, the thresholds update_cases.forms restates are the ones in update.hip and the library's own queries, the grid inputs
make every result independent of the order of every sum (the float32 CPU evaluation equals the float64 one bit for bit) and
hold the relu's edge, and the float inputs meet the GPU test's tolerances when the same operation is evaluated in float32."""
import os
import re

import pytest
import torch

import update_cases as UC
from helpers import REL_TOL, assert_close, norm_err, rel_err

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
OUT_NORM_TOL, GRAD_NORM_TOL = 1e-5, 2e-5         # the bounds of tests/test_gpu_float.py::test_update_layer_matches_torch
_ids = lambda c: c.name
GRID = [c for c in UC.CASES if c.kind == 'grid']
FLOAT = [c for c in UC.CASES if c.kind == 'float']


def test_case_names_are_unique():
    names = [c.name for c in UC.CASES]
    assert len(set(names)) == len(names)


def test_constants_are_the_sources():
    src = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'update.hip')).read()
    defines = {k: int(v) for k, v in re.findall(r'^#define (UPD_\w+) (\d+)\b', src, re.M)}
    mine = {'UPD_KSPLIT_BELOW': UC.KSPLIT_BELOW, 'UPD_SPLIT_BELOW': UC.SPLIT_BELOW, 'UPD_WAVE_ROWS': UC.WAVE_ROWS,
            'UPD_WAVE_ROWS_SMALL': UC.WAVE_ROWS_SMALL, 'UPD_MAX_BODIES': UC.MAX_BODIES}
    assert {k: defines.get(k) for k in mine} == mine
    # the conditions as the source writes them
    for line, count in (('if (R < UPD_KSPLIT_BELOW) hipLaunchKernelGGL((update_fwd_ksplit_kernel<DD>)', 1),
                        ('const bool split = R < UPD_SPLIT_BELOW;', 2),                     # forward and dx
                        ('return 4 * (R < UPD_KSPLIT_BELOW ? UPD_WAVE_ROWS_SMALL : UPD_WAVE_ROWS);', 1),
                        ('if (R >= UPD_KSPLIT_BELOW) return SGNN_ERR_BAD_ARG;', 2),         # both _many entries
                        ('(n_chunks > 1 && R >= UPD_KSPLIT_BELOW)', 1),
                        ('const int64_t per = (n_blocks + 3) / 4;', 1)):
        assert src.count(line) == count, line
    from subgnn_amd import ops
    assert tuple(ops.UPDATE_DIMS) == UC.DIMS


def test_library_queries_agree():
    from subgnn_amd import _lib
    lib = _lib.load()
    assert lib.sgnn_update_fwd_chunks_max_rows() == UC.KSPLIT_BELOW - 1
    assert lib.sgnn_update_many_max_bodies() == UC.MAX_BODIES
    for R, D in sorted({(c.R, c.D) for c in UC.CASES}):
        assert lib.sgnn_update_bwd_workspace_bytes(R, D) == UC.workspace_bytes(R, D), (R, D)


def test_cases_reach_every_form_on_both_sides_of_every_threshold():
    for D in UC.DIMS:
        here = [c for c in UC.CASES if c.D == D]
        fs = [UC.forms(c) for c in here]
        assert {f['fwd'] for f in fs} >= {'ksplit', 'split', 'wide'}, D
        assert {f['dx'] for f in fs} >= {'split', 'wide'}, D
        assert {f['dw'] for f in fs} >= {'small', 'large'}, D
        rows = {c.R for c in here if c.via == 'layer' and c.bodies == (UC.Body(),)}
        assert rows >= {UC.KSPLIT_BELOW - 1, UC.KSPLIT_BELOW, UC.SPLIT_BELOW - 1, UC.SPLIT_BELOW, UC.SPLIT_BELOW + 1}, D
        assert {c.kind for c in here if c.R in (UC.KSPLIT_BELOW - 1, UC.KSPLIT_BELOW, UC.SPLIT_BELOW - 1, UC.SPLIT_BELOW)
                and c.name.startswith('rows-')} == {'float', 'grid'}
        # chunk adding in the kernel at every chunk count, a 3-D aggregate of one chunk, the bodies' launches
        assert {c.bodies[0].chunks for c in here if len(c.bodies) == 1 and UC.forms(c)['chunk_adding']} >= {2, 3, 70}
        assert any(c.bodies[0].chunks == 1 for c in here if len(c.bodies) == 1)
        assert {UC.forms(c)['many'] for c in here if c.via == 'layers'} >= {1, 2}
        assert {len(c.bodies) for c in here if c.via == 'layers'} >= {2, 3, 8, 9}
        assert any(not b.go for c in here for b in c.bodies)
    blocks = {UC.forms(c)['blocks'] for c in UC.CASES if c.D == 64}
    assert blocks >= {1, 2, 3, 4, 5, 16, 17, 64, 65}
    small = {UC.forms(c)['blocks'] for c in UC.CASES if c.D == 64 and UC.forms(c)['dw'] == 'small'}
    assert small >= {1, 2, 3, 4, 5} and {UC.partial_blocks(R) for R in (64, 65, 129, 193, 257)} == {1, 2, 3, 4, 5}
    assert [UC.partial_blocks(R) for R in (4096, 4097, 16384, 16385)] == [16, 17, 64, 65]
    # ops' fall-backs: the chunks added in torch, a list that runs one body after the other
    assert any(UC.forms(c)['torch_sum'] and c.via == 'layer' for c in UC.CASES)
    assert any(c.via == 'layers' and len(c.bodies) >= 2 and UC.forms(c)['many'] == 0 and c.R >= UC.KSPLIT_BELOW for c in UC.CASES)
    # all 16 gradient subsets at one shape per forward kernel
    for R, D in UC.GRAD_SHAPES:
        assert len({c.bodies[0].grads for c in UC.CASES if (c.R, c.D) == (R, D) and c.name.startswith('grads-')}) == 16
    assert {UC.forms(c)['fwd'] for c in UC.CASES if c.name.startswith('grads-')} == {'ksplit', 'split', 'wide'}
    # the edges of the values
    assert {c.R for c in UC.CASES if c.bodies[0].bias is None} >= {33, 4097}
    assert any(c.R == 0 for c in UC.CASES) and any(UC.dead(c) for c in UC.CASES) and any(c.zero_row for c in UC.CASES)
    assert max(c.R for c in UC.CASES) == 16415 and {c.D for c in UC.CASES} == set(UC.DIMS)         # nothing larger: the tests stay quick


def _bits_equal(a32, a64, what):
    assert (a32 is None) == (a64 is None), what
    if a32 is not None:
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and a32.shape == a64.shape, what
        assert torch.equal(a32.double(), a64), what


@pytest.mark.parametrize('case', GRID, ids=_ids)
def test_grid_float32_equals_float64_and_holds_the_relu_edge(case):
    inp = UC.inputs(case)
    ref = UC.reference(case)
    got = UC.evaluate(case, inp, torch.float32)
    for k, (body, b, r32, r64) in enumerate(zip(case.bodies, inp['bodies'], got, ref)):
        for t in (b['x'], b['aggr'], b['W'], b['b'], b['go']):
            if t is not None and not UC.dead(case):
                assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= UC.GRID_MAX
        for name in ('out', 'x', 'aggr', 'W', 'b'):
            _bits_equal(r32[name], r64[name], '%s %s of body %d' % (case.name, name, k))
        pre = UC.pre_activation(b)
        assert (pre == 0).any(), 'no pre-activation is exactly 0'
        if UC.dead(case):
            assert float(r64['out'].abs().max()) == 0.0
            assert all(float(r64[n].abs().max()) == 0.0 for n in ('x', 'aggr', 'W', 'b'))
        else:
            assert (r64['out'] > 0).any()
            zeros = float((r64['out'] == 0).double().mean())
            assert 0.3 < zeros < 0.7 or case.R * case.D < 2048, zeros
        # a gradient arrives exactly where it is asked for and the body's output is used
        wanted = dict(zip(('x', 'aggr', 'W', 'b'), body.grads))
        for name in ('x', 'aggr', 'W', 'b'):
            assert (r64[name] is not None) == (wanted[name] and body.go and b[name] is not None), name
        if body.chunks and r64['aggr'] is not None:
            assert r64['aggr'].shape == (body.chunks, case.R, case.D)
            assert all(torch.equal(r64['aggr'][0], r64['aggr'][j]) for j in range(1, body.chunks))
    if case.zero_row:
        z = inp['zero_row']
        b = inp['bodies'][0]
        pre = UC.pre_activation(b)
        assert (pre[z, 0::2] == 0).all() and (b['go'][z, 0::2] != 0).any() and (pre[z, 1::2] > 0).any()
        # torch's gradient at a pre-activation of exactly 0 is 0: the row's gradient comes from its odd columns alone
        want = (b['go'][z].double() * (pre[z] > 0)) @ b['W'].double()
        assert torch.equal(torch.cat([ref[0]['x'][z], ref[0]['aggr'][z]]), want)


@pytest.mark.parametrize('case', FLOAT, ids=_ids)
def test_float32_evaluation_meets_the_gpu_tolerances(case):
    """The bounds tests/test_gpu_update.py asserts are the ones a plain float32 evaluation of the same operation keeps."""
    ref = UC.reference(case)
    got = UC.evaluate(case, UC.inputs(case), torch.float32)
    worst = [0.0, 0.0]
    for k, (r32, r64) in enumerate(zip(got, ref)):
        for name in ('out', 'x', 'aggr', 'W', 'b'):
            assert (r32[name] is None) == (r64[name] is None)
            if r64[name] is None:
                continue
            assert_close(r32[name], r64[name], '%s %s of body %d' % (case.name, name, k), tol=REL_TOL,
                         norm_tol=OUT_NORM_TOL if name == 'out' else GRAD_NORM_TOL)
            worst = [max(worst[0], rel_err(r32[name], r64[name])), max(worst[1], norm_err(r32[name], r64[name]))]
    print('%s: element-wise %.2e, norm %.2e' % (case.name, *worst))


@pytest.mark.parametrize('name', ['rows-float-257-64', 'no-bias-float-33-64'])
def test_reference_is_linear_and_relu(name):
    case = next(c for c in UC.CASES if c.name == name)
    b = UC.inputs(case)['bodies'][0]
    D = case.D
    lin = torch.nn.Linear(2 * D, D, bias=b['b'] is not None).double()
    with torch.no_grad():
        lin.weight.copy_(b['W'])
        if b['b'] is not None:
            lin.bias.copy_(b['b'])
    x, a = b['x'].double().requires_grad_(True), b['aggr'].double().requires_grad_(True)
    out = torch.relu(lin(torch.cat([x, a], 1)))
    (out * b['go'].double()).sum().backward()
    ref = UC.reference(case)[0]
    assert torch.allclose(out.detach(), ref['out'], rtol=0, atol=1e-13)
    for got, want in ((x.grad, ref['x']), (a.grad, ref['aggr']), (lin.weight.grad, ref['W'])):
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
    if b['b'] is not None:
        assert torch.allclose(lin.bias.grad, ref['b'], rtol=0, atol=1e-12)

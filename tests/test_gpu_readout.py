"""-m gpu: the fused read-out (subgnn_amd/csrc/readout.hip through ops.subgraph_embedding) against the float64 CPU
reference of tests/readout_cases.py, at the anchor widths, anchor counts, component counts and row counts its kernels
branch on (tests/test_readout_cases_host.py shows on the CPU which branch each case reaches, and that the tolerances
used here are met by a float32 evaluation of the same operation).  Tolerances: helpers.REL_TOL element-wise, and
max|a - b| / max|b| below 1e-6 for values and 1e-5 for gradients, as in test_gpu_float.py."""
import numpy as np
import pytest
import torch

import readout_cases as RC
from helpers import assert_close, norm_err, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ops():
    from subgnn_amd import ops
    return ops


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(ops, case):
    """One forward + backward of the case on the device -> (out, {leaf name: gradient or None})."""
    inp = RC.inputs(case)
    B, C = case.B, case.C
    R = B * C
    mask = inp['mask'].reshape(-1).to(torch.uint8).to(DEV)
    want = dict(RC.leaf_names(case))
    leaves, pieces = {}, []

    def leaf(name, t):
        leaves[name] = t.to(DEV).clone().requires_grad_(want[name])
        return leaves[name]
    for i, (p, d) in enumerate(zip(case.pieces, inp['pieces'])):
        if isinstance(p, RC.Tensor):
            pieces.append(leaf('p%d.x' % i, d['x']))
        elif isinstance(p, RC.Scores):
            s, bp = leaf('p%d.s' % i, d['s']), leaf('p%d.bp' % i, d['bp'])
            pieces.append(ops.ReadoutPiece(_dev(d['sims']), _dev(d['col']), s, bp, p.A, mask, R))
        elif p.D is None:
            pieces.append(ops.ReadoutPiece(None, None, None, leaf('p%d.bp' % i, d['bp']), p.A, mask, R))
        else:
            X, wp, bp = leaf('p%d.X' % i, d['X']), leaf('p%d.wp' % i, d['wp']), leaf('p%d.bp' % i, d['bp'])
            pieces.append(ops.ReadoutPiece(_dev(d['sims']), _dev(d['col']), None, bp, p.A, mask, R, X=X, wp=wp, ids=_dev(d['ids'])))
    out = ops.subgraph_embedding(pieces, mask, B, C)
    if out.requires_grad:
        (out * inp['go'].to(DEV)).sum().backward()
    return out.detach(), {k: t.grad for k, t in leaves.items()}


@pytest.mark.parametrize('case', RC.CASES, ids=lambda c: c.name)
def test_subgraph_embedding_matches_float64_reference(case, monkeypatch):
    """The embedding and every requested gradient against readout_cases.reference (float64, CPU); gradients nobody asked
    for are None; a second run gives the same bits; no ticket of the finish launch is left non-zero; the call makes
    the launch groups readout_cases.launch_groups says it makes."""
    ops = _ops()
    if case.together_below is not None:
        monkeypatch.setattr(ops, 'SLOTS_TOGETHER_BELOW', case.together_below)
    groups, plain = [], ops._readout_groups

    def counted(many, tensors):
        got = plain(many, tensors)
        groups.append([len(g) for g in got])
        return got
    monkeypatch.setattr(ops, '_readout_groups', counted)
    ref_out, ref_g = RC.reference(case)
    out, grads = _run(ops, case)
    assert groups == [RC.launch_groups(case)]
    assert not ops._readout_tickets(torch.device(DEV)).any(), 'a ticket of readout_bwd_finish_many_kernel was left non-zero'
    out2, grads2 = _run(ops, case)
    assert not ops._readout_tickets(torch.device(DEV)).any()
    print('%s embedding: element-wise %.3e, norm %.3e' % (case.name, rel_err(out, ref_out), norm_err(out, ref_out)))
    assert_close(out, ref_out.float(), case.name + ' embedding', norm_tol=1e-6)
    assert torch.equal(out, out2), 'the embedding differs between two runs'
    for name, wanted in RC.leaf_names(case):
        if not wanted:
            assert grads[name] is None and ref_g[name] is None, name
            continue
        assert grads[name] is not None, 'no gradient of ' + name
        print('%s gradient of %s: element-wise %.3e, norm %.3e' % (case.name, name, rel_err(grads[name], ref_g[name]),
                                                                    norm_err(grads[name], ref_g[name])))
        assert_close(grads[name], ref_g[name].float(), '%s gradient of %s' % (case.name, name), norm_tol=1e-5)
        assert torch.equal(grads[name], grads2[name]), 'the gradient of %s differs between two runs' % name


def test_anchor_width_above_the_maximum_is_refused(monkeypatch):
    """D = 1025: sgnn_readout_many_fwd returns SGNN_ERR_BAD_ARG before its first launch (ro_fill_pieces) and _lib.check
    raises SubgnnHipError; the score buffer it would have written keeps its bytes."""
    ops = _ops()
    from subgnn_amd._lib import SubgnnHipError
    B, C, A, D = 3, 2, 5, RC.MAX_D + 1
    g = torch.Generator().manual_seed(0)
    mask = torch.ones(B * C, dtype=torch.uint8, device=DEV)
    sims = torch.rand(B * C, A, generator=g).to(DEV)
    X = torch.randn(A, D, generator=g).to(DEV).requires_grad_(True)
    wp = torch.randn(D, generator=g).to(DEV).requires_grad_(True)
    bp = torch.zeros(1, device=DEV, requires_grad=True)
    made, plain = [], torch.empty

    def empty_filled(*a, **k):                                # the buffers the call allocates, poisoned: nothing may write them
        t = plain(*a, **k)
        if t.is_cuda and t.dtype == torch.float32:
            made.append(t.fill_(-7.0))
        return t
    with monkeypatch.context() as mp:
        mp.setattr(torch, 'empty', empty_filled)
        with pytest.raises(SubgnnHipError, match='sgnn_readout_many_fwd failed: SGNN_ERR_BAD_ARG'):
            ops.subgraph_embedding([ops.ReadoutPiece(sims, None, None, bp, A, mask, B * C, X=X, wp=wp)], mask, B, C)
    torch.cuda.synchronize()
    assert sorted(t.numel() for t in made) == [A, B * A] and all((t == -7.0).all() for t in made)     # the scores, the embedding
    assert not ops._readout_tickets(torch.device(DEV)).any()
    # the widest width that is taken, right after: the refusal left nothing behind
    piece = ops.ReadoutPiece(sims, None, None, bp, A, mask, B * C, X=X[:, :RC.MAX_D].contiguous(), wp=wp[:RC.MAX_D].contiguous())
    out = ops.subgraph_embedding([piece], mask, B, C)
    s = (X[:, :RC.MAX_D].double() @ wp[:RC.MAX_D].double()).float()
    ref = torch.relu(sims.view(B, C, A).double() * s.double() + bp.double()).sum(1)
    assert_close(out, ref.float(), 'D = 1024 after the refusal', norm_tol=1e-6)


def test_slots_backward_skips_a_null_gradient_pointer():
    """masked_sum_slots_bwd_kernel's ``if (gx)``: a piece listed with a null gradient pointer is skipped, its neighbours
    are written.  ops leaves such a piece out of the list, so the library is called directly."""
    ops = _ops()
    from subgnn_amd import _lib
    lib = _lib.load()
    B, C, ws = 9, 3, (3, 2, 5, 1)
    H = sum(ws) + 2
    g = torch.Generator().manual_seed(4)
    mask = (torch.rand(B * C, generator=g) > 0.3).to(torch.uint8).to(DEV)
    go = torch.randn(B, H, generator=g).to(DEV)
    offs = np.array([1, 4, 6, 11], dtype=np.int64)                     # (the pieces need not tile the row)
    grads = [torch.full((B, C, w), -7.0, device=DEV) if i != 1 else None for i, w in enumerate(ws)]
    ptrs = ops._ptr_table(grads)
    assert ptrs[1] == 0
    widths = np.array(ws, dtype=np.int64)
    _lib.check(lib.sgnn_masked_sum_slots_bwd(ops._ptr(go), H, ops._ptr(mask), B, C, ptrs.ctypes.data, widths.ctypes.data,
                                             offs.ctypes.data, len(ws), ops._stream()), 'sgnn_masked_sum_slots_bwd')
    torch.cuda.synchronize()
    m = mask.view(B, C, 1).float()
    for i, w in enumerate(ws):
        if grads[i] is not None:
            want = go[:, int(offs[i]):int(offs[i]) + w].view(B, 1, w) * m
            assert torch.equal(grads[i], want.expand(B, C, w)), i

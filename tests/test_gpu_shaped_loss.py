"""-m gpu: label smoothing and focal loss -- the shaped launches of the fused head (csrc/head.hip: heads_fwd_kernel<ML, SH>,
heads_bwd_kernel<NB, ML, SH>), the shaped stand-alone pairs (csrc/loss.hip) and the model path that uses them
(hparams['label_smoothing'] / ['focal_gamma'], SubGNN.training_step) against loss_weights.ShapedLoss in float64 on the CPU.
Tolerances are those of tests/test_gpu_weighted_loss.py for the same kernels: logits assert_close's default, loss
1e-5 max(1, |ref|), gradients assert_close(norm_tol=2e-5)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close
import shaped_loss_cases as C
import weighted_loss_cases as WC
from test_gpu_weighted_loss import Guarded, SENTINEL, SMALL, ROUTES, _raw_inputs, _model, _step_gradients, write_datasets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ops():
    from subgnn_amd import ops
    return ops


def _dev(t):
    return None if t is None else t.to(DEV)


def _loss_close(got, ref):
    assert abs(float(got) - ref) <= 1e-5 * max(1.0, abs(ref)), (float(got), ref)


def _mods(shape):
    B, H0, H1, H2, K = shape
    return [m.to(DEV) for m in WC.head_modules(H0, H1, H2, K, 3)]


def _head(mode, x, mods, case, y=None, w='case', pw='case'):
    ops = _ops()
    name, ml, eps, gamma = mode
    y = _dev(case['y'] if y is None else y)
    w = _dev(case['w']) if isinstance(w, str) else w
    pw = _dev(case['pw']) if isinstance(pw, str) else pw
    if ml:
        return ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.0, None, targets=y, class_weight=w, pos_weight=pw, focal_gamma=gamma)
    return ops.fused_head(x, mods[0], mods[1], mods[2], y, 0.0, None, class_weight=w, label_smoothing=eps, focal_gamma=gamma)


@pytest.mark.parametrize('case', C.all_head_cases(), ids=C.case_id)
def test_shaped_head_matches_shaped_loss(case):
    """ops.fused_head(label_smoothing= / focal_gamma=) == the head + ShapedLoss of float64 torch: values, every gradient (through
    the loss, and through loss + logits), the accuracy, the call twice bit-identical; -100 rows, a zero class weight and the
    constructed rows (lead / trail by 40 and 100) are part of every case that has the rows for them; a label of K gives NaN."""
    shape, mode = case
    name, ml, eps, gamma = mode
    B, H0, H1, H2, K = shape
    c = C.head_case(shape, mode)
    mods = _mods(shape)
    params = [p for m in mods for p in (m.weight, m.bias)]
    xg = c['x'].to(DEV).requires_grad_(True)
    lg, loss, acc = _head(mode, xg, mods, c)
    loss.backward()
    ref = c['ref']
    assert_close(lg.detach(), ref['logits'], 'logits')
    print('%s: loss %.9g ref %.9g' % (C.case_id(case), float(loss.detach()), ref['loss']))
    assert bool(torch.isfinite(loss.detach()))
    _loss_close(loss.detach(), ref['loss'])
    y = c['y'].to(DEV)
    if ml:
        hits = int(((torch.sigmoid(lg.detach()) > 0.5) == (y != 0)).all(1).sum())
    else:
        hits = int(((lg.detach().argmax(1) == y) & (y >= 0)).sum())
    assert acc.shape == (1,) and float(acc) == float(torch.tensor(float(hits), dtype=torch.float32) / B)     # unweighted, unchanged
    for got, want, nm in zip([xg.grad] + [p.grad for p in params], ref['grads'], C.GRAD_NAMES):
        assert bool(torch.isfinite(got).all()), nm
        assert_close(got, want, 'grad ' + nm, norm_tol=2e-5)
    lg3, loss3, acc3 = _head(mode, c['x'].to(DEV), mods, c)
    assert torch.equal(lg3, lg.detach()) and torch.equal(loss3, loss.detach()) and torch.equal(acc3, acc)
    for p in params:
        p.grad = None
    xg2 = c['x'].to(DEV).requires_grad_(True)
    lg2, loss2, _ = _head(mode, xg2, mods, c)
    (loss2 + (lg2 * c['go'].to(DEV)).sum()).backward()
    for got, want, nm in zip([xg2.grad] + [p.grad for p in params], c['ref2']['grads'], C.GRAD_NAMES):
        assert_close(got, want, 'grad %s through loss + logits' % nm, norm_tol=2e-5)
    if not ml:
        bad = c['y'].clone()
        bad[B // 2] = K
        assert torch.isnan(_head(mode, c['x'].to(DEV), mods, c, y=bad)[1])


def _pair(mode, x, c, w='case', pw='case'):
    ops = _ops()
    name, ml, eps, gamma = mode
    w = _dev(c['w']) if isinstance(w, str) else w
    pw = _dev(c['pw']) if isinstance(pw, str) else pw
    if ml:
        return ops.bce_with_logits_and_accuracy(x, c['y'].to(DEV), weight=w, pos_weight=pw, focal_gamma=gamma)
    return ops.cross_entropy_with_accuracy(x, c['y'].to(DEV), weight=w, label_smoothing=eps, focal_gamma=gamma)


@pytest.mark.parametrize('case', C.all_pair_cases(), ids=C.case_id)
def test_shaped_pair_matches_shaped_loss(case):
    shape, mode = case
    name, ml, eps, gamma = mode
    B, K = shape
    c = C.pair_case(shape, mode)
    xg = c['x'].to(DEV).requires_grad_(True)
    loss, acc = _pair(mode, xg, c)
    (loss * 1.5).backward()
    print('%s: loss %.9g ref %.9g' % (C.case_id(case), float(loss.detach()), c['loss']))
    assert bool(torch.isfinite(loss.detach())) and bool(torch.isfinite(xg.grad).all())
    _loss_close(loss.detach(), c['loss'])
    y = c['y'].to(DEV)
    hits = int(((torch.sigmoid(xg.detach()) > 0.5) == (y != 0)).all(1).sum()) if ml else int(((xg.detach().argmax(1) == y) & (y >= 0)).sum())
    assert round(float(acc) * B) == hits
    assert_close(xg.grad, c['grad'], 'grad logits', norm_tol=2e-5)
    if gamma and c['extreme']:
        # the closed form at the constructed rows: a target that leads by 40 or 100 has q = 0 in float32 -- its gradient is exactly
        # 0 (single-label: the whole row); one that trails has q = 1 and a finite gradient
        rows = xg.grad[c['extreme']]
        if ml:
            lead = torch.tensor(C.LEADS, device=DEV).view(4, 1) * torch.where(y[c['extreme']] != 0, 1.0, -1.0)
            assert bool((rows[lead >= 100] == 0).all()) and bool((rows[lead <= -40] != 0).sum() > 0)
        else:
            assert bool((rows[0] == 0).all()) and bool((rows[2] == 0).all()) and bool((rows[1] != 0).any()) and bool((rows[3] != 0).any())
    loss2, acc2 = _pair(mode, c['x'].to(DEV), c)
    assert torch.equal(loss2, loss.detach()) and torch.equal(acc2, acc)
    if not ml:
        ops = _ops()
        bad = c['y'].clone()
        bad[B // 2] = K
        assert torch.isnan(ops.cross_entropy_with_accuracy(c['x'].to(DEV), bad.to(DEV), weight=_dev(c['w']), label_smoothing=eps,
                                                           focal_gamma=gamma)[0])


# ---- raw entries: guarded buffers -----------------------------------------------------------------------------------------------------

def _raw_head(shape, z1, mods, labels, mode, w=None, pw=None, p=0.0, rng=None, g_loss=1.0, expect=0):
    """sgnn_head_fwd[_ml]_shaped + sgnn_head_bwd[_ml]_shaped on guarded buffers -> dict of Guarded."""
    from subgnn_amd import _lib
    ops = _ops()
    lib = _lib.load()
    name, ml, eps, gamma = mode
    B, H0, H1, H2, K = shape
    b = {'a1': Guarded(B * H1), 'a2': Guarded(B * H2), 'logits': Guarded(B * K), 'lse': Guarded(B + 1), 'out': Guarded(3),
         'dz1': Guarded(B * H1), 'w': None if w is None else Guarded(K, fill=w), 'pw': None if pw is None else Guarded(K, fill=pw)}
    ws = ops._head_workspace(torch.device(DEV), B)
    st = ops._stream()
    P, nb = int(lib.sgnn_head_partial_floats(H1, H2, K)), int(lib.sgnn_head_blocks(B))
    b['partial'] = Guarded(nb * P)
    W2, b2, W3, b3 = (t.detach().contiguous() for t in (mods[1].weight, mods[1].bias, mods[2].weight, mods[2].bias))
    wp = None if w is None else b['w'].ptr
    pwp = None if pw is None else b['pw'].ptr
    head = (ops._ptr(z1), B, H1, H2, K, ops._ptr(W2), ops._ptr(b2), ops._ptr(W3), ops._ptr(b3), ops._ptr(labels), float(p), ops._ptr(rng),
            b['a1'].ptr, b['a2'].ptr, b['logits'].ptr)
    g = torch.tensor([g_loss], dtype=torch.float32, device=DEV)
    rows = ctypes.c_void_p(b['out'].t.data_ptr() + 8)
    tail = (ops._ptr(g), None, rows, b['a1'].ptr, b['a2'].ptr, ops._ptr(W2), ops._ptr(W3), B, H1, H2, K, float(p), b['dz1'].ptr,
            b['partial'].ptr, st)
    if ml:
        rc = lib.sgnn_head_fwd_ml_shaped(*head, b['out'].ptr, ops._ptr(ws), ws.numel() * 4, st, wp, pwp, gamma)
        assert rc == expect, rc
        rc = lib.sgnn_head_bwd_ml_shaped(b['logits'].ptr, ops._ptr(labels), *tail, wp, pwp, gamma)
    else:
        rc = lib.sgnn_head_fwd_shaped(*head, b['lse'].ptr, b['out'].ptr, ops._ptr(ws), ws.numel() * 4, st, wp, eps, gamma)
        assert rc == expect, rc
        rc = lib.sgnn_head_bwd_shaped(b['logits'].ptr, b['lse'].ptr, ops._ptr(labels), *tail, wp, eps, gamma)
    assert rc == expect, rc
    torch.cuda.synchronize()
    return {k: v for k, v in b.items() if v is not None}


def _labels(mode, B, K, g):
    return (torch.rand(B, K, generator=g) < 0.4).long().to(DEV) if mode[1] else WC.labels_for(B, K, g).to(DEV)


@pytest.mark.parametrize('mode', C.MODES, ids=lambda m: m[0])
def test_guard_words_ones_rows_and_refused_calls(mode):
    """The raw shaped entries on guarded buffers (three chunks, the last short): every guard word around logits, lse, grad (dz1),
    the activations, the partials and the weight rows intact; rows of ones give the bits of absent rows; a refused call (a value
    outside its domain, both set) returns SGNN_ERR_BAD_ARG and writes nothing."""
    name, ml, eps, gamma = mode
    B, H0, H1, H2, K = SMALL
    g, mods, z1 = _raw_inputs(SMALL)
    y = _labels(mode, B, K, g)
    w = WC.class_weights(K, g)
    pw = WC.class_weights(K, g, zero=False) if ml else None
    got = _raw_head(SMALL, z1, mods, y, mode, w=w, pw=pw)
    for nm, buf in got.items():
        assert buf.intact(), nm
    assert torch.equal(got['w'].t.cpu(), w) and bool(torch.isfinite(got['out'].t).all()) and bool(torch.isfinite(got['dz1'].t).all())
    absent = _raw_head(SMALL, z1, mods, y, mode)
    ones = _raw_head(SMALL, z1, mods, y, mode, w=torch.ones(K), pw=torch.ones(K) if ml else None)
    for nm in ('a1', 'a2', 'logits', 'out', 'dz1', 'partial') + (() if ml else ('lse',)):
        assert torch.equal(absent[nm].t, ones[nm].t), nm
        assert absent[nm].intact() and ones[nm].intact(), nm
    assert not torch.equal(absent['out'].t[:1], got['out'].t[:1])                 # ... and the weights were applied
    refused = [(name, ml, 0.0, -1.0), (name, ml, 0.0, float('inf')), (name, ml, 0.0, float('nan'))]
    if not ml:
        refused += [(name, ml, 1.0, 0.0), (name, ml, -0.25, 0.0), (name, ml, 0.1, 2.0)]
    for bad in refused:
        b = _raw_head(SMALL, z1, mods, y, bad, w=w, pw=pw, expect=-1)
        for nm in ('a1', 'a2', 'logits', 'lse', 'out', 'dz1', 'partial'):
            assert bool((b[nm].buf == SENTINEL).all()), (bad, nm)


@pytest.mark.parametrize('mode', C.MODES, ids=lambda m: m[0])
def test_pairs_guard_words_ones_rows_and_refused_calls(mode):
    """The raw stand-alone entries at (257, 40): two workgroups forward, K above the head's limit."""
    from subgnn_amd import _lib
    ops = _ops()
    lib = _lib.load()
    name, ml, eps, gamma = mode
    B, K = C.EXTRA_PAIR
    c = C.pair_case((B, K), mode)
    x, y = c['x'].to(DEV).contiguous(), c['y'].to(DEV)
    st = ops._stream()
    gl = torch.ones(1, device=DEV)

    def run(w, pw, eps, gamma, expect=0):
        b = {'lse': Guarded(B + 1), 'res': Guarded(2), 'grad': Guarded(B * K), 'w': None if w is None else Guarded(K, fill=w),
             'pw': None if pw is None else Guarded(K, fill=pw)}
        wp = None if w is None else b['w'].ptr
        pwp = None if pw is None else b['pw'].ptr
        acc = ctypes.c_void_p(b['res'].t.data_ptr() + 4)
        if ml:
            wsb = int(lib.sgnn_bce_logits_workspace_bytes(B))
            b['ws'] = Guarded(wsb // 4 + 1)
            assert lib.sgnn_bce_logits_fwd_shaped(ops._ptr(x), ops._ptr(y), B, K, b['res'].ptr, acc, b['ws'].ptr, wsb, st, wp, pwp, gamma) == expect
            assert lib.sgnn_bce_logits_bwd_shaped(ops._ptr(x), ops._ptr(y), ops._ptr(gl), B, K, b['grad'].ptr, st, wp, pwp, gamma) == expect
        else:
            wsb = int(lib.sgnn_cross_entropy_workspace_bytes(B))
            b['ws'] = Guarded(wsb // 4 + 1)
            assert lib.sgnn_cross_entropy_fwd_shaped(ops._ptr(x), ops._ptr(y), B, K, b['lse'].ptr, b['res'].ptr, acc, b['ws'].ptr, wsb, st,
                                                     wp, eps, gamma) == expect
            assert lib.sgnn_cross_entropy_bwd_shaped(ops._ptr(x), ops._ptr(y), b['lse'].ptr, ops._ptr(gl), B, K, b['grad'].ptr, st, wp, eps,
                                                     gamma) == expect
        torch.cuda.synchronize()
        return {k: v for k, v in b.items() if v is not None}
    got = run(c['w'], c['pw'], eps, gamma)
    for nm, buf in got.items():
        assert buf.intact(), nm
    _loss_close(got['res'].t[0], c['loss'])
    assert_close(got['grad'].t.view(B, K) * 1.5, c['grad'], 'grad logits', norm_tol=2e-5)
    absent, ones = run(None, None, eps, gamma), run(torch.ones(K), torch.ones(K) if ml else None, eps, gamma)
    for nm in ('res', 'grad') + (() if ml else ('lse',)):
        assert torch.equal(absent[nm].t, ones[nm].t) and ones[nm].intact(), nm
    for bad_eps, bad_gamma in [(0.0, -1.0), (0.0, float('nan'))] + ([] if ml else [(1.0, 0.0), (0.1, 2.0)]):
        b = run(c['w'], c['pw'], bad_eps, bad_gamma, expect=-1)
        for nm in ('lse', 'res', 'grad', 'ws'):
            assert bool((b[nm].buf == SENTINEL).all()), (bad_eps, bad_gamma, nm)


@pytest.mark.parametrize('mode', C.MODES, ids=lambda m: m[0])
def test_dropout_masks_do_not_depend_on_the_loss_mode(mode):
    """p = 0.3, the same {seed, step}: logits, a1, a2 and the state after a shaped call equal those of a bare call."""
    ops = _ops()
    name, ml, eps, gamma = mode
    shape = (3000, 40, 64, 32, 4)
    B, H0, H1, H2, K = shape
    g, mods, z1 = _raw_inputs(shape, seed=1)
    y = _labels(mode, B, K, g)
    rng = torch.tensor([1234, 5], dtype=torch.int64, device=DEV)
    shaped = _raw_head(shape, z1, mods, y, mode, w=WC.class_weights(K, g), p=0.3, rng=rng)
    assert rng.tolist() == [1234, 6]
    rng = torch.tensor([1234, 5], dtype=torch.int64, device=DEV)
    bare = _raw_head(shape, z1, mods, y, (name, ml, 0.0, 0.0), p=0.3, rng=rng)          # both 0: the bare launch
    assert rng.tolist() == [1234, 6]
    for nm in ('logits', 'a1', 'a2'):
        assert torch.equal(shaped[nm].t, bare[nm].t), nm
    assert float((bare['a1'].t == 0).float().mean()) > 0.3                              # masks were drawn
    assert not torch.equal(shaped['out'].t[:1], bare['out'].t[:1])                      # ... and the loss shaped
    # both 0 through the new entries IS the existing entry: against ops at the defaults
    x = torch.randn(B, H0, generator=g).to(DEV)
    r0 = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    kw = {'targets': y} if ml else {'labels': y}
    a = ops.fused_head(x, mods[0], mods[1], mods[2], p=0.3, rng=r0, **kw)
    r1 = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    b = ops.fused_head(x, mods[0], mods[1], mods[2], p=0.3, rng=r1, label_smoothing=0.0, focal_gamma=0.0, **kw)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and r0.tolist() == r1.tolist() == [1234, 1]


# ---- the model ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def datasets(tmp_path_factory):
    return write_datasets(tmp_path_factory.mktemp('shaped'))


MODEL_CASES = [('tiny', {'focal_gamma': 2.0}), ('tiny', {'label_smoothing': 0.1}), ('ml', {'focal_gamma': 2.0, 'pos_weight': 'balanced'})]


def _reference_loss(m, batch):
    """The float64 ShapedLoss value of the step's logits (no dropout in these models: the eval forward is the training one)."""
    from subgnn_amd.loss_weights import ShapedLoss
    labels = batch['label'].squeeze(-1)
    with torch.no_grad():
        m.eval()
        logits = m._forward_batch('train', batch)
        m.train()
    ref = ShapedLoss(m.multilabel, m.loss.label_smoothing, m.loss.focal_gamma,
                     weight=None if m.loss.weight is None else m.loss.weight.cpu(),
                     pos_weight=None if m.loss.pos_weight is None else m.loss.pos_weight.cpu())
    return float(ref(logits.double().cpu(), labels.cpu()))


@pytest.mark.parametrize('name,shape', MODEL_CASES)
def test_model_routes_agree(datasets, name, shape, monkeypatch):
    """One training step's loss is the float64 ShapedLoss value of its logits on each of the three routes (fused head, fused_head:
    false, fused_forward: false), every parameter gradient agrees across them, the kernel routes never reach the module's forward,
    and the loss is not the bare model's."""
    from subgnn_amd import ops
    from subgnn_amd.loss_weights import ShapedLoss
    res = {}
    for route, over in ROUTES:
        seen = {'head': 0, 'pair': 0, 'module': 0}
        o_head, o_ce, o_bce, o_fwd = ops.fused_head, ops.cross_entropy_with_accuracy, ops.bce_with_logits_and_accuracy, ShapedLoss.forward

        def shaped(k):
            return int(bool(k.get('label_smoothing')) or bool(k.get('focal_gamma')))

        def head(*a, _s=seen, **k):
            _s['head'] += shaped(k)
            return o_head(*a, **k)

        def pair(fn, _s=seen):
            def f(*a, **k):
                _s['pair'] += shaped(k)
                return fn(*a, **k)
            return f

        def fwd(self, *a, _s=seen, **k):
            _s['module'] += 1
            return o_fwd(self, *a, **k)
        monkeypatch.setattr(ops, 'fused_head', head)
        monkeypatch.setattr(ops, 'cross_entropy_with_accuracy', pair(o_ce))
        monkeypatch.setattr(ops, 'bce_with_logits_and_accuracy', pair(o_bce))
        monkeypatch.setattr(ShapedLoss, 'forward', fwd)
        try:
            m, loss, grads, batch = _step_gradients(datasets, name, **dict(shape, **over))
        finally:
            monkeypatch.undo()
        assert type(m.loss) is ShapedLoss
        want = _reference_loss(m, batch)
        print(name, shape, route, 'loss %.9g  float64 ShapedLoss %.9g' % (loss, want), seen)
        assert (seen['head'] > 0, seen['pair'] > 0, seen['module'] > 0) == {'fused': (True, False, False), 'standalone': (False, True, False),
                                                                           'library': (False, False, True)}[route], (route, seen)
        _loss_close(loss, want)
        res[route] = (loss, grads)
    ref_loss, ref_grads = res['library']
    for route in ('fused', 'standalone'):
        loss, grads = res[route]
        assert grads.keys() == ref_grads.keys() and len(grads) > 10
        for k in grads:
            assert_close(grads[k], ref_grads[k], '%s: grad %s' % (route, k))
    for k in res['fused'][1]:
        assert_close(res['fused'][1][k], res['standalone'][1][k], 'fused against stand-alone: grad ' + k, norm_tol=2e-5)
    _, bare_loss, _, _ = _step_gradients(datasets, name, **{k: v for k, v in shape.items() if k == 'pos_weight'})
    assert abs(bare_loss - ref_loss) > 1e-4 * abs(ref_loss), (bare_loss, ref_loss)


@pytest.mark.parametrize('name,shape', MODEL_CASES)
def test_validation_loss_is_the_modules(datasets, name, shape):
    from subgnn_amd.loss_weights import ShapedLoss
    m, hp = _model(datasets, name, **shape)
    torch.manual_seed(5)
    m.prepare_data()
    m.eval()
    with torch.no_grad():
        batch = m.make_batch('val', torch.arange(min(int(hp['batch_size']), len(m.val_sub_G))))
        out = m.validation_step(batch, 0)
        logits, labels = out['val_logits'], out['val_labels']
        assert type(m.loss) is ShapedLoss
        by_hand = m.loss(logits, labels.type_as(logits) if name == 'ml' else labels)
        assert torch.equal(out['val_loss'], by_hand)
        ref = ShapedLoss(m.multilabel, m.loss.label_smoothing, m.loss.focal_gamma,
                         weight=None if m.loss.weight is None else m.loss.weight.cpu(),
                         pos_weight=None if m.loss.pos_weight is None else m.loss.pos_weight.cpu())
        on_host = float(ref(logits.double().cpu(), labels.cpu()))
        host = m.val_test_outputs('val', logits.cpu(), labels.cpu())
        assert not host['val_loss'].is_cuda
        _loss_close(host['val_loss'], on_host)
        _loss_close(out['val_loss'], on_host)


@pytest.mark.parametrize('name,shape', MODEL_CASES)
def test_recorded_and_eager_epochs_agree(datasets, name, shape):
    """Two epochs of the Trainer with hip_graph_step True and False: {eps, gamma} travel by value in the launch, so the recorded
    step replays the shaped kernels -- training losses equal BIT FOR BIT; the validation loss (evaluated on host copies when
    recorded) within the 1e-6 the existing recorded-versus-eager tests ask."""
    from subgnn_amd.train_config import Trainer
    runs = {}
    for graph_step in (False, True):
        m, hp = _model(datasets, name, **shape)
        tr = Trainer(2, hp.get('grad_clip', 0.0), log=lambda *a, **k: None, hip_graph_step=graph_step)
        torch.manual_seed(5)
        tr.fit(m)
        assert tr.hip_graph_step == graph_step                               # the step was recorded, not abandoned
        runs[graph_step] = {'train': [h['train_loss'] for h in tr.history], 'val': [h['val_loss'] for h in tr.history]}
        assert all(np.isfinite(runs[graph_step]['train'] + runs[graph_step]['val']))
    for k in ('train', 'val'):
        print(name, shape, k, 'eager', ['%.9g' % v for v in runs[False][k]], 'recorded', ['%.9g' % v for v in runs[True][k]])
    assert runs[False]['train'] == runs[True]['train'], runs
    for a, b in zip(runs[False]['val'], runs[True]['val']):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), runs


def test_a_loss_assigned_by_hand(datasets):
    """model.loss = ShapedLoss(...) takes the kernels (its forward is not reached in training_step) and gives the float64 value;
    nn.CrossEntropyLoss(label_smoothing=0.1) still takes the library and gives torch's value."""
    from subgnn_amd.loss_weights import ShapedLoss
    m, hp = _model(datasets, 'tiny')
    torch.manual_seed(5)
    m.prepare_data()
    m.train()
    batch = m.make_batch('train', torch.arange(min(int(hp['batch_size']), len(m.train_sub_G))))
    labels = batch['label'].squeeze(-1)
    K = m.num_classes
    w = WC.class_weights(K, torch.Generator().manual_seed(4), zero=False)
    bare = float(m.training_step(batch, 0)['loss'])
    orig = ShapedLoss.forward
    for kw in ({'focal_gamma': 1.5}, {'label_smoothing': 0.2}):
        m.loss = ShapedLoss(False, weight=w, **kw).to(DEV)
        want = _reference_loss(m, batch)

        def boom(self, *a, **k):
            raise AssertionError('ShapedLoss.forward was reached in training_step')
        ShapedLoss.forward = boom
        try:
            got = float(m.training_step(batch, 0)['loss'])
        finally:
            ShapedLoss.forward = orig
        print(kw, 'bare %.9g  shaped %.9g  float64 %.9g' % (bare, got, want))
        _loss_close(got, want)
        assert abs(got - bare) > 1e-4 * abs(bare)
    with torch.no_grad():
        m.eval()
        logits = m._forward_batch('train', batch)
        m.train()
    m.loss = torch.nn.CrossEntropyLoss(weight=w.to(DEV), label_smoothing=0.1)
    calls = {'n': 0}
    orig_ce = F.cross_entropy

    def counted(*a, **k):
        calls['n'] += 1
        return orig_ce(*a, **k)
    F.cross_entropy = counted
    try:
        got = float(m.training_step(batch, 0)['loss'])
    finally:
        F.cross_entropy = orig_ce
    assert calls['n'] > 0
    _loss_close(got, float(F.cross_entropy(logits.double().cpu(), labels.cpu(), weight=w.double(), label_smoothing=0.1)))

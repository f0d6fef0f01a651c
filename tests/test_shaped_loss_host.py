"""CPU: what label smoothing and focal loss (hparams['label_smoothing'] / ['focal_gamma']) add below the GPU tests --
loss_weights.ShapedLoss against torch and against the closed forms, the refusals, make_loss / plan / route, the hyper-parameter
round trip, the state_dict, the C ABI entries and the built kernels' registers."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from helpers import write_dataset_from_golden
import shaped_loss_cases as C
import weighted_loss_cases as WC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import kernel_resources as KR                                      # noqa: E402

LIBDIR = os.path.join(REPO, 'subgnn_amd', 'lib')


# ---- ShapedLoss ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('eps', [0.1, 0.9])
def test_smoothing_is_torchs(weighted, eps):
    """ShapedLoss(label_smoothing=) IS F.cross_entropy(label_smoothing=): with and without weights, with -100 rows, to the bit."""
    from subgnn_amd.loss_weights import ShapedLoss
    g = torch.Generator().manual_seed(3)
    B, K = 50, 5
    x = torch.randn(B, K, generator=g, dtype=torch.float64) * 2
    y = WC.labels_for(B, K, g)
    assert int((y == -100).sum()) > 0
    w = WC.class_weights(K, g) if weighted else None
    for dtype in (torch.float64, torch.float32):
        xr = x.clone().to(dtype).detach().requires_grad_(True)
        got = ShapedLoss(False, label_smoothing=eps, weight=w)(xr, y)
        got.backward()
        xt = x.clone().to(dtype).detach().requires_grad_(True)
        want = F.cross_entropy(xt, y, weight=None if w is None else w.to(dtype), label_smoothing=eps)
        want.backward()
        assert torch.equal(got, want) and torch.equal(xr.grad, xt.grad)


def test_both_zero_is_the_weighted_nn_loss():
    from subgnn_amd.loss_weights import ShapedLoss
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(20, 4, generator=g), torch.randint(0, 4, (20,), generator=g)
    w = WC.class_weights(4, g)
    assert torch.equal(ShapedLoss(False, weight=w)(x, y), F.cross_entropy(x, y, weight=w))
    t = (torch.rand(20, 4, generator=g) < 0.4)
    pw = WC.class_weights(4, g, zero=False)
    want = F.binary_cross_entropy_with_logits(x, t.float(), weight=w, pos_weight=pw)
    assert torch.equal(ShapedLoss(True, weight=w, pos_weight=pw)(x, t.long()), want)
    assert torch.equal(ShapedLoss(True, weight=w, pos_weight=pw)(x, t.float()), want)      # (the model hands float targets)


def _closed_form_matches(x, y, w, pw, ml, eps, gamma, what):
    xr = x.detach().double().clone().requires_grad_(True)           # (a copy: the cases are shared and stay as they are)
    loss = C.shaped_loss(ml, eps, gamma, w, pw)(xr, y)
    (loss * 1.5).backward()
    loss = loss.detach()
    want_loss, want_grad = C.numpy_loss_and_grad(x.detach().double().numpy(), y.numpy(), None if w is None else w.numpy(),
                                                 None if pw is None else pw.numpy(), ml, eps, gamma, g=1.5)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(xr.grad).all()), what
    assert abs(float(loss) - want_loss) <= 1e-14 * max(1.0, abs(want_loss)), (what, float(loss), want_loss)
    err = float(np.abs(xr.grad.numpy() - want_grad).max())
    assert err <= 1e-14 * max(1.0, float(np.abs(want_grad).max())), (what, err)


@pytest.mark.parametrize('case', [c for c in C.all_pair_cases() if c[0][0] <= 257], ids=C.case_id)
def test_closed_forms_equal_float64_autograd_on_the_pair_cases(case):
    """The numpy restatement of every formula == float64 autograd of ShapedLoss, loss and gradient, on the stand-alone cases the GPU
    tests use -- -100 rows, zero weights and the constructed rows (lead / trail by 40 and 100) included."""
    shape, mode = case
    name, ml, eps, gamma = mode
    c = C.pair_case(shape, mode)
    _closed_form_matches(c['x'], c['y'], c['w'], c['pw'], ml, eps, gamma, C.case_id(case))
    if c['extreme'] and not ml:                            # the constructed rows are what they are said to be
        x, y = c['x'].double(), c['y']
        for r, lead in zip(c['extreme'], C.LEADS):
            others = torch.cat((x[r, :int(y[r])], x[r, int(y[r]) + 1:]))
            assert abs(float(x[r, int(y[r])] - others.max()) - lead) < 1e-4
    # without weight rows too
    _closed_form_matches(c['x'], c['y'], None, None, ml, eps, gamma, C.case_id(case) + ' unweighted')


@pytest.mark.parametrize('mode', C.MODES, ids=lambda m: m[0])
def test_head_cases_carry_their_constructed_rows(mode):
    """The (33, ...) head case: its last four rows lead / trail by at least 40 / 100 in the float64 logits, their labels have a
    positive weight, and the closed forms equal autograd on the case's logits."""
    name, ml, eps, gamma = mode
    c = C.head_case(C.EXTRA_SHAPE, mode)
    lg, y = c['ref']['logits'], c['y']
    assert c['extreme'] == [29, 30, 31, 32]
    for r, lead in zip(c['extreme'], C.LEADS):
        if ml:
            z = torch.where(y[r] != 0, lg[r], -lg[r])
            live = (c['w'] > 0) & ((y[r] == 0) | (c['pw'] > 0))
            assert float(z[live].max() if lead > 0 else -z[live].min()) >= abs(lead), (r, z)
        else:
            k = int(y[r])
            others = torch.cat((lg[r, :k], lg[r, k + 1:]))
            assert float(c['w'][k]) > 0 and (float(lg[r, k] - others.max()) >= lead if lead > 0 else float(others.max() - lg[r, k]) >= -lead)
    _closed_form_matches(lg, y, c['w'], c['pw'], ml, eps, gamma, name)


@pytest.mark.parametrize('gamma', [0.5, 1.0, 2.0])
def test_gradients_are_finite_and_zero_where_pt_is_one_in_float32(gamma):
    """A target logit leading by 40 (single-label: lse == x_y in float32, q = 0) and an element at z = +-120 (multi-label:
    sigmoid(-z) underflows): loss 0, gradient exactly 0 and finite, also for gamma < 1 where q^(gamma - 1) alone is infinite."""
    from subgnn_amd.loss_weights import ShapedLoss
    x = torch.tensor([[40.0, 0.0, -1.0], [0.5, 90.0, 1.0]], requires_grad=True)
    y = torch.tensor([0, 1])
    loss = ShapedLoss(False, focal_gamma=gamma, weight=[2.0, 0.5, 1.0])(x, y)
    loss.backward()
    assert float(loss) == 0.0 and bool(torch.isfinite(x.grad).all()) and bool((x.grad == 0).all()), (loss, x.grad)
    z = torch.tensor([[120.0, -120.0]], requires_grad=True)
    loss = ShapedLoss(True, focal_gamma=gamma, pos_weight=[3.0, 3.0])(z, torch.tensor([[1, 0]]))
    loss.backward()
    assert float(loss) == 0.0 and bool(torch.isfinite(z.grad).all()) and bool((z.grad == 0).all()), (loss, z.grad)
    # the other end: p_t = 0 (the target trails by 120): finite, the loss is w * 120 / w
    x = torch.tensor([[-120.0, 0.0, -1.0]], requires_grad=True)
    loss = ShapedLoss(False, focal_gamma=gamma)(x, torch.tensor([0]))
    loss.backward()
    assert math.isfinite(float(loss)) and abs(float(loss) - 120.313) < 1e-2 and bool(torch.isfinite(x.grad).all())


def test_refusals():
    from subgnn_amd import loss_weights as LW
    from subgnn_amd import ops
    bad = [dict(multilabel=True, label_smoothing=0.1),                # torch has no smoothing for BCE
           dict(multilabel=False, label_smoothing=0.1, focal_gamma=2.0),
           dict(multilabel=False, label_smoothing=1.0), dict(multilabel=False, label_smoothing=-0.1),
           dict(multilabel=False, label_smoothing=float('nan')),
           dict(multilabel=False, focal_gamma=-1.0), dict(multilabel=False, focal_gamma=float('inf')),
           dict(multilabel=True, focal_gamma=float('nan')), dict(multilabel=False, focal_gamma='2')]
    for kw in bad:
        with pytest.raises(ValueError):
            LW.ShapedLoss(**kw)
        with pytest.raises(ValueError):
            LW.make_loss(kw['multilabel'], None, None, kw.get('label_smoothing', 0.0), kw.get('focal_gamma', 0.0))
    with pytest.raises(ValueError):
        LW.ShapedLoss(False, focal_gamma=1.0, pos_weight=[1.0, 2.0])
    # ops refuse on the host, before any device is touched
    x, y = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    lin = [nn.Linear(4, 3), nn.Linear(3, 2), nn.Linear(2, 3)]
    for kw in ({'label_smoothing': 1.0}, {'label_smoothing': -0.5}, {'focal_gamma': -2.0}, {'focal_gamma': float('nan')},
               {'label_smoothing': 0.1, 'focal_gamma': 1.0}):
        with pytest.raises(ValueError):
            ops.cross_entropy_with_accuracy(x, y, **kw)
        with pytest.raises(ValueError):
            ops.fused_head(torch.zeros(2, 4), lin[0], lin[1], lin[2], labels=y, **kw)
    with pytest.raises(ValueError):
        ops.bce_with_logits_and_accuracy(x, torch.zeros(2, 3, dtype=torch.int64), focal_gamma=-1.0)
    with pytest.raises(ValueError):
        ops.fused_head(torch.zeros(2, 4), lin[0], lin[1], lin[2], targets=torch.zeros(2, 3, dtype=torch.int64), label_smoothing=0.1)


# ---- make_loss, plan, route -----------------------------------------------------------------------------------------------------------

def test_make_loss_with_both_keys_zero_returns_what_it_returned():
    from subgnn_amd import loss_weights as LW
    for ml, cw, pw in ((False, None, None), (False, [1.0, 2.0], None), (True, None, None), (True, [1.0, 2.0], [3.0, 4.0])):
        a, b = LW.make_loss(ml, cw, pw), LW.make_loss(ml, cw, pw, 0.0, 0.0)
        assert type(a) is type(b) is (nn.BCEWithLogitsLoss if ml else nn.CrossEntropyLoss)
        for name in ('weight', 'pos_weight'):
            u, v = getattr(a, name, None), getattr(b, name, None)
            assert (u is None and v is None) or torch.equal(u, v)
        assert list(b.state_dict().keys()) == []
    s = LW.make_loss(False, [1.0, 2.0], None, 0.1, 0.0)
    assert type(s) is LW.ShapedLoss and s.label_smoothing == 0.1 and s.focal_gamma == 0.0 and s.weight.tolist() == [1.0, 2.0]
    assert s.weight.dtype == torch.float32 and list(s.state_dict().keys()) == [] and s.pos_weight is None
    f = LW.make_loss(True, None, [3.0, 4.0], 0.0, 2.0)
    assert type(f) is LW.ShapedLoss and f.multilabel and f.focal_gamma == 2.0 and f.weight is None and f.pos_weight.tolist() == [3.0, 4.0]
    assert list(f.state_dict().keys()) == []
    LW.refuse_multi_rank(LW.make_loss(False, None, None, 0.0, 2.0))      # no weight rows: nothing to refuse, whatever the group


def test_plan_and_route_for_every_module_kind():
    from subgnn_amd import loss_weights as LW
    w3 = torch.tensor([1.0, 2.0, 0.5])
    # nn modules: kernel_plan keeps every answer, plan appends (0.0, 0.0), route is unchanged
    for what, make, hp, ml, head_ok, want in WC.route_cases():
        kp = LW.kernel_plan(make(), ml, 3)
        p = LW.plan(make(), ml, 3)
        assert (p is None) == (kp is None), what
        if kp is not None:
            assert len(p) == 4 and p[2:] == (0.0, 0.0), what
            for a, b in zip(p[:2], kp):
                assert (a is None and b is None) or torch.equal(a, b), what
        assert LW.route(make(), hp, ml, 3, head_ok) == want, what
    assert LW.kernel_plan(nn.CrossEntropyLoss(label_smoothing=0.1), False, 3) is None
    assert LW.plan(nn.CrossEntropyLoss(label_smoothing=0.1), False, 3) is None
    assert LW.route(nn.CrossEntropyLoss(label_smoothing=0.1), {}, False, 3, True) == 'library'
    # kernel_plan does not know ShapedLoss: plan does
    s = LW.ShapedLoss(False, label_smoothing=0.1, weight=w3)
    assert LW.kernel_plan(s, False, 3) is None
    p = LW.plan(s, False, 3)
    assert p[0] is s.weight and p[1] is None and p[2:] == (0.1, 0.0)
    f = LW.ShapedLoss(True, focal_gamma=2.0, pos_weight=w3)
    p = LW.plan(f, True, 3)
    assert p[0] is None and p[1] is f.pos_weight and p[2:] == (0.0, 2.0)
    assert LW.plan(LW.ShapedLoss(False, focal_gamma=2.0), False, 3) == (None, None, 0.0, 2.0)
    # what sends a ShapedLoss to the library: rows of another length or device, the other kind of dataset, a subclass
    assert LW.plan(s, False, 4) is None and LW.plan(s, False, 3, device='meta') is None
    assert LW.plan(s, True, 3) is None and LW.plan(f, False, 3) is None
    assert LW.plan(type('Mine', (LW.ShapedLoss,), {})(False, focal_gamma=1.0), False, 3) is None
    for loss, ml in ((s, False), (f, True)):
        assert LW.route(loss, {}, ml, 3, True) == 'fused_head'
        assert LW.route(loss, {}, ml, 3, False) == 'standalone'
        assert LW.route(loss, {'fused_head': False}, ml, 3, True) == 'standalone'
        assert LW.route(loss, {'fused_forward': False}, ml, 3, True) == 'library'
    assert LW.route(f, {'fused_multilabel_loss': False}, True, 3, True) == 'library'
    assert LW.route(s, {}, False, 4, True) == 'library'


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def _model(tiny, root, **over):
    from subgnn_amd import config
    from subgnn_amd.SubGNN import SubGNN, dataset_paths
    name = write_dataset_from_golden(tiny, root)
    config.PROJECT_ROOT = root
    hp = dict(tiny.hp)
    hp.update(over)
    torch.manual_seed(0)
    return SubGNN(hp, **dataset_paths(name))


def test_model_builds_a_shaped_loss_and_keeps_its_state_dict(tiny, tmp_path):
    from subgnn_amd import loss_weights as LW
    bare = _model(tiny, tmp_path)
    assert type(bare.loss) is nn.CrossEntropyLoss
    zero = _model(tiny, tmp_path, label_smoothing=0.0, focal_gamma=0.0)
    assert type(zero.loss) is nn.CrossEntropyLoss and zero.loss.weight is None
    foc = _model(tiny, tmp_path, focal_gamma=2.0, class_weight='balanced')
    bal = _model(tiny, tmp_path, class_weight='balanced')
    assert type(foc.loss) is LW.ShapedLoss and foc.loss.focal_gamma == 2.0 and not foc.loss.multilabel
    assert torch.equal(foc.loss.weight, bal.loss.weight) and foc.loss.weight.device == foc.lin3.weight.device
    smo = _model(tiny, tmp_path, label_smoothing=0.1)
    assert type(smo.loss) is LW.ShapedLoss and smo.loss.label_smoothing == 0.1 and smo.loss.weight is None
    for m in (foc, smo, zero):
        assert list(m.state_dict().keys()) == list(bare.state_dict().keys())
        bare.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})       # strict, both ways
        m.load_state_dict({k: v.clone() for k, v in bare.state_dict().items()})
    for kw in ({'label_smoothing': 0.1, 'focal_gamma': 2.0}, {'label_smoothing': 1.0}, {'focal_gamma': -1.0},
               {'focal_gamma': float('inf')}):
        with pytest.raises(ValueError):
            _model(tiny, tmp_path, **kw)
    # the validation loss is the module's
    g = torch.Generator().manual_seed(1)
    K = bare.num_classes
    logits, labels = torch.randn(6, K, generator=g), torch.randint(0, K, (6,), generator=g)
    out = smo.val_test_outputs('val', logits, labels)
    assert torch.equal(out['val_loss'], F.cross_entropy(logits, labels, label_smoothing=0.1))
    out = foc.val_test_outputs('val', logits, labels)
    ref = LW.ShapedLoss(False, focal_gamma=2.0, weight=foc.loss.weight.cpu())(logits, labels)
    assert abs(float(out['val_loss']) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))


def test_numbers_round_trip_through_hyperparams_json_and_a_search_choice_reaches_the_model(tiny, tmp_path):
    from test_gpu_train_driver import CONFIG
    from subgnn_amd import config, train_config
    from subgnn_amd import loss_weights as LW
    write_dataset_from_golden(tiny, tmp_path, 'ds')
    fix = dict(tiny.hp)
    for k in ('batch_size', 'learning_rate', 'n_layers'):
        fix.pop(k, None)
    fix.update({'max_epochs': 1, 'seed': 3, 'label_smoothing': 0.15})
    (tmp_path / 'config.json').write_text(CONFIG % json.dumps(fix))
    config.PROJECT_ROOT = tmp_path
    rc = train_config.read_json(tmp_path / 'config.json')
    model, hp = train_config.build_model(rc, train_config.FixedTrial())
    assert hp['label_smoothing'] == 0.15 and type(model.loss) is LW.ShapedLoss and model.loss.label_smoothing == 0.15
    train_config.write_hyperparams(tmp_path / 'results', hp)
    back = json.loads((tmp_path / 'results' / 'hyperparams.json').read_text())
    assert back['label_smoothing'] == 0.15
    again, _ = train_config.build_model(rc, hp=back)
    assert type(again.loss) is LW.ShapedLoss and again.loss.label_smoothing == 0.15
    assert list(again.state_dict().keys()) == list(model.state_dict().keys())
    # a hyperparams_optuna choice of focal_gamma reaches the trial's model
    rc['hyperparams_fix'].pop('label_smoothing')
    rc['hyperparams_optuna']['focal_gamma'] = {'type': 'suggest_categorical', 'args': [[0.0, 1.0, 2.0]]}
    m2, hp2 = train_config.build_model(rc, train_config.FixedTrial({'focal_gamma': 2.0}))
    assert hp2['focal_gamma'] == 2.0 and type(m2.loss) is LW.ShapedLoss and m2.loss.focal_gamma == 2.0
    m0, hp0 = train_config.build_model(rc, train_config.FixedTrial({'focal_gamma': 0.0}))
    assert hp0['focal_gamma'] == 0.0 and type(m0.loss) is nn.CrossEntropyLoss


# ---- C ABI and kernels ------------------------------------------------------------------------------------------------------------------

def _header():
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'\b(sgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', bare)}


def test_abi_entries_are_declared_mirrored_exported_and_refuse_on_the_host():
    from subgnn_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    decl = _header()
    for name in C.NEW_ENTRIES:
        base = name[:-len('_shaped')] + '_weighted'
        extra = 1 if ('_ml_' in name or '_bce_' in name) else 2
        assert name in decl, name
        assert decl[name][:-extra] == decl[base], name                # the weighted list plus the floats at the end
        assert decl[name][-extra:] == ['float label_smoothing', 'float focal_gamma'][-extra:], decl[name][-extra:]
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][1][:-extra] == _lib.SIGNATURES[base][1], name
        assert len(_lib.SIGNATURES[name][1]) == len(decl[name]) and hasattr(lib, name), name
    # a value outside its domain, or both non-zero: -1 (SGNN_ERR_BAD_ARG) on the host, before the other arguments are looked at
    for eps, gamma in ((1.0, 0.0), (-0.1, 0.0), (float('nan'), 0.0), (0.0, -1.0), (0.0, float('inf')), (0.0, float('nan')), (0.1, 2.0)):
        assert lib.sgnn_cross_entropy_fwd_shaped(None, None, 1, 1, None, None, None, None, 0, None, None, eps, gamma) == -1
        assert lib.sgnn_cross_entropy_bwd_shaped(None, None, None, None, 1, 1, None, None, None, eps, gamma) == -1
        assert lib.sgnn_head_fwd_shaped(None, 1, 1, 1, 1, None, None, None, None, None, 0.0, None, None, None, None, None, None, None, 0,
                                        None, None, eps, gamma) == -1
        assert lib.sgnn_head_bwd_shaped(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, 0.0, None, None, None,
                                        None, eps, gamma) == -1
    for gamma in (-1.0, float('inf'), float('nan'), 2.0):           # (2.0: null required pointers)
        assert lib.sgnn_bce_logits_fwd_shaped(None, None, 1, 1, None, None, None, 0, None, None, None, gamma) == -1
        assert lib.sgnn_bce_logits_bwd_shaped(None, None, None, 1, 1, None, None, None, None, gamma) == -1
        assert lib.sgnn_head_fwd_ml_shaped(None, 1, 1, 1, 1, None, None, None, None, None, 0.0, None, None, None, None, None, None, 0, None,
                                           None, None, gamma) == -1
        assert lib.sgnn_head_bwd_ml_shaped(None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, 0.0, None, None, None, None,
                                           None, gamma) == -1


def test_shaped_kernels_neither_spill_vectors_nor_use_scratch():
    from subgnn_amd import build
    build.build(verbose=False)
    ks = [k for f in ('head.o', 'loss.o') for k in KR.kernels(os.path.join(LIBDIR, f))]
    assert len(C.SHAPED_KERNELS) == 18
    for pattern in C.SHAPED_KERNELS:
        hits = [k for k in ks if pattern in k['demangled']]
        assert len(hits) == 1, (pattern, [k['demangled'] for k in hits])
        k = hits[0]
        print('%-60s vgpr %3d  vspill %d  sspill %2d  scratch %d' % (k['demangled'][:60], k['vgpr_count'], k['vgpr_spill_count'],
                                                                     k['sgpr_spill_count'], k['private_segment_fixed_size']))
        assert k['vgpr_spill_count'] == 0, (k['demangled'], k['vgpr_spill_count'])
        assert k['private_segment_fixed_size'] == 0, (k['demangled'], k['private_segment_fixed_size'])
        # kernels of their own, outside the name patterns tests/test_kernel_resources.py ratchets
        assert 'head_fwd_kernel' not in k['demangled'] and 'head_bwd_kernel<1>' not in k['demangled']

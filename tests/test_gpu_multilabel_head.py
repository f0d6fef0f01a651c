"""-m gpu: the multi-label mode of the fused head (csrc/head.hip: head_fwd_ml_kernel / head_bwd_ml_kernel), the stand-alone pair
sgnn_bce_logits_fwd / _bwd (csrc/loss.hip) and the model path that uses them (SubGNN.training_step on a multi-label dataset,
hparams['fused_multilabel_loss']): nn.BCEWithLogitsLoss (SubGNN.py:133) + the exact-match accuracy of su:108-124 against float64
torch on the CPU; the accuracy against torch's own ``sigmoid(x) > 0.5`` ON THE DEVICE from the kernel's returned logits (a float64
reference may predict otherwise on a logit within rounding of the threshold)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, write_dataset_from_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ops():
    from subgnn_amd import ops
    return ops


def _head_modules(H0, H1, H2, K, seed):
    """Initialisation of tests/test_gpu_float.py::test_fused_head_matches_torch (activations and logits of order 1)."""
    g = torch.Generator().manual_seed(seed)
    mods = [torch.nn.Linear(H0, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, K)]
    for m in mods:
        m.weight.data = torch.randn(m.weight.shape, generator=g) / m.in_features ** 0.5
        m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.3
    return mods


def _device_hits(lg, targets):
    """The yardstick of every accuracy here: torch's ``sigmoid(x) > 0.5`` on the device, from the kernel's own logits -> the rows
    whose K predictions all equal their targets, as a float32 vector of 0 / 1."""
    return ((torch.sigmoid(lg) > 0.5) == (targets != 0)).all(1).float()


def _assert_accuracy(acc, lg, targets):
    """acc is EXACTLY hits / B with torch's hits.  The quotient is the correctly rounded float32 division the kernels (and
    sklearn's accuracy_score, in double) compute: ``.float().mean()`` of torch on the device multiplies the sum by a rounded
    1 / B instead and is one ulp off at e.g. 8685 / 70001 (measured: 0.12406966 against 0.12406965), with the same hits -- so the
    hit COUNT is compared exactly, and the quotient against the IEEE division of that count."""
    B = lg.shape[0]
    hits = int(_device_hits(lg, targets).sum())
    assert acc.shape == (1,)
    assert round(float(acc) * B) == hits, (float(acc) * B, hits)
    assert float(acc) == float(torch.tensor(float(hits), dtype=torch.float32) / B), (float(acc), hits, B)


def _sweep_values():
    """+-2^-e for e = 18..30 (26 logits), 0.0 and -0.0: around the largest x whose float32 sigmoid still rounds to 0.5."""
    v = [s * 2.0 ** -e for e in range(18, 31) for s in (1.0, -1.0)] + [0.0, -0.0]
    return torch.tensor(v, dtype=torch.float32)


@pytest.mark.parametrize('B,H0,H1,H2,K', [(1, 7, 3, 2, 1), (31, 20, 16, 8, 2), (32, 20, 16, 8, 2), (33, 20, 16, 8, 2),
                                          (1000, 566, 64, 64, 10), (4133, 130, 128, 128, 32), (9000, 70, 100, 37, 5),
                                          (32801, 16, 8, 8, 3)])
def test_multilabel_head_matches_torch(B, H0, H1, H2, K):
    """ops.fused_head(targets=) (p = 0) == lin -> relu -> lin2 -> relu -> lin3 -> BCEWithLogitsLoss of float64 torch on the CPU:
    logits, loss, every gradient; the accuracy exactly torch's on the device; the call twice bit-identical; a gradient through the
    logits as well as the loss adds up."""
    ops = _ops()
    g = torch.Generator().manual_seed(B + H0)
    x = torch.randn(B, H0, generator=g)
    targets = (torch.rand(B, K, generator=g) < 0.35).long()
    if B > 10:
        targets[3, 0] = 7                                  # a non-zero target counts as 1
    tf = (targets != 0).double()
    ref_m, got_m = [m.double() for m in _head_modules(H0, H1, H2, K, 3)], [m.to(DEV) for m in _head_modules(H0, H1, H2, K, 3)]
    xr = x.double().requires_grad_(True)
    lg_r = ref_m[2](F.relu(ref_m[1](F.relu(ref_m[0](xr)))))
    loss_r = F.binary_cross_entropy_with_logits(lg_r, tf)
    loss_r.backward()
    td = targets.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    lg, loss, acc = ops.fused_head(xg, got_m[0], got_m[1], got_m[2], None, 0.0, None, targets=td)
    loss.backward()
    assert_close(lg.detach(), lg_r.detach(), 'logits')
    assert abs(float(loss.detach()) - float(loss_r.detach())) <= 1e-5 * max(1.0, abs(float(loss_r.detach())))
    _assert_accuracy(acc, lg.detach(), td)
    assert_close(xg.grad, xr.grad, 'grad x', norm_tol=2e-5)
    for a, b, nm in zip(got_m, ref_m, ('lin', 'lin2', 'lin3')):
        assert_close(a.weight.grad, b.weight.grad, 'grad %s.weight' % nm, norm_tol=2e-5)
        assert_close(a.bias.grad, b.bias.grad, 'grad %s.bias' % nm, norm_tol=2e-5)
    # twice the same call: bit-identical (fixed summation orders, the ticket leaves its counter at zero)
    lg3, loss3, acc3 = ops.fused_head(x.to(DEV), got_m[0], got_m[1], got_m[2], None, 0.0, None, targets=td)
    assert torch.equal(lg3, lg.detach()) and torch.equal(loss3, loss.detach()) and torch.equal(acc3, acc)
    # a gradient that arrives through the logits as well as the loss
    for m in got_m + ref_m:
        m.zero_grad()
    go = torch.randn(B, K, generator=g)
    xg2 = x.to(DEV).requires_grad_(True)
    lg2, loss2, _ = ops.fused_head(xg2, got_m[0], got_m[1], got_m[2], None, 0.0, None, targets=td)
    (loss2 + (lg2 * go.to(DEV)).sum()).backward()
    xr2 = x.double().requires_grad_(True)
    lg_r2 = ref_m[2](F.relu(ref_m[1](F.relu(ref_m[0](xr2)))))
    (F.binary_cross_entropy_with_logits(lg_r2, tf) + (lg_r2 * go.double()).sum()).backward()
    assert_close(xg2.grad, xr2.grad, 'grad x through loss + logits', norm_tol=2e-5)
    assert_close(got_m[1].weight.grad, ref_m[1].weight.grad, 'grad lin2.weight through loss + logits', norm_tol=2e-5)
    assert_close(got_m[2].bias.grad, ref_m[2].bias.grad, 'grad lin3.bias through loss + logits', norm_tol=2e-5)


def test_threshold_sweep_standalone():
    """The prediction rule is torch's float32 ``sigmoid(x) > 0.5`` on the device, not ``x > 0``: logits +-2^-18 .. +-2^-30 and
    both zeros, each against target 0 and target 1, one value per row (K = 1) -- per-row hits from single-row calls and from
    all rows at once."""
    ops = _ops()
    v = _sweep_values()
    x = torch.cat([v, v]).view(-1, 1).to(DEV)
    t = torch.cat([torch.zeros(len(v)), torch.ones(len(v))]).long().view(-1, 1).to(DEV)
    want = _device_hits(x, t)
    print('device threshold: sigmoid(x) > 0.5 is', dict(zip(['%+.0e' % float(a) for a in v], (torch.sigmoid(v.to(DEV)) > 0.5).tolist())))
    for i in range(x.shape[0]):
        _, acc = ops.bce_with_logits_and_accuracy(x[i:i + 1], t[i:i + 1])
        assert float(acc) == float(want[i]), (float(x[i]), int(t[i]), float(acc), float(want[i]))
    _, acc = ops.bce_with_logits_and_accuracy(x, t)
    _assert_accuracy(acc, x, t)


def test_threshold_sweep_fused_head():
    """The same sweep through the fused head: lin3.weight = 0 and lin3.bias = the values make every row's logits the sweep itself
    (K = 28); the targets are chosen per row so that each row hits or misses on ONE column only."""
    ops = _ops()
    v = _sweep_values()
    K = len(v)
    mods = [m.to(DEV) for m in _head_modules(5, 4, 3, K, 1)]
    mods[2].weight.data.zero_()
    mods[2].bias.data.copy_(v.to(DEV))
    pred = torch.sigmoid(v.to(DEV)) > 0.5                     # torch's prediction per column, on the device
    # row i < K: every target equals torch's prediction except column i (flipped): a miss unless the kernel disagrees there;
    # row K: all targets equal the predictions: a hit only if the kernel agrees with torch in every column
    t = pred.long().repeat(K + 1, 1)
    for i in range(K):
        t[i, i] = 1 - t[i, i]
    x = torch.randn(K + 1, 5, generator=torch.Generator().manual_seed(2)).to(DEV)
    lg, _, acc = ops.fused_head(x, mods[0], mods[1], mods[2], None, 0.0, None, targets=t)
    assert torch.equal(lg, v.to(DEV).repeat(K + 1, 1))
    _assert_accuracy(acc, lg, t)
    assert int(_device_hits(lg, t).sum()) == 1
    for i in range(K + 1):                                      # row by row: no column is predicted otherwise than torch does
        _, _, a = ops.fused_head(x[i:i + 1], mods[0], mods[1], mods[2], None, 0.0, None, targets=t[i:i + 1])
        assert float(a) == (1.0 if i == K else 0.0), (i, float(a))


def test_extreme_logits():
    """+-50, +-90, +-1e4: exp(-x) overflows float32 past 88.7 -- the loss stays finite and equal to the float64 value, the
    gradients finite, sigma saturates to exactly 0 or 1 (never NaN); through the stand-alone pair and the fused head."""
    ops = _ops()
    v = torch.tensor([50.0, -50.0, 90.0, -90.0, 1e4, -1e4])
    x = torch.cat([v, v]).view(-1, 1)
    t = torch.cat([torch.zeros(6), torch.ones(6)]).long().view(-1, 1)
    ref = F.binary_cross_entropy_with_logits(x.double(), t.double())
    xg = x.to(DEV).requires_grad_(True)
    loss, acc = ops.bce_with_logits_and_accuracy(xg, t.to(DEV))
    (loss * x.numel()).backward()                            # grad = (sigma - y) * 12 / 12: the scale is exactly 1
    assert torch.isfinite(loss) and abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
    assert torch.isfinite(xg.grad).all()
    sig = xg.grad.cpu() + t.float()
    assert torch.equal(sig[[4, 5, 10, 11]].view(-1), torch.tensor([1.0, 0.0, 1.0, 0.0]))
    _assert_accuracy(acc, xg.detach(), t.to(DEV))
    # the fused head: lin3.weight = 0, lin3.bias = the six values, rows with all-zero and all-one targets
    mods = [m.to(DEV) for m in _head_modules(5, 4, 3, 6, 1)]
    mods[2].weight.data.zero_()
    mods[2].bias.data.copy_(v.to(DEV))
    tt = torch.stack([torch.zeros(6), torch.ones(6)]).long().to(DEV)
    xh = torch.randn(2, 5, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    lg, lh, _ = ops.fused_head(xh, mods[0], mods[1], mods[2], None, 0.0, None, targets=tt)
    (lh * 12).backward()
    assert torch.isfinite(lh) and abs(float(lh.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
    gb = mods[2].bias.grad.cpu()                              # sum over the two rows of sigma - y
    assert torch.isfinite(gb).all() and torch.isfinite(xh.grad).all() and torch.isfinite(mods[1].weight.grad).all()
    assert torch.equal(gb[4:], torch.tensor([1.0, -1.0]))                      # sigma(1e4) = 1 twice - 1; sigma(-1e4) = 0 twice - 1


@pytest.mark.parametrize('B,K', [(1, 1), (33, 10), (1000, 100), (70001, 3)])
def test_standalone_pair_matches_torch(B, K):
    ops = _ops()
    g = torch.Generator().manual_seed(B + K)
    x = torch.randn(B, K, generator=g) * 3
    t = (torch.rand(B, K, generator=g) < 0.4).long()
    if B > 10:
        t[5, 0] = -3                                       # non-zero: 1
    xr = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(xr, (t != 0).double())
    ref.backward()
    xg = x.to(DEV).requires_grad_(True)
    loss, acc = ops.bce_with_logits_and_accuracy(xg, t.to(DEV))
    (loss * 1.5).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * max(1.0, abs(float(ref.detach())))
    _assert_accuracy(acc, xg.detach(), t.to(DEV))
    assert_close(xg.grad, xr.grad * 1.5, 'grad logits', norm_tol=2e-5)
    loss2, acc2 = ops.bce_with_logits_and_accuracy(x.to(DEV), t.to(DEV))
    assert torch.equal(loss2, loss.detach()) and torch.equal(acc2, acc)


def test_dropout_masks_do_not_depend_on_the_loss_mode():
    """p = 0.3, the same {seed, step}: the logits of the multi-label call are those of the label-less call bit for bit, and the
    step counter advances by one per call."""
    ops = _ops()
    B, H0, H1, H2, K, p = 3000, 40, 64, 32, 4, 0.3
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H0, generator=g).to(DEV)
    mods = [m.to(DEV) for m in _head_modules(H0, H1, H2, K, 5)]
    t = (torch.rand(B, K, generator=g) < 0.5).long().to(DEV)
    rng = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    lg_a, loss_a, _ = ops.fused_head(x, mods[0], mods[1], mods[2], None, p, rng, targets=t)
    assert rng.tolist() == [1234, 1]
    lg_b, _, _ = ops.fused_head(x, mods[0], mods[1], mods[2], None, p, rng, targets=t)
    assert rng.tolist() == [1234, 2] and not torch.equal(lg_a, lg_b)
    rng0 = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    lg_c, loss_c, acc_c = ops.fused_head(x, mods[0], mods[1], mods[2], None, p, rng0)
    assert rng0.tolist() == [1234, 1] and loss_c is None and acc_c is None
    assert torch.equal(lg_a, lg_c)
    rng1 = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    lg_d, loss_d, _ = ops.fused_head(x, mods[0], mods[1], mods[2], None, p, rng1, targets=t)
    assert torch.equal(lg_a, lg_d) and torch.equal(loss_a, loss_d)


# ---- the model ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def ml_dataset(tmp_path_factory):
    """The density golden turned multi-label as tests/test_gpu_train_driver.py does it: every third label a pair."""
    from conftest import load_golden
    root = tmp_path_factory.mktemp('multilabel')
    golden = load_golden('density')
    name = write_dataset_from_golden(golden, root, with_ego=False)
    f = os.path.join(str(root), name, 'subgraphs.pth')
    rows = open(f).read().splitlines()
    out = []
    for i, r in enumerate(rows):
        c = r.split('\t')
        lab = int(c[1])
        c[1] = '%d-%d' % (lab, (lab + 1) % 3) if i % 3 == 0 else str(lab)
        out.append('\t'.join(c))
    open(f, 'w').write('\n'.join(out) + '\n')
    return root, name, golden


def _model(ds, **over):
    from subgnn_amd import config
    from subgnn_amd.SubGNN import SubGNN, dataset_paths
    root, name, golden = ds
    config.PROJECT_ROOT = root
    hp = dict(golden.hp)
    hp.update({'seed': golden.seed, 'neigh_sample_border_size': 2, 'lin_dropout': 0.0, 'lstm_dropout': 0.0})
    hp.update(over)
    torch.manual_seed(0)
    m = SubGNN(hp, **dataset_paths(name))
    assert m.multilabel and isinstance(m.loss, torch.nn.BCEWithLogitsLoss)
    return m, hp


def _one_step(ds, monkeypatch=None, **over):
    """One eager training step (training_step -> backward -> clip -> Adam) on the first batch -> (loss, parameters after it,
    kernels the step launched or None)."""
    from subgnn_amd import standins
    from subgnn_amd.graph_step import train_step
    m, hp = _model(ds, **over)
    torch.manual_seed(5)
    m.prepare_data()
    m.train()
    opt = m.configure_optimizers()
    B = min(int(hp['batch_size']), len(m.train_sub_G))
    batch = m.make_batch('train', torch.arange(B))
    if monkeypatch is not None:
        def boom(*a, **k):
            raise AssertionError('F.binary_cross_entropy_with_logits was reached in training_step')
        monkeypatch.setattr(F, 'binary_cross_entropy_with_logits', boom)
    try:
        loss = float(train_step(m, opt, batch, hp.get('grad_clip', 0.0))[0])
        post = {k: v.detach().clone() for k, v in m.state_dict().items() if v.dtype == torch.float32}
        n_k = standins.count_kernels(lambda: train_step(m, opt, batch, hp.get('grad_clip', 0.0)))
    finally:
        if monkeypatch is not None:
            monkeypatch.undo()
    return loss, post, n_k


def test_model_step_fused_and_library_paths_agree(ml_dataset, monkeypatch):
    """hparams['fused_multilabel_loss'] True / False from the same initial state: the losses within 1e-5 relative, the parameters
    after the step within 1e-4 element-wise (test_one_trainer_step_matches_the_reference's tolerance); the fused model never
    reaches F.binary_cross_entropy_with_logits; its step launches strictly fewer kernels."""
    loss_t, post_t, k_t = _one_step(ml_dataset, monkeypatch, fused_multilabel_loss=True)
    loss_f, post_f, k_f = _one_step(ml_dataset, None, fused_multilabel_loss=False)
    assert np.isfinite(loss_t) and abs(loss_t - loss_f) <= 1e-5 * max(1.0, abs(loss_f)), (loss_t, loss_f)
    assert post_t.keys() == post_f.keys() and len(post_t) > 10
    for k in post_t:
        assert_close(post_t[k], post_f[k], 'post-step ' + k, 1e-4)
    print('kernels per eager step: fused %s, library %s' % (k_t, k_f))
    if k_t is not None and k_f is not None:
        assert k_t < k_f, (k_t, k_f)


def test_model_step_through_the_standalone_pair(ml_dataset, monkeypatch):
    """A head the fused kernel does not take (linear_hidden_dim_1 = 130 > 128) trains through ops.bce_with_logits_and_accuracy:
    the library loss is not reached, and the step agrees with the library path."""
    from subgnn_amd import ops
    assert not ops.head_supported(130, 32, 3)
    loss_t, post_t, _ = _one_step(ml_dataset, monkeypatch, linear_hidden_dim_1=130, fused_multilabel_loss=True)
    loss_f, post_f, _ = _one_step(ml_dataset, None, linear_hidden_dim_1=130, fused_multilabel_loss=False)
    assert np.isfinite(loss_t) and abs(loss_t - loss_f) <= 1e-5 * max(1.0, abs(loss_f)), (loss_t, loss_f)
    for k in post_t:
        assert_close(post_t[k], post_f[k], 'post-step ' + k, 1e-4)


def test_recorded_and_eager_epochs_agree(ml_dataset):
    """Two epochs of the Trainer with hip_graph_step True and False on the fused multi-label model agree to 1e-6 (as the driver
    test asks of the library path): the recorded step replays the multi-label head's launches."""
    from subgnn_amd.train_config import Trainer
    runs = {}
    for graph_step in (False, True):
        m, hp = _model(ml_dataset)
        tr = Trainer(2, hp.get('grad_clip', 0.0), log=lambda *a, **k: None, hip_graph_step=graph_step)
        torch.manual_seed(5)
        tr.fit(m)
        runs[graph_step] = [v for h in tr.history for v in (h['train_loss'], h['val_loss'])]
        assert all(np.isfinite(runs[graph_step]))
        assert runs[graph_step][2] < runs[graph_step][0]                  # the training loss went down
    for a, b in zip(runs[False], runs[True]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), runs

"""-m gpu: structure_similarity_fn = 'dtw_exact' -- the exact DTW distance in fastdtw's place, from the kernels up to the
model.  Every comparison is bit for bit: the cost function is the one whose division step is proven exact on the CPU
(test_reciprocal_division_is_exact), min and + round once, and the value of a minimum over warp paths does not depend on
the order cells are visited in."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from dtw_exact_ref import exact_dtw_similarities, seeded_set
from helpers import write_dataset_from_golden
from oracle import fastdtw_restate as FD

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FN = 'dtw_exact'


def _ops():
    from subgnn_amd import ops
    return ops


def _call(xs, ys, max_x, max_y, **kw):
    ops = _ops()
    X, Y = ops.Ragged.from_lists(xs, DEV), ops.Ragged.from_lists(ys, DEV)
    return ops.dtw_similarity(X.ptr, X.nodes, max_x, Y.ptr, Y.nodes, max_y, fn=kw.pop('fn', FN), **kw)


def _raw(xs, ys, max_x, max_y, kernel):
    """sgnn_dtw_exact_similarity into an output buffer of NaNs -> the buffer."""
    from subgnn_amd import _lib
    ops = _ops()
    lib = _lib.load()
    X, Y = ops.Ragged.from_lists(xs, DEV), ops.Ragged.from_lists(ys, DEV)
    out = torch.full((len(xs), len(ys)), float('nan'), dtype=torch.float32, device=DEV)
    wsb = lib.sgnn_dtw_exact_workspace_bytes(len(xs), max_x, len(ys), max_y)
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.sgnn_dtw_exact_similarity(p(X.ptr), p(X.nodes), len(xs), max_x, p(Y.ptr), p(Y.nodes), len(ys), max_y, kernel, None,
                                       p(out), p(ws), wsb, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('sort', [True, False])
def test_seeded_set_equals_the_oracle(sort):
    """64 x rows (3 empty) against 48 y rows, sorted like degree sequences and as drawn: the kernels equal
    oracle.fastdtw_restate.exact_dtw on all 2928 pairs, empty rows are PAD, no predecessor rule changes anything -- and the
    result is NOT fastdtw's (rule 2 lies above the exact distance on 10 sorted / 1161 unsorted pairs of this set)."""
    xs, ys = seeded_set(sort)
    want = np.zeros((64, 48), dtype=np.float32)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            if x:
                want[i, j] = np.float32(1.0 / (FD.exact_dtw(x, y, FD.calc_dist) + 1.0))
    assert np.array_equal(want, exact_dtw_similarities(xs, ys))
    got = _call(xs, ys, 20, 50)
    assert got.dtype == torch.float32 and got.shape == (64, 48)
    assert np.array_equal(got.cpu().numpy(), want)
    empty = [i for i, x in enumerate(xs) if not x]
    assert len(empty) == 3 and float(got[empty].abs().max()) == 0.0
    assert torch.equal(_call(xs, ys, 20, 50, kernel=1), got)       # the general kernel
    for tie in (0, 1, 2):
        assert torch.equal(_call(xs, ys, 20, 50, tie_order=tie), got), tie
    fast = _call(xs, ys, 20, 50, fn='dtw', tie_order=2)
    differ = int((fast != got).sum())
    print('pairs where fastdtw (rule 2) and the exact similarity differ: %d' % differ)
    assert differ >= 1
    assert bool((fast <= got).all())                               # fastdtw's path is one of the warp paths


@pytest.mark.parametrize('max_x', [1, 11, 12, 13, 19, 20, 21, 31, 32, 33, 200])
def test_sizes_at_the_instantiation_boundaries_and_beyond(max_x):
    """x rows of every length up to ``max_x`` -- at and around the row counts the register kernel is instantiated for (12,
    20, 32), one past its limit and up to 200 entries through the general kernel -- against y rows of 1, 2, 50, 51 and 300
    entries: every kernel that applies equals the float64 restatement and writes every pair of an output buffer of NaNs."""
    rng = np.random.default_rng(100 + max_x)
    lens = list(range(0, max_x + 1)) if max_x <= 33 else [0, 1, 33, 64, 65, 127, 199, 200]
    lens += [max_x] * 3 + [int(v) for v in rng.integers(0, max_x + 1, 70)]           # more than one wavefront of rows
    xs = [sorted(rng.integers(0, 25, n).tolist()) for n in lens]
    ys = [sorted(rng.integers(0, 40, n).tolist()) for n in (1, 2, 50, 51, 300)]
    ys.append(rng.integers(0, 40, 37).tolist())                                      # one unsorted row
    want = exact_dtw_similarities(xs, ys)
    for kernel in (0, 1):
        got = _raw(xs, ys, max_x, 300, kernel)
        assert not bool(torch.isnan(got).any()), kernel
        assert np.array_equal(got.cpu().numpy(), want), kernel
    assert np.array_equal(_call(xs, ys, max_x, 300).cpu().numpy(), want)
    assert np.array_equal(_call(xs, ys, max_x, 300, order_rows=False).cpu().numpy(), want)


def test_an_empty_y_row_gives_what_the_fastdtw_entry_gives():
    """No patch is ever empty, but the entries accept one: sgnn_dtw_similarity writes PAD for its pairs, and so does the
    exact entry, in both kernels."""
    xs = [[1, 2, 3], [], [4] * 20, list(range(40))]
    ys = [[2, 2], [], [5]]
    for max_x, rows in ((20, xs[:3]), (40, xs)):
        old = _call(rows, ys, max_x, 2, fn='dtw')
        assert float(old[:, 1].abs().max()) == 0.0
        for kernel in (0, 1):
            new = _raw(rows, ys, max_x, 2, kernel)
            assert torch.equal(new[:, 1], old[:, 1]) and not bool(torch.isnan(new).any())
            assert np.array_equal(new.cpu().numpy(), exact_dtw_similarities(rows, ys))


def test_grouping_order_kept_preparation_and_live_range_change_nothing():
    """3000 x rows drawn from 40 distinct ones: grouping repeated rows (which hands the kernel the live range of the
    processing order), ordering the rows, and a kept preparation over three calls whose values change all give the plain call's
    matrix, and that one is the restatement's."""
    ops = _ops()
    rng = np.random.default_rng(77)
    base = [sorted(rng.integers(0, 6, int(rng.integers(0, 21))).tolist()) for _ in range(40)]
    pick = rng.integers(0, 40, 3000)
    ys = [sorted(rng.integers(0, 50, int(rng.integers(1, 51))).tolist()) for _ in range(23)]
    keep, keep_plain = ops.DtwRowPrep(), ops.DtwRowPrep()
    for shift in (0, 3, 1):                                   # same rows repeat each other; other values every call
        xs = [[v + shift for v in base[int(i)]] for i in pick]
        plain = _call(xs, ys, 20, 50, dedupe=False, order_rows=False)
        want_base = exact_dtw_similarities([[v + shift for v in b] for b in base], ys)
        assert np.array_equal(plain.cpu().numpy(), want_base[pick])
        for dedupe in (True, False):
            for order_rows in (True, False):
                assert torch.equal(_call(xs, ys, 20, 50, dedupe=dedupe, order_rows=order_rows), plain), (dedupe, order_rows)
        assert torch.equal(_call(xs, ys, 20, 50, x_prep=keep), plain)
        assert torch.equal(_call(xs, ys, 20, 50, dedupe=False, x_prep=keep_plain), plain)
        assert torch.equal(_call(xs, ys, 20, 50, kernel=1, x_prep=keep), plain)
    assert keep.grouping is not None and keep.grouping.live is not None and keep.grouped_order is not None   # the live-range form ran
    assert keep_plain.order is not None
    # the live-range entry itself: positions [first, first + count) of the order are computed, the rest stays as it was
    from subgnn_amd import _lib
    lib = _lib.load()
    xs = [base[int(i)] for i in pick[:300]]
    X, Y = ops.Ragged.from_lists(xs, DEV), ops.Ragged.from_lists(ys, DEV)
    lens = np.array([len(x) for x in xs])
    order = torch.from_numpy(np.argsort(lens, kind='stable').astype(np.int32)).to(DEV)
    first = int((lens == 0).sum())
    live = torch.tensor([first, len(xs) - first], dtype=torch.int64, device=DEV)
    out = torch.zeros((len(xs), len(ys)), dtype=torch.float32, device=DEV)
    wsb = lib.sgnn_dtw_exact_workspace_bytes(len(xs), 20, len(ys), 50)
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.sgnn_dtw_exact_similarity_live(p(X.ptr), p(X.nodes), len(xs), 20, p(Y.ptr), p(Y.nodes), len(ys), 50, 0, p(order),
                                              p(live), p(out), p(ws), wsb, ops._stream()) == 0
    assert np.array_equal(out.cpu().numpy(), exact_dtw_similarities(xs, ys))
    assert lib.sgnn_dtw_exact_similarity_live(p(X.ptr), p(X.nodes), len(xs), 20, p(Y.ptr), p(Y.nodes), len(ys), 50, 0, None,
                                              p(live), p(out), p(ws), wsb, ops._stream()) == -1       # a range needs its order


def test_calc_dtw_and_the_matrix_form_take_the_function():
    from subgnn_amd import gamma
    x, y = [0, 1, 5, 5, 9], [3, 0, 0, 7, 2, 2, 8]
    want = 1.0 / (FD.exact_dtw(x, y, FD.calc_dist) + 1.0)
    assert gamma.calc_dtw(DEV, x, y, fn=FN) == float(np.float32(want))
    assert gamma.calc_dtw(DEV, [], y, fn=FN) == 1.0
    ops = _ops()
    X, Y = ops.Ragged.from_lists([x, []], DEV), ops.Ragged.from_lists([y], DEV)
    got = gamma.dtw_similarity_matrix(X, X.nodes, Y, Y.nodes, fn=FN)
    assert got.cpu().tolist() == [[float(np.float32(want))], [0.0]]
    with pytest.raises(ValueError):
        gamma.dtw_similarity_matrix(X, X.nodes, Y, Y.nodes, fn='nope')


# ---- through the model ------------------------------------------------------------------------------------------------------

def _models(golden, tmp_path, over=None):
    from test_gpu_hotpath import _models as make
    return make(golden, tmp_path, dict({'structure_similarity_fn': FN}, **(over or {})))


def _restated_slabs(m):
    """(S, C, patches) structure similarities of the train split from the model's own degree sequences."""
    from subgnn_amd import gamma, ops
    S, C, L = m.train_cc_ids.shape
    g = m.networkx_graph
    use_dict = g.full_degree is not None
    out = []
    for internal in (True, False):
        c_sets, c_seq = gamma.degree_sequences(g, m.train_cc_ids.view(S * C, L), internal, use_dict)
        a_sets, a_seq = gamma.degree_sequences(g, m.structure_anchors, internal, use_dict)
        rows = lambda sets, seq: ops.Ragged(sets.ptr, seq).to_lists()
        out.append(exact_dtw_similarities(rows(c_sets, c_seq), rows(a_sets, a_seq)).reshape(S, C, -1))
    return out


@pytest.mark.parametrize('name', ['tiny', 'density'])
def test_dense_and_large_graph_paths_compute_the_exact_similarities(name, tmp_path):
    """hparams['structure_similarity_fn'] = 'dtw_exact' reaches both prepare paths: the dense prepare_data slabs and the
    large-graph pass's slabs are equal to each other and to the restatement, they are not the fastdtw slabs' twins by
    accident of dispatch (the cache files carry the function's name), a second model loads those files, and a training
    step runs."""
    from conftest import load_golden
    from subgnn_amd import hotpath
    golden = load_golden(name)
    dense, sparse = _models(golden, tmp_path)
    assert dense.hparams['structure_similarity_fn'] == FN
    dense.prepare_data()
    hotpath.prepare_sparse(sparse, 'train')
    want_int, want_bor = _restated_slabs(dense)
    for m in (dense, sparse):
        assert np.array_equal(m.train_int_struc_similarities.cpu().numpy(), want_int)
        assert np.array_equal(m.train_bor_struc_similarities.cpu().numpy(), want_bor)
    assert torch.equal(dense.train_int_struc_similarities, sparse.train_int_struc_similarities)
    assert torch.equal(dense.train_bor_struc_similarities, sparse.train_bor_struc_similarities)
    # a second large-graph pass (kept grouping and processing order) gives the same slabs
    hotpath.prepare_sparse(sparse, 'train')
    assert np.array_equal(sparse.train_int_struc_similarities.cpu().numpy(), want_int)
    assert np.array_equal(sparse.train_bor_struc_similarities.cpu().numpy(), want_bor)
    names = sorted(n for n in os.listdir(dense._sim_dir()) if 'struc' in n and n.endswith('similarities.npy'))
    assert names and all('_dtw_exact_' in n for n in names), names
    assert {n.split('_')[0] for n in names} == {'int', 'bor'}
    second = _models(golden, tmp_path, {'compute_similarities': False})[0]
    before = {n: os.path.getmtime(dense._sim_dir() / n) for n in names}
    second.prepare_data()
    assert {n: os.path.getmtime(dense._sim_dir() / n) for n in names} == before          # read, not computed again
    assert torch.equal(second.train_int_struc_similarities, dense.train_int_struc_similarities)
    assert torch.equal(second.train_bor_struc_similarities, dense.train_bor_struc_similarities)
    for m in (dense, sparse):
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        batch = m.make_batch('train', torch.arange(6)) if m is dense else hotpath.full_split_batch(m, 'train')
        out = m.training_step(batch, 0)
        out['loss'].backward()
        opt.step()
        assert torch.isfinite(out['loss'])
        assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_recorded_passes_equal_the_eager_ones(tmp_path):
    """hotpath.GraphedPasses (--graph both) with 'dtw_exact': the preparation, the exact-DTW launches included, is recorded
    into a hipGraph (no host wait inside the capture) and replays to the losses and parameters of the eager schedule."""
    from conftest import load_golden
    from subgnn_amd import hotpath, optim
    golden = load_golden('density')
    seq, cap = _models(golden, tmp_path, {'lin_dropout': 0.0, 'lstm_dropout': 0.0})
    cap.load_state_dict(seq.state_dict())
    seq.train(); cap.train()
    lr, clip = 0.01, 0.5
    o_seq = optim.ClipAdam(seq.parameters(), lr, max_norm=clip)
    o_cap = optim.ClipAdam(cap.parameters(), lr, max_norm=clip, capturable=True)
    want = []
    for k in range(6):
        hotpath.prepare_sparse(seq, 'train')
        out = seq.training_step(hotpath.full_split_batch(seq, 'train'), 0)
        out['loss'].backward()
        o_seq.step()
        o_seq.zero_grad(set_to_none=True)
        want.append(float(out['loss'].detach()))
    passes = hotpath.GraphedPasses(cap, o_cap, 'train', warmup=2)
    got = [float(passes.step()[0]) for _ in range(6)]
    torch.cuda.synchronize()
    assert passes.recordings == 2 and all(s is not None for s in passes.slots)
    assert got == want
    for (n1, a), (_, b) in zip(seq.named_parameters(), cap.named_parameters()):
        assert torch.equal(a, b), n1


def test_other_similarity_functions_are_still_not_implemented(tmp_path):
    from conftest import load_golden
    dense = _models(load_golden('tiny'), tmp_path, {'structure_similarity_fn': 'edit_distance'})[0]
    with pytest.raises(NotImplementedError):
        dense.compute_structure_patch_similarities(None, tmp_path / 'x.npy', True, torch.zeros((1, 1, 1), dtype=torch.int64, device=DEV))
    with pytest.raises(NotImplementedError):
        dense.prepare_data()


def test_train_config_trains_a_model_with_the_exact_function(tiny, tmp_path):
    """The reference-format driver on a written dataset: hyperparams.json and a restored run carry the value, the similarity
    cache is written under the function's name, the loss falls."""
    from test_gpu_train_driver import CONFIG
    from subgnn_amd import config, train_config
    write_dataset_from_golden(tiny, tmp_path, 'ds')
    fix = dict(tiny.hp)
    for k in ('batch_size', 'learning_rate', 'n_layers'):
        fix.pop(k, None)
    fix.update({'max_epochs': 6, 'seed': 3, 'lin_dropout': 0.0, 'compute_similarities': True, 'structure_similarity_fn': FN})
    cfg = tmp_path / 'config.json'
    cfg.write_text(CONFIG % json.dumps(fix))
    config.PROJECT_ROOT = tmp_path
    rc = train_config.read_json(cfg)
    best, model, trainer = train_config.train_model(rc, results_dir=tmp_path / 'results', log=lambda *a: None, checkpoint_k=1)
    assert model.hparams['structure_similarity_fn'] == FN and len(model.metric_scores) == 6
    h = trainer.history
    assert all(np.isfinite(e['train_loss']) for e in h) and h[-1]['train_loss'] < h[0]['train_loss']
    assert json.loads((tmp_path / 'results' / 'hyperparams.json').read_text())['structure_similarity_fn'] == FN
    names = set(os.listdir(tmp_path / 'ds' / 'similarities'))
    assert any(n.startswith('int_struc_') and '_dtw_exact_train' in n for n in names), names
    assert not any(n.startswith('int_struc_') and n.endswith('_0_train_similarities.npy') for n in names)   # no fastdtw file
    ck = trainer.best_checkpoint_path()
    assert ck is not None
    _, again, _ = train_config.train_model(rc, restore_path=tmp_path / 'results', restore_name=os.path.basename(str(ck)),
                                           no_train=True, log=lambda *a: None)
    assert again.hparams['structure_similarity_fn'] == FN
    assert torch.equal(again.train_int_struc_similarities, model.train_int_struc_similarities)

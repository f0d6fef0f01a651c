"""CPU: what class-weighted losses (hparams['class_weight'] / ['pos_weight']) add below the GPU tests -- the
hyper-parameter forms and 'balanced', the C ABI entries, the state_dict, the built kernels' registers, the route a loss module
takes through a training step, the hyperparams.json round trip, and the refusal of a multi-rank run."""
import json
import math
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
from torch import nn

from helpers import write_dataset_from_golden
import weighted_loss_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import kernel_resources as KR                                      # noqa: E402

LIBDIR = os.path.join(REPO, 'subgnn_amd', 'lib')

# The bare kernels as the parent commit built them (tools/kernel_resources.py on its head.o / loss.o):
# pattern -> (VGPRs, spilled VGPRs, spilled SGPRs).  The bare launches must stay the code they were: none may use more.
PARENT = {
    'head_fwd_kernel(': (71, 0, 38), 'head_fwd_ml_kernel(': (71, 0, 18),
    'head_bwd_kernel<1>': (97, 0, 31), 'head_bwd_kernel<2>': (127, 0, 42), 'head_bwd_kernel<4>': (161, 0, 36),
    'head_bwd_ml_kernel<1>': (97, 0, 25), 'head_bwd_ml_kernel<2>': (127, 0, 51), 'head_bwd_ml_kernel<4>': (163, 0, 31),
    'ce_fwd_kernel(': (15, 0, 0), 'ce_finish_kernel(': (16, 0, 0), 'ce_bwd_kernel(': (13, 0, 0),
    'bce_fwd_kernel(': (26, 0, 0), 'bce_finish_kernel(': (12, 0, 0), 'bce_bwd_kernel(': (14, 0, 0),
}


# ---- hyper-parameter forms ------------------------------------------------------------------------------------------------------------

def test_balanced_class_weight_is_sklearns():
    from sklearn.utils.class_weight import compute_class_weight
    from subgnn_amd import loss_weights as LW
    y = torch.tensor([0, 0, 0, 0, 0, 1, 1, 2, 3, 3, 3, 0, 2, 2, 2, 2])
    got = LW.resolve('balanced', 'class_weight', 4, False, labels=y)
    want = compute_class_weight('balanced', classes=np.arange(4), y=y.numpy())
    assert np.allclose(got, want, rtol=1e-12, atol=0), (got, want)
    counts, N = LW.class_counts(y, 4)
    assert counts.tolist() == [6, 2, 5, 3] and N == 16
    assert got == [16 / (4 * 6), 16 / (4 * 2), 16 / (4 * 5), 16 / (4 * 3)]


def test_balanced_pos_weight_and_absent_classes():
    from subgnn_amd import loss_weights as LW
    rows = [[0], [0, 2], [2], [0], [1, 2], [0], [2, 0]]             # n = [5, 1, 4, 0] of N = 7
    got = LW.resolve('balanced', 'pos_weight', 4, True, labels=rows)
    assert got == [(7 - 5) / 5, (7 - 1) / 1, (7 - 4) / 4, 1.0]
    # an absent class gets 1.0 in the single-label form too, and ignored rows are not counted
    y = torch.tensor([0, 0, 2, -100, 2, 0])
    assert LW.resolve('balanced', 'class_weight', 4, False, labels=y) == [5 / (4 * 3), 1.0, 5 / (4 * 2), 1.0]


def test_list_and_dict_forms_and_what_is_refused():
    from subgnn_amd import loss_weights as LW
    assert LW.resolve(None, 'class_weight', 3, False) is None
    assert LW.resolve([1, 2.5, 0], 'class_weight', 3, False) == [1.0, 2.5, 0.0]
    assert LW.resolve((1, 2, 3), 'pos_weight', 3, True) == [1.0, 2.0, 3.0]
    assert LW.resolve(np.array([1.0, 2.0]), 'class_weight', 2, True) == [1.0, 2.0]
    # a dict names classes by their label strings; missing labels get 1
    assert LW.resolve({'b': 4, 'c': 0.5}, 'class_weight', 3, False, names=['a', 'b', 'c']) == [1.0, 4.0, 0.5]
    assert LW.resolve({1: 3}, 'pos_weight', 3, True) == [1.0, 3.0, 1.0]            # without names: the class indices
    for bad in ([1, 2], [1, 2, 3, 4], [1, -0.5, 1], [1, float('nan'), 1], [1, float('inf'), 1], [1, 'x', 1], [1, True, 1], 'uniform',
                3.0, {'zz': 2}):
        with pytest.raises(ValueError):
            LW.resolve(bad, 'class_weight', 3, False, names=['a', 'b', 'c'])
    with pytest.raises(ValueError):
        LW.resolve('balanced', 'class_weight', 3, True, labels=[[0], [1, 2]])       # no balanced per-column weight
    with pytest.raises(ValueError):
        LW.resolve([1, 1, 1], 'pos_weight', 3, False)                               # pos_weight is multi-label only
    with pytest.raises(ValueError):
        LW.resolve('balanced', 'class_weight', 3, False)                            # no labels to count


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------

def _header():
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    decl = {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'\b(sgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', bare)}
    return txt, decl


def test_abi_entries_are_declared_mirrored_exported_and_refuse_nulls():
    from subgnn_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    txt, decl = _header()
    assert '#define SGNN_ABI_VERSION 14' in txt and lib.sgnn_abi_version() == 14
    for name in C.NEW_ENTRIES:
        base = name[:-len('_weighted')]
        assert name in decl and base in decl, name
        extra = 2 if ('_ml_' in name or '_bce_' in name) else 1
        # the existing argument list plus the weight rows at the end, as const float*
        assert decl[name][:-extra] == decl[base], name
        assert all(a.startswith('const float*') for a in decl[name][-extra:]), decl[name][-extra:]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl[name]), name
        assert _lib.SIGNATURES[name][1][:-extra] == _lib.SIGNATURES[base][1], name
        assert hasattr(lib, name), name
    assert 'SubGNN.py:133' in txt[txt.index('sgnn_cross_entropy_fwd_weighted') - 2500:txt.index('sgnn_cross_entropy_fwd_weighted')]
    assert 'SubGNN.py:133' in txt[txt.index('int sgnn_head_fwd_weighted') - 1500:txt.index('int sgnn_head_fwd_weighted')]
    # the existing entries keep their signatures
    assert (len(decl['sgnn_head_fwd']), len(decl['sgnn_head_bwd']), len(decl['sgnn_head_fwd_ml']), len(decl['sgnn_head_bwd_ml'])) \
        == (20, 18, 19, 17)
    assert (len(decl['sgnn_cross_entropy_fwd']), len(decl['sgnn_cross_entropy_bwd']), len(decl['sgnn_bce_logits_fwd']),
            len(decl['sgnn_bce_logits_bwd'])) == (10, 8, 9, 7)
    # null required pointers: -1 (SGNN_ERR_BAD_ARG) on the host, before any launch -- this runs without a device
    assert lib.sgnn_cross_entropy_fwd_weighted(None, None, 1, 1, None, None, None, None, 0, None, None) == -1
    assert lib.sgnn_cross_entropy_bwd_weighted(None, None, None, None, 1, 1, None, None, None) == -1
    assert lib.sgnn_bce_logits_fwd_weighted(None, None, 1, 1, None, None, None, 0, None, None, None) == -1
    assert lib.sgnn_bce_logits_bwd_weighted(None, None, None, 1, 1, None, None, None, None) == -1
    assert lib.sgnn_head_fwd_weighted(None, 1, 1, 1, 1, None, None, None, None, None, 0.0, None, None, None, None, None, None, None, 0,
                                      None, None) == -1
    assert lib.sgnn_head_bwd_weighted(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, 0.0, None, None, None,
                                      None) == -1
    assert lib.sgnn_head_fwd_ml_weighted(None, 1, 1, 1, 1, None, None, None, None, None, 0.0, None, None, None, None, None, None, 0, None,
                                         None, None) == -1
    assert lib.sgnn_head_bwd_ml_weighted(None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, 0.0, None, None, None, None,
                                         None) == -1


def test_ops_check_the_weight_rows_on_the_host():
    from subgnn_amd import ops
    x, y = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    for bad in (torch.ones(4), torch.ones(3, dtype=torch.float64), torch.ones(1, 3), [1.0, 1.0, 1.0], torch.ones(3)):
        with pytest.raises(ValueError):                        # wrong length, dtype, rank, type -- and a host tensor: not on a device
            ops.cross_entropy_with_accuracy(x, y, weight=bad)
        with pytest.raises(ValueError):
            ops.bce_with_logits_and_accuracy(x, torch.zeros(2, 3, dtype=torch.int64), pos_weight=bad)
    lin = [nn.Linear(4, 3), nn.Linear(3, 2), nn.Linear(2, 3)]
    with pytest.raises(ValueError):
        ops.fused_head(torch.zeros(2, 4), lin[0], lin[1], lin[2], labels=y, pos_weight=torch.ones(3))     # pos_weight: targets only
    with pytest.raises(ValueError):
        ops.fused_head(torch.zeros(2, 4), lin[0], lin[1], lin[2], labels=y, class_weight=torch.ones(2))


# ---- kernels --------------------------------------------------------------------------------------------------------------------------

def _kernels():
    from subgnn_amd import build
    build.build(verbose=False)
    return [k for f in ('head.o', 'loss.o') for k in KR.kernels(os.path.join(LIBDIR, f))]


def test_weighted_kernels_neither_spill_vectors_nor_use_scratch():
    ks = _kernels()
    for pattern in C.WEIGHTED_KERNELS:
        hits = [k for k in ks if pattern in k['demangled']]
        assert hits, pattern
        for k in hits:
            print('%-60s vgpr %3d  vspill %d  sspill %2d  scratch %d' % (k['demangled'][:60], k['vgpr_count'], k['vgpr_spill_count'],
                                                                         k['sgpr_spill_count'], k['private_segment_fixed_size']))
            assert k['vgpr_spill_count'] == 0, (k['demangled'], k['vgpr_spill_count'])
            assert k['private_segment_fixed_size'] == 0, (k['demangled'], k['private_segment_fixed_size'])
            # kernels of their own, outside the name patterns tests/test_kernel_resources.py ratchets
            assert 'head_fwd_kernel' not in k['demangled'] and 'head_bwd_kernel<' not in k['demangled']


def test_bare_kernels_use_no_more_registers_than_the_parent_commits():
    ks = _kernels()
    for pattern, (vgprs, vspill, sspill) in PARENT.items():
        # ('void ' leads a template instantiation's demangled name; 'ce_fwd_kernel(' also ends 'bce_fwd_kernel(')
        hits = [k for k in ks if k['demangled'].replace('void ', '', 1).startswith(pattern)]
        assert len(hits) == 1, (pattern, [k['demangled'] for k in hits])
        k = hits[0]
        print('%-40s vgpr %3d (parent %3d)  vspill %d (%d)  sspill %2d (%2d)' % (pattern, k['vgpr_count'], vgprs, k['vgpr_spill_count'],
                                                                                 vspill, k['sgpr_spill_count'], sspill))
        assert k['vgpr_count'] <= vgprs, (pattern, k['vgpr_count'], vgprs)
        assert k['vgpr_spill_count'] <= vspill, (pattern, k['vgpr_spill_count'], vspill)
        assert k['sgpr_spill_count'] <= sspill, (pattern, k['sgpr_spill_count'], sspill)


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------

def test_route_reaches_every_path_and_every_refusal():
    from subgnn_amd import loss_weights as LW
    seen = set()
    for what, make, hp, ml, head_ok, want in C.route_cases():
        got = LW.route(make(), hp, ml, 3, head_ok)
        assert got == want, (what, got, want)
        seen.add(got)
    assert seen == {'fused_head', 'standalone', 'library'}
    # the three non-default settings are refused one by one, whatever else is default
    for kw in ({'reduction': 'sum'}, {'ignore_index': 1}, {'label_smoothing': 0.1}):
        assert LW.kernel_plan(nn.CrossEntropyLoss(**kw), False, 3) is None, kw
    # a plan carries the module's own rows: the kernels and the module apply the same weights
    w = torch.tensor([1.0, 2.0, 0.5])
    plan = LW.kernel_plan(nn.CrossEntropyLoss(weight=w), False, 3)
    assert plan[0] is not None and torch.equal(plan[0], w) and plan[1] is None
    assert LW.kernel_plan(nn.CrossEntropyLoss(), False, 3) == (None, None)
    plan = LW.kernel_plan(nn.BCEWithLogitsLoss(pos_weight=w), True, 3)
    assert plan[0] is None and torch.equal(plan[1], w)
    # rows on another device than the step's tensors: the library
    assert LW.kernel_plan(nn.CrossEntropyLoss(weight=w), False, 3, device='meta') is None


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


def test_model_builds_its_loss_from_the_hyper_parameters_and_keeps_its_state_dict(tiny, tmp_path):
    from subgnn_amd import loss_weights as LW
    bare = _model(tiny, tmp_path)
    assert type(bare.loss) is nn.CrossEntropyLoss and bare.loss.weight is None
    K = bare.num_classes
    bal = _model(tiny, tmp_path, class_weight='balanced')
    counts, N = LW.class_counts(bal.train_sub_G_label, K)
    want = [N / (K * n) if n else 1.0 for n in counts.tolist()]
    assert type(bal.loss) is nn.CrossEntropyLoss and bal.loss.weight.dtype == torch.float32
    assert bal.loss.weight.device == bal.lin3.weight.device
    assert torch.equal(bal.loss.weight.cpu(), torch.tensor(want, dtype=torch.float32))
    assert bal.hparams['class_weight'] == 'balanced'                  # the hyper-parameter keeps its configured form
    lst = _model(tiny, tmp_path, class_weight=[0.5] + [2.0] * (K - 1))
    assert lst.loss.weight.tolist() == [0.5] + [2.0] * (K - 1)
    # a dict names classes by the label strings of subgraphs.pth (numbered in order of first appearance)
    from subgnn_amd.subgraph_utils import label_names
    names = label_names(os.path.join(str(tmp_path), 'ds', 'subgraphs.pth'))
    dct = _model(tiny, tmp_path, class_weight={names[-1]: 3.0})
    assert dct.loss.weight.tolist() == [1.0] * (K - 1) + [3.0]
    for bad in ([1.0] * (K + 1), [-1.0] + [1.0] * (K - 1), [float('nan')] + [1.0] * (K - 1), {'no such label': 1.0}):
        with pytest.raises(ValueError):
            _model(tiny, tmp_path, class_weight=bad)
    with pytest.raises(ValueError):
        _model(tiny, tmp_path, pos_weight='balanced')                 # a single-label dataset has no pos_weight
    # the weights are no state: the keys are equal, and a checkpoint loads both ways
    assert list(bal.state_dict().keys()) == list(bare.state_dict().keys())
    assert not any(k.startswith('loss') for k in bal.state_dict())
    sd_bare = {k: v.clone() for k, v in bare.state_dict().items()}
    sd_bal = {k: v.clone() for k, v in bal.state_dict().items()}
    bal.load_state_dict(sd_bare)                                      # strict
    bare.load_state_dict(sd_bal)
    assert torch.equal(bal.loss.weight.cpu(), torch.tensor(want, dtype=torch.float32))      # loading did not touch the weights
    assert bare.loss.weight is None
    # val_test_outputs takes device tensors or host copies: the weights follow the logits
    g = torch.Generator().manual_seed(1)
    logits, labels = torch.randn(6, K, generator=g), torch.randint(0, K, (6,), generator=g)
    out = bal.val_test_outputs('val', logits, labels)
    ref = torch.nn.functional.cross_entropy(logits, labels, weight=torch.tensor(want, dtype=torch.float32))
    assert abs(float(out['val_loss']) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))


def test_balanced_round_trips_through_hyperparams_json(tiny, tmp_path):
    """A config with "class_weight": "balanced" -> get_hyperparams -> hyperparams.json (as train_model writes it) -> the
    hyper-parameters a restored run reads: the same word, and a model built from them carries the same weights."""
    from test_gpu_train_driver import CONFIG
    from subgnn_amd import config, train_config
    write_dataset_from_golden(tiny, tmp_path, 'ds')
    fix = dict(tiny.hp)
    for k in ('batch_size', 'learning_rate', 'n_layers'):
        fix.pop(k, None)
    fix.update({'max_epochs': 1, 'seed': 3, 'class_weight': 'balanced'})
    (tmp_path / 'config.json').write_text(CONFIG % json.dumps(fix))
    config.PROJECT_ROOT = tmp_path
    rc = train_config.read_json(tmp_path / 'config.json')
    model, hp = train_config.build_model(rc, train_config.FixedTrial())
    assert hp['class_weight'] == 'balanced' and model.loss.weight is not None
    train_config.write_hyperparams(tmp_path / 'results', hp)
    back = json.loads((tmp_path / 'results' / 'hyperparams.json').read_text())
    assert back['class_weight'] == 'balanced' and 'pos_weight' not in back
    again, hp2 = train_config.build_model(rc, hp=back)
    assert torch.equal(again.loss.weight, model.loss.weight)
    assert list(again.state_dict().keys()) == list(model.state_dict().keys())
    # a list survives as a list, and a choice of forms is an ordinary hyperparams_optuna entry
    rc['hyperparams_optuna']['class_weight'] = {'type': 'suggest_categorical', 'args': [[None, 'balanced']]}
    assert train_config.get_hyperparams(rc, train_config.FixedTrial({'class_weight': 'balanced'}))['class_weight'] == 'balanced'
    assert train_config.get_hyperparams(rc, train_config.FixedTrial())['class_weight'] is None


# ---- more than one rank ---------------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, root, hp, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['HIP_VISIBLE_DEVICES'] = ''                       # a host-side refusal: no rank opens a device
    os.environ['CUDA_VISIBLE_DEVICES'] = ''
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from subgnn_amd import config
    from subgnn_amd.SubGNN import SubGNN, dataset_paths
    config.PROJECT_ROOT = root
    res = {}
    for what, over in (('bare', {}), ('class_weight', {'class_weight': 'balanced'}), ('list', {'class_weight': [1.0] * hp.pop('_K')})):
        try:
            SubGNN(dict(hp, **over), **dataset_paths('ds'))
            res[what] = 'built'
        except RuntimeError as e:
            res[what] = 'refused: %s' % e
    q.put((rank, res))
    dist.destroy_process_group()


def test_a_weighted_model_under_two_ranks_is_refused(tiny, tmp_path):
    """Per-rank weighted means averaged over ranks are not the global weighted mean: constructing a model with loss weights under
    an initialised 2-rank group (gloo, CPU) raises; a bare model is built as before."""
    import torch.multiprocessing as mp
    write_dataset_from_golden(tiny, tmp_path, 'ds')
    from subgnn_amd.subgraph_utils import label_names
    K = len(label_names(os.path.join(str(tmp_path), 'ds', 'subgraphs.pth')))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, tmp_path, dict(tiny.hp, _K=K), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, r in res:
        assert r['bare'] == 'built', r
        assert r['class_weight'].startswith('refused') and 'multi-rank' in r['class_weight'], r
        assert r['list'].startswith('refused'), r


def test_a_single_process_is_not_a_multi_rank_run():
    from subgnn_amd import loss_weights as LW
    LW.refuse_multi_rank(LW.make_loss(False, [1.0, 2.0]))          # no process group: nothing to refuse
    loss = LW.make_loss(True, [1.0, 2.0], [3.0, 4.0])
    assert type(loss) is nn.BCEWithLogitsLoss and loss.weight.tolist() == [1.0, 2.0] and loss.pos_weight.tolist() == [3.0, 4.0]
    assert list(loss.state_dict().keys()) == [] and math.isclose(float(loss(torch.zeros(1, 2), torch.ones(1, 2))),
                                                                 (3.0 * 1.0 + 4.0 * 2.0) * math.log(2.0) / 2, rel_tol=1e-6)

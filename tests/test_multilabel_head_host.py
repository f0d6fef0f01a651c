"""CPU: what the multi-label head (HPO-NEURO: nn.BCEWithLogitsLoss + exact-match accuracy) adds below the GPU tests -- the C ABI
entries, the kernels in the built code objects, the hpo_neuro stand-in's preset and label column, and the argument check of
ops.fused_head."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import kernel_resources as KR                                      # noqa: E402

LIBDIR = os.path.join(REPO, 'subgnn_amd', 'lib')
NEW_ENTRIES = ('sgnn_head_fwd_ml', 'sgnn_head_bwd_ml', 'sgnn_bce_logits_workspace_bytes', 'sgnn_bce_logits_fwd', 'sgnn_bce_logits_bwd')
NEW_KERNELS = ('head_fwd_ml_kernel', 'head_bwd_ml_kernel<1>', 'head_bwd_ml_kernel<2>', 'head_bwd_ml_kernel<4>', 'bce_fwd_kernel',
               'bce_finish_kernel', 'bce_bwd_kernel')


def _header_arg_counts():
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return {m.group(1): (0 if m.group(2).strip() in ('', 'void') else m.group(2).count(',') + 1)
            for m in re.finditer(r'\b(sgnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', txt)}


def test_new_entries_are_declared_mirrored_and_exported():
    from subgnn_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    declared = _header_arg_counts()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == declared[name], (name, len(_lib.SIGNATURES[name][1]), declared[name])
        assert hasattr(lib, name), name
    # the existing head entries keep their signatures
    assert declared['sgnn_head_fwd'] == 20 and declared['sgnn_head_bwd'] == 18
    assert lib.sgnn_bce_logits_workspace_bytes(1000) >= 2 * 4 * 4 and lib.sgnn_bce_logits_workspace_bytes(-1) == -1
    assert lib.sgnn_bce_logits_fwd(None, None, 1, 1, None, None, None, 0, None) == -1
    assert lib.sgnn_head_fwd_ml(None, 1, 1, 1, 1, None, None, None, None, None, 0.0, None, None, None, None, None, None, 0, None) == -1


def test_new_kernels_are_in_the_code_objects_without_spills_or_scratch():
    from subgnn_amd import build
    build.build(verbose=False)
    ks = [k for f in ('head.o', 'loss.o') for k in KR.kernels(os.path.join(LIBDIR, f))]
    for pattern in NEW_KERNELS:
        hits = [k for k in ks if pattern in k['demangled']]
        assert hits, pattern
        for k in hits:
            assert k['vgpr_spill_count'] == 0, (k['demangled'], k['vgpr_spill_count'])
            assert k['private_segment_fixed_size'] == 0, (k['demangled'], k['private_segment_fixed_size'])
    # the multi-label instantiations are kernels of their own: the single-label ones keep their names (and their budgets in
    # tests/test_kernel_resources.py)
    assert [k for k in ks if k['demangled'].startswith('head_fwd_kernel(')]
    assert [k for k in ks if 'head_bwd_kernel<1>' in k['demangled']]


def test_hpo_neuro_preset_and_its_label_column(tmp_path):
    from subgnn_amd import standins, subgraph_utils
    P = standins.PRESETS['hpo_neuro']
    metab = standins.PRESETS['hpo_metab']
    assert (P['n'], P['m'], P['n_classes']) == (metab['n'], metab['m'], 10)
    hp = P['hp']
    assert hp['use_structure'] and not hp['use_neighborhood'] and not hp['use_position']
    assert (hp['n_layers'], hp['batch_size'], hp['linear_hidden_dim_1'], hp['linear_hidden_dim_2']) == (5, 128, 64, 64)
    assert hp['n_anchor_patches_structure'] == 43
    assert abs(hp['lin_dropout'] - 0.214) < 1e-3 and abs(hp['lstm_dropout'] - 0.0867) < 1e-4
    labs = standins.neuro_labels(90, 10)
    assert len(labs) == 90
    pairs = [l for l in labs if '-' in l]
    singles = [l for l in labs if '-' not in l]
    assert len(pairs) == 30 and all('-' in labs[i] for i in range(0, 90, 3)) and singles
    for l in pairs:
        a, b = l.split('-')
        assert a != b
    assert {int(c) for l in labs for c in l.split('-')} == set(range(10))
    # su:24-92 reads them into lists of class indices
    f = tmp_path / 'subgraphs.pth'
    f.write_text(''.join('%d-%d\t%s\t%s\t\n' % (3 * i, 3 * i + 1, l, 'train' if i < 60 else ('val' if i < 75 else 'test'))
                         for i, l in enumerate(labs)))
    tr, tr_lab, va, va_lab, te, te_lab = subgraph_utils.read_subgraphs(str(f))
    assert isinstance(tr_lab, list) and len(tr_lab) == 60 == len(tr)
    assert sorted({len(l) for l in tr_lab}) == [1, 2]
    assert {c for l in tr_lab + va_lab + te_lab for c in l} == set(range(10))


def test_fused_head_refuses_labels_and_targets_together():
    import torch
    from subgnn_amd import ops
    lin = [torch.nn.Linear(4, 3), torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)]
    with pytest.raises(ValueError):
        ops.fused_head(torch.zeros(2, 4), lin[0], lin[1], lin[2], labels=torch.zeros(2, dtype=torch.int64),
                       targets=torch.zeros(2, 2, dtype=torch.int64))
    assert hasattr(ops, 'bce_with_logits_and_accuracy')

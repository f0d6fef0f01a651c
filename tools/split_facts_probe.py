"""What a split's kept facts cost in device memory at the benchmark's size (hotpath.SplitFacts + the DTW row sides' kept
values), and that passes from them equal recomputed passes there.  usage: python tools/split_facts_probe.py [bench.py options]
-> one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import bench                                                             # noqa: E402


def main():
    args = bench.parse()
    from subgnn_amd import hotpath, ops
    from subgnn_amd.SubGNN import SubGNN
    dev = torch.device('cuda', 0)
    rowptr, col, subs, total, _ = bench.build_inputs(args, 0, 1)
    g = ops.DeviceGraph(rowptr, col, np.arange(1, args.nodes + 1, dtype=np.int32), dev)
    torch.manual_seed(0)
    emb = torch.randn(args.nodes, args.embed, device=dev)
    labels = torch.randint(0, 3, (total,), generator=torch.Generator().manual_seed(0))
    models = []
    for keep in (True, False):
        hp = dict(bench.ALL_DENSITY_HP, node_embed_size=args.embed, keep_split_facts=keep)
        models.append(SubGNN.from_memory(hp, g, {'train': subs, 'val': [], 'test': []},
                                         {'train': labels, 'val': labels[:0], 'test': labels[:0]}, emb, num_classes=3))
    kept_m, off_m = models
    equal = True
    for k in range(4):
        a, b = hotpath.prepare_pass(kept_m, 'train'), hotpath.prepare_pass(off_m, 'train')
        torch.cuda.synchronize()
        for nm in ('train_cc_ids', 'train_int_struc_similarities', 'train_bor_struc_similarities'):
            equal = equal and torch.equal(a.attrs[nm], b.attrs[nm])
        for l, t in a.per_split['anchors_neigh_border'].items():
            equal = equal and torch.equal(t, b.per_split['anchors_neigh_border'][l])
        hotpath.install_pass(kept_m, a)
        hotpath.install_pass(off_m, b)
    facts = kept_m.__dict__['_split_facts']['train']
    rec = facts.dtw_rows
    facts_bytes, dtw_bytes = hotpath.split_facts_bytes(kept_m, 'train')
    each = {nm: t.numel() * t.element_size() for nm, t in (
        ('cc_ids', facts.cc_ids), ('cc_ids._sgnn_ids32', facts.cc_ids._sgnn_ids32), ('cc_ids._sgnn_mask_u8', facts.cc_ids._sgnn_mask_u8),
        ('real', facts.real), ('cc_sets.ptr', facts.cc_sets.ptr), ('has_pad_c', facts.has_pad_c), ('cc_canon.nodes', facts.cc_canon.nodes),
        ('ci', facts.ci), ('ce', facts.ce))}
    sides = {name: {'grouped': bool(s.group), 'rows_bytes': s.prep.rows.nbytes if s.prep.rows is not None else 0,
                    'grouped_val_bytes': s.prep.grouped_val.numel() * 4 if s.prep.grouped_val is not None else 0}
             for name, s in (('internal', rec.internal), ('external', rec.external))}
    print(json.dumps({'subgraphs': len(subs), 'cc_ids_shape': list(facts.cc_ids.shape), 'facts_bytes': facts_bytes,
                      'facts_tensors_bytes': each, 'dtw_row_sides_bytes': dtw_bytes, 'dtw_row_sides': sides,
                      'kept_bytes_per_split': facts_bytes + dtw_bytes, 'passes_equal_recomputed': bool(equal)}))


if __name__ == '__main__':
    main()

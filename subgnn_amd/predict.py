"""Labels and embeddings for subgraphs that are NOT rows of ``subgraphs.pth``, from a trained model.

Everything the splits' preparation ties to a split is tied to the request's CONTENT here, so that a prediction is a function
of the model and the node set and of nothing else -- not of where the subgraph stands in the request, nor of what else the
request holds:

  * every node list becomes the ascending set of its nodes, so its components (by smallest member) and their member order are the set's;
  * the tape item of every neighbourhood / position draw is a 64-bit key of the drawing set's content (ops.set_keys:
    sgnn_set_keys) in place of the row number, under the split code ``tape.SPLIT_CODE['predict']``;
  * the PAD rule compares a row with the widths of the TRAINING matrices, frozen once (a request row is one more row of the
    matrix the model was trained on), never with the other rows of the request;
  * the shared anchors (position-external anchors, structure patches, their walks and the layers' picks) are the model's own,
    as restored; the position-external similarities are read from hop tables of those anchors built once (ops.bfs_hops), so a
    request runs no search over the graph for them.

A subgraph's draws here are not the draws it would get as a row of the test split (the tape items differ by design); their
distribution is the same.

    python -m subgnn_amd.predict -config_path CONFIG -restoreModelPath DIR [-restoreModelName F] -subgraphs FILE -out FILE
                                 [-embeddings FILE.npy] [-batch_size B]
"""
import argparse
import json
from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch

from . import checkpoint, cli, config, gamma, hotpath, ops, subgraph_utils, tape

SPLIT = 'predict'


class Predictor:
    """Owns a prepared, trained model (``train_cc_ids`` and the shared anchors exist: ``prepare_data`` or
    ``hotpath.prepare_sparse(model, 'train')`` ran).  ``label_names``: the label strings by class index, if known."""

    def __init__(self, model, label_names=None):
        if getattr(model, 'train_cc_ids', None) is None:
            raise ValueError('Predictor needs a prepared model (prepare_data / hotpath.prepare_sparse)')
        self.model = model
        self.label_names = list(label_names) if label_names is not None else None
        self._frozen = None

    @classmethod
    def from_run(cls, run_config, restore_path, restore_name=None):
        """The model of a finished run: hyper-parameters from ``restore_path/hyperparams.json``, weights from ``restore_name``
        (default: the best ``epoch*.ckpt`` by the config's monitored metric, else ``last.ckpt``), anchors restored as
        ``train_model(..., no_train=True)`` restores them (prepare_data, then the checkpoint's resample epoch)."""
        from .train_config import build_model
        restore_path = Path(restore_path)
        hp = json.loads((restore_path / 'hyperparams.json').read_text(), object_pairs_hook=OrderedDict)
        model, hp = build_model(run_config, hp=hp)
        if restore_name is None:
            opt_cfg = run_config.get('optuna', {})
            mode = 'max' if opt_cfg.get('opt_direction', 'maximize') == 'maximize' else 'min'
            restore_name = checkpoint.best_checkpoint(restore_path, opt_cfg.get('monitor_metric', 'val_micro_f1'), mode)
            if restore_name is None:
                restore_name = checkpoint.LAST
        model.prepare_data()
        checkpoint.load_checkpoint(model, restore_path / restore_name)
        names = subgraph_utils.label_names(Path(config.PROJECT_ROOT) / model.subgraph_path)
        p = cls(model, names)
        p.restored_from = restore_name
        return p

    # ------------------------------------------------------------------ frozen, once -----
    def freeze(self):
        """What every request reads of the model and the training split, computed once: the training matrices' padded widths,
        the hop tables of the position-external anchors, the structure patches' degree sequences."""
        if self._frozen is not None:
            return self._frozen
        m = self.model
        hp, g, dev = m.hparams, m.networkx_graph, m.device
        f = {'epoch': int(m.__dict__.get('_resample_epoch', 0)), 'seed': int(hp.get('seed', 0)) & tape.MASK64}
        tcc = m.train_cc_ids.to(dev)
        f['cc_len'] = int(tcc.shape[2])
        f['degree'] = (g.rowptr[1:] - g.rowptr[:-1]).cpu().numpy()          # degree by id (row 0: PAD)
        if hp['use_neighborhood']:
            # the width of the training split's padded border matrix: its largest border (aps:190 pads every row to it)
            sets = ops.Ragged.from_padded(tcc.reshape(-1, tcc.shape[2]))
            f['border_width'] = int(ops.khop_border(g, sets, hp['neigh_sample_border_size']).lengths.max().item())
        if hp['use_position']:
            cap = hp.get('max_bfs_hops', 32)
            f['pos_ext'] = {l: a.to(dev) for l, a in m.anchors_pos_ext.items()}
            f['hop_tables'] = {l: ops.bfs_hops(g, a.to(torch.int32).contiguous(), max_hops=cap, node_major=True)
                               for l, a in f['pos_ext'].items()}
        if hp['use_structure']:
            if hp['structure_similarity_fn'] not in ops.DTW_FNS:
                raise NotImplementedError(hp['structure_similarity_fn'])
            a_sets = ops.Ragged.from_padded(m.structure_anchors.to(dev))
            ai, ae = ops.degree_sequence(g, a_sets, sort=True, use_degree_dict=g.full_degree is not None)
            f['patches'] = (a_sets, ai, ae)
            f['anchors_structure'] = m.anchors_structure
        self._frozen = f
        return f

    # ------------------------------------------------------------------ a request --------
    def map_subgraphs(self, subgraphs, allow_empty=False):
        """Node lists in the dataset's numbering -> the model's (read_data: id + 1), as sets: without the ids that are no nodes
        of the graph (beyond its ids, or without an edge: what subgraph_properties drops), without repeats, ascending ->
        (ptr int64[n + 1], ids int32[total]) numpy arrays.  A list with nothing left is an error naming its index (or, with
        ``allow_empty``, an empty set)."""
        import itertools
        deg = self.freeze()['degree']
        max_id = deg.shape[0] - 1
        n = len(subgraphs)
        lens = np.fromiter(map(len, subgraphs), dtype=np.int64, count=n)
        flat = np.fromiter(itertools.chain.from_iterable(subgraphs), dtype=np.int64, count=int(lens.sum())) + 1
        rows = np.repeat(np.arange(n, dtype=np.int64), lens)
        ok = (flat >= 1) & (flat <= max_id)
        ok[ok] = deg[flat[ok]] > 0
        flat, rows = flat[ok], rows[ok]
        order = np.lexsort((flat, rows))
        flat, rows = flat[order], rows[order]
        first = np.ones(flat.shape[0], dtype=bool)
        first[1:] = (flat[1:] != flat[:-1]) | (rows[1:] != rows[:-1])
        flat, rows = flat[first], rows[first]
        counts = np.bincount(rows, minlength=n)
        if n and not allow_empty and int(counts.min()) == 0:
            raise ValueError('subgraph %d holds no node of the graph' % int(np.argmin(counts != 0)))
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=ptr[1:])
        return ptr, flat.astype(np.int32)

    def request_sets(self, subgraphs):
        """``map_subgraphs`` on the device: the request as an ops.Ragged of ascending sets (what ``prepare_sets`` takes)."""
        if len(subgraphs) == 0:
            raise ValueError('no subgraphs')
        ptr, flat = self.map_subgraphs(subgraphs)
        dev = self.model.device
        return ops.Ragged(torch.from_numpy(ptr).to(dev), torch.from_numpy(flat).to(dev), max_len=int((ptr[1:] - ptr[:-1]).max()))

    def prepare(self, subgraphs):
        """Components, anchors and similarities of the request, installed on the model as split 'predict' ->
        hotpath.PassState (``attrs`` / ``per_split`` hold them by the names forward reads; ``subgraphs``: the mapped node sets, ascending)."""
        return self.prepare_sets(self.request_sets(subgraphs))

    def prepare_sets(self, sets, epoch_offset=0, want_lists=True, sub_keys=None):
        """``prepare`` behind the mapping: ``sets`` is a device ops.Ragged of non-empty ascending sets of model ids without repeats
        (``request_sets``; ``ops.occlusion_sets`` of one).  ``want_lists=False`` leaves ``st.subgraphs`` None: the sets stay on
        the device.  ``sub_keys``: the sets' ``ops.set_keys``, where the caller holds them.

        ``epoch_offset=d`` is draw d of the request: the neighbourhood anchors (internal and border) and the position-internal
        anchors are drawn from the streams of resample epoch ``epoch + d``, so draw 0 is ``prepare``'s answer and every draw is
        keyed by content as that one is.  The model's own shared anchors are NOT redrawn: the position-external anchors, the
        structure patches and the layers' picks of them stay as restored, whatever the draw (they belong to the trained model,
        not to the request)."""
        f = self.freeze()
        m = self.model
        hp, g, dev = m.hparams, m.networkx_graph, m.device
        seed, ep, L = f['seed'], f['epoch'] + int(epoch_offset), hp['n_layers']
        if sets.n == 0:
            raise ValueError('no subgraphs')

        def stream(kind, l):
            return tape.stream_id(kind, SPLIT, l, ep)

        st = hotpath.PassState(SPLIT)
        st.subgraphs = sets.to_lists() if want_lists else None
        subs = sets
        labels = ops.cc_labels(g, subs)
        cc_ids = subgraph_utils.components_from_labels(subs.ptr, subs.nodes, labels, subs.max_len)
        S, C, Lc = cc_ids.shape
        cc_ids._sgnn_ids32 = cc_ids.reshape(-1).to(torch.int32)
        real = cc_ids[:, :, 0] != 0
        cc_ids._sgnn_mask, cc_ids._sgnn_mask_u8 = real, real.reshape(-1).to(torch.uint8)
        st.attrs[SPLIT + '_cc_ids'] = cc_ids
        cc_sets = ops.sort_ragged(ops.Ragged.from_padded(cc_ids.reshape(S * C, Lc)))
        cc_keys = ops.set_keys(cc_sets)
        if sub_keys is None:
            sub_keys = ops.set_keys(subs)
        st.keys = {'components': cc_keys.view(S, C), 'subgraphs': sub_keys}
        sims = {}
        if hp['use_neighborhood']:
            A_in, A_out = hp['n_anchor_patches_N_in'], hp['n_anchor_patches_N_out']
            has_pad_c = (cc_sets.lengths < f['cc_len']).to(torch.uint8)
            border, hops = ops.khop_border(g, cc_sets, hp['neigh_sample_border_size'], want_hops=True)
            border, hops = ops.sort_ragged(border, extra=hops)
            has_pad_b = (border.lengths < f['border_width']).to(torch.uint8)
            ni, nb = {}, {}
            for l in range(L):
                ni[l] = ops.sample_anchors_ragged_keyed(cc_sets, cc_keys, has_pad_c, A_in, seed,
                                                        stream(tape.STREAM_N_INT, l)).view(S, C, -1)
                sims[('N', 'in', l)] = ops.ZeroSims(ni[l].shape, dev)
                a, w = ops.draw_border_anchors_keyed(border, hops.contiguous(), cc_keys, has_pad_b, A_out, seed,
                                                     stream(tape.STREAM_N_BOR, l))
                nb[l], sims[('N', 'out', l)] = a.view(S, C, -1), w.view(S, C, -1).contiguous()
            st.per_split['anchors_neigh_int'], st.per_split['anchors_neigh_border'] = ni, nb
            st.per_split['_mpn_edge_plans'] = {}
        if hp['use_position']:
            cap = hp.get('max_bfs_hops', 32)
            pint = {l: ops.choice_ragged_keyed(subs, sub_keys, hp['n_anchor_patches_pos_in'], seed, stream(tape.STREAM_P_INT, l))
                    for l in range(L)}
            st.per_split['anchors_pos_int'] = pint
            for l in range(L):
                sims[('P', 'out', l)] = ops.min_hops_to_sets(f['hop_tables'][l], cc_sets, node_major=True).view(S, C, -1).contiguous()
                if C == 1:
                    sims[('P', 'in', l)] = ops.ZeroSims((S, C, hp['n_anchor_patches_pos_in']), dev)
                    continue
                # as hotpath.prepare_pass: hops from the distinct drawn anchors, reduced over every component's members
                uniq, inv = torch.unique(pint[l], return_inverse=True)
                if uniq.numel() * (g.max_id + 1) <= hotpath.MAX_PINT_BYTES:
                    d = ops.bfs_hops(g, uniq.to(torch.int32).contiguous(), max_hops=cap, node_major=True)
                    full = ops.min_hops_to_sets(d, cc_sets, node_major=True).view(S, C, -1)
                    w = torch.gather(full, 2, inv.view(S, 1, -1).expand(S, C, -1))
                else:
                    w = hotpath._pint_sims_streamed(g, uniq, inv, cc_sets, S, C, cap)
                sims[('P', 'in', l)] = (w * real.unsqueeze(-1)).contiguous()
        if hp['use_structure']:
            a_sets, ai, ae = f['patches']
            ci, ce = ops.degree_sequence(g, cc_sets, sort=True, use_degree_dict=g.full_degree is not None)
            fn, tie = hp['structure_similarity_fn'], hp['dtw_tie_order']
            for name, x, y in (('_int', ci, ai), ('_bor', ce, ae)):
                st.attrs[SPLIT + name + '_struc_similarities'] = gamma.dtw_similarity_matrix(cc_sets, x, a_sets, y, tie, fn=fn).view(S, C, -1)
        else:
            st.attrs[SPLIT + '_int_struc_similarities'] = st.attrs[SPLIT + '_bor_struc_similarities'] = None
        st.attrs[SPLIT + '_neigh_pos_similarities'] = sims if sims else None
        st.attrs[SPLIT + '_N_border'] = None
        # install_pass marks the model as prepared by sparse passes (a resample would then re-prepare train / val that way):
        # a request is no preparation of the model's own splits, so the mark stays what it was
        mark = m.__dict__.get('_sparse_prepared')
        hotpath.install_pass(m, st)
        if mark is None:
            m.__dict__.pop('_sparse_prepared', None)
        else:
            m.__dict__['_sparse_prepared'] = mark
        return st

    def _batch(self, st, lo, hi):
        m = self.model
        cc = st.attrs[SPLIT + '_cc_ids']
        S = cc.shape[0]
        if lo == 0 and hi == S:
            pick, idx = (lambda t: t), hotpath._whole_split_index(m, S)
        else:
            sel = torch.arange(lo, hi, device=m.device)
            pick, idx = (lambda t: None if t is None else t.index_select(0, sel)), sel.view(-1, 1)
        np_sim = st.attrs[SPLIT + '_neigh_pos_similarities']
        return {'subgraph_ids': None, 'cc_ids': pick(cc), 'N_border': None,
                'NP_sim': None if np_sim is None else {k: pick(v) for k, v in np_sim.items()},
                'I_S_sim': pick(st.attrs[SPLIT + '_int_struc_similarities']),
                'B_S_sim': pick(st.attrs[SPLIT + '_bor_struc_similarities']), 'subgraph_idx': idx, 'label': None}

    def forward_prepared(self, st, batch_size=None):
        """Forward over an installed request in chunks of ``batch_size`` -> (logits (R, K), embeddings (R, H): the head's input)."""
        m = self.model
        S = st.attrs[SPLIT + '_cc_ids'].shape[0]
        bs = S if not batch_size else int(batch_size)
        was_training = m.training
        m.eval()
        kept = m.__dict__['_head_inputs'] = []
        try:
            with torch.no_grad():
                logits = [m._forward_batch(SPLIT, self._batch(st, lo, min(lo + bs, S))) for lo in range(0, S, bs)]
        finally:
            m.__dict__.pop('_head_inputs', None)
            m.train(was_training)
        return torch.cat(logits, 0), torch.cat(kept, 0)

    def _probabilities(self, logits):
        return torch.sigmoid(logits) if self.model.multilabel else torch.softmax(logits, dim=-1)

    def predict(self, subgraphs, batch_size=None, return_embeddings=False, draws=1):
        """-> dict: ``logits`` (R, K) float32, ``probabilities`` (softmax; sigmoid for a multi-label model), ``labels`` (argmax
        (R,) int64; for a multi-label model the (R, K) bool of the float32 expression sigmoid(x) > 0.5, as the fused head
        evaluates it), ``subgraphs`` (the mapped node sets: model ids, ascending) and, on request, ``embeddings`` (R, H).  ``batch_size`` only chunks
        the forward pass.  ``draws=E > 1`` adds ``logits_mean``, ``logits_std`` (the sample standard deviation) and
        ``probabilities_mean`` over draws 0 .. E - 1 of the request's own anchors (``prepare_sets``: ``epoch_offset``); everything
        else stays draw 0's."""
        return self._predict_sets(self.request_sets(subgraphs), batch_size, return_embeddings, draws)[0]

    def _predict_sets(self, sets, batch_size, return_embeddings, draws):
        """``predict`` on device sets -> (its dict, the float32 logits of every draw (E, R, K))."""
        if batch_size is not None and int(batch_size) <= 0:
            raise ValueError('batch_size must be positive')
        if int(draws) != draws or int(draws) <= 0:
            raise ValueError('draws must be a positive integer')
        st = self.prepare_sets(sets)
        logits, emb = self.forward_prepared(st, batch_size)
        logits = logits.float()
        if self.model.multilabel:
            prob = torch.sigmoid(logits)
            labels = prob > 0.5
        else:
            prob = torch.softmax(logits, dim=-1)
            labels = logits.argmax(dim=-1)
        out = {'logits': logits, 'probabilities': prob, 'labels': labels, 'subgraphs': st.subgraphs}
        if return_embeddings:
            out['embeddings'] = emb
        per_draw = torch.stack([logits] + [self.draw_logits(sets, d, batch_size) for d in range(1, int(draws))])
        if draws > 1:
            out['logits_mean'], out['logits_std'] = per_draw.mean(dim=0), per_draw.std(dim=0, unbiased=True)
            out['probabilities_mean'] = self._probabilities(per_draw).mean(dim=0)
        return out, per_draw

    def draw_logits(self, sets, draw, batch_size=None, sub_keys=None):
        """The float32 logits of device sets at draw ``draw`` (``prepare_sets`` + ``forward_prepared``; no Python lists)."""
        st = self.prepare_sets(sets, epoch_offset=draw, want_lists=False, sub_keys=sub_keys)
        return self.forward_prepared(st, batch_size)[0].float()

    def explain(self, subgraphs, unit='node', target=None, draws=1, batch_size=None, max_variants=65536):
        """Leave-one-out attribution of every request over its nodes or components: ``explain.explain``."""
        from . import explain as _explain
        return _explain.explain(self, subgraphs, unit=unit, target=target, draws=draws, batch_size=batch_size,
                                max_variants=max_variants)

    def suggest(self, subgraphs, candidates='border', hops=1, target=None, draws=1, batch_size=None, max_variants=65536):
        """The gain of every node each request could be given (its border, or a shared pool of ids): ``suggest.suggest``."""
        from . import suggest as _suggest
        return _suggest.suggest(self, subgraphs, candidates=candidates, hops=hops, target=target, draws=draws,
                                batch_size=batch_size, max_variants=max_variants)

    def grow(self, subgraphs, steps, target=None, min_gain=0.0, candidates='border', hops=1, draws=1, batch_size=None):
        """Greedy growth: every request takes its best candidate, round by round, while it gains: ``suggest.grow``."""
        from . import suggest as _suggest
        return _suggest.grow(self, subgraphs, steps, target=target, min_gain=min_gain, candidates=candidates, hops=hops,
                             draws=draws, batch_size=batch_size)

    def discover(self, seeds, sizes=(8,), per_seed=16, target=None, restart=0.15, max_steps=None, draws=1, top=100,
                 top_per_seed=None, novel=False, batch_size=None, max_variants=65536, sample_seed=None, max_overlap=None,
                 overlap_pool=4096):
        """Connected candidate subgraphs sampled around seed nodes on the device, scored and ranked: ``discover.discover``."""
        from . import discover as _discover
        return _discover.discover(self, seeds, sizes=sizes, per_seed=per_seed, target=target, restart=restart, max_steps=max_steps,
                                  draws=draws, top=top, top_per_seed=top_per_seed, novel=novel, batch_size=batch_size,
                                  max_variants=max_variants, sample_seed=sample_seed, max_overlap=max_overlap,
                                  overlap_pool=overlap_pool)

    def nearest(self, index, subgraphs, k=10):
        """The ``k`` rows of ``index`` (a neighbors.SubgraphIndex) nearest to each requested subgraph: ``index.query``."""
        return index.query(self, subgraphs, k)

    def names_of(self, labels_row):
        """The label strings of one row of ``labels``."""
        name = (lambda k: self.label_names[k]) if self.label_names is not None else str
        if self.model.multilabel:
            return [name(k) for k, on in enumerate(labels_row.tolist()) if on]
        return [name(int(labels_row))]


# ---------------------------------------------------------------------- files, CLI --------
def read_requests(path):
    """One subgraph per line in the first column's format of ``subgraphs.pth`` (``n1-n2-...``; further tab-separated columns
    are ignored, blank lines skipped) -> list of node lists."""
    out = []
    with open(path) as fin:
        for line in fin:
            first = line.split('\t')[0].strip()
            if first:
                out.append([int(n) for n in first.split('-') if n != ''])
    return out


def format_line(nodes, label_strings, probabilities):
    """``n1-n2-...\\tlabel[-label]\\tp_1,...,p_K`` (9 significant digits: a float32 survives the round trip)."""
    return '%s\t%s\t%s' % ('-'.join(str(int(n)) for n in nodes), '-'.join(label_strings),
                           ','.join('%.9g' % float(p) for p in probabilities))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Predict labels (and embeddings) of subgraphs outside the dataset from a checkpoint')
    cli.add_run_arguments(ap)
    ap.add_argument('-subgraphs', type=str, required=True, help='one subgraph per line: n1-n2-... (further columns ignored)')
    ap.add_argument('-out', type=str, required=True, help='text file: n1-n2-...<TAB>label[-label]<TAB>p_1,...,p_K per request')
    ap.add_argument('-embeddings', type=str, default=None, help='write the (R, H) subgraph embeddings to this .npy file')
    ap.add_argument('-batch_size', type=int, default=None, help='chunk the forward pass (default: one batch)')
    args = ap.parse_args(argv)
    cli.require_positive(ap, args, ('batch_size',))
    if args.embeddings is not None and not args.embeddings.endswith('.npy'):
        ap.error('-embeddings takes a .npy file name')
    if args.out == args.subgraphs or (args.embeddings is not None and args.embeddings in (args.out, args.subgraphs)):
        ap.error('-subgraphs, -out and -embeddings must be different files')
    return args


def main(argv=None):
    args = parse_args(argv)
    requests = read_requests(args.subgraphs)
    p = cli.open_predictor(args)
    res = p.predict(requests, batch_size=args.batch_size, return_embeddings=args.embeddings is not None)
    prob, labels = res['probabilities'].cpu().numpy(), res['labels'].cpu()
    cli.write_lines(args.out, (format_line([n - 1 for n in nodes], p.names_of(labels[i]), prob[i])
                               for i, nodes in enumerate(res['subgraphs'])))
    if args.embeddings is not None:
        np.save(args.embeddings, res['embeddings'].cpu().numpy())
    return res


if __name__ == '__main__':
    main()

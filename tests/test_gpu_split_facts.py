"""-m gpu: a split's kept facts (hotpath.SplitFacts: components, component sets, their sorted form and degree sequences, and
behind them the DTW launches' prepared x side).  A pass that takes them equals a pass that recomputes them, bit for bit; a
steady pass does not recompute; another list, count or split never reads them.  "Equal" is torch.equal throughout."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_NODES, N_TRAIN, N_VAL = 2000, 96, 24

_CASE = {}


def _n_components(sub, rowptr, col):
    """Connected components of the subgraph induced by ``sub`` (1-based ids), on the host."""
    parent = {v: v for v in sub}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for v in sub:
        for w in col[rowptr[v]:rowptr[v + 1]]:
            if int(w) in parent:
                parent[find(v)] = find(int(w))
    return len({find(v) for v in sub})


def _case():
    """BA graph (2 000 nodes, m = 3); subgraph lists of 4-12 nodes: breadth-first ones, twelve per list made of two or three
    disconnected pieces (C > 1, padded component rows), one single node.  Built once per process."""
    if _CASE:
        return _CASE
    from subgnn_amd import synthetic
    rowptr, col = synthetic.sorted_csr(synthetic.barabasi_albert_edges(N_NODES, 3, seed=11), N_NODES)

    def lists(count, seed):
        rng = np.random.default_rng(seed)
        out, tries = [], 0
        while len(out) < count:
            i, tries = len(out), tries + 1
            if i % 8 == 3:                                   # pieces far apart in id: checked to be disconnected below
                n_pieces = 2 + (i // 8) % 2
                sub = []
                for p in range(n_pieces):
                    piece = synthetic.bfs_subgraphs(rowptr, col, 1, int(rng.integers(2, 5)), seed=seed * 1000 + tries * 7 + p)[0]
                    sub += [v for v in piece if v not in sub]
                if _n_components(sub, rowptr, col) < 2 or not 4 <= len(sub) <= 12:
                    continue
            elif i == 5:
                sub = [int(rng.integers(1, N_NODES + 1))]
            else:
                sub = synthetic.bfs_subgraphs(rowptr, col, 1, 4 + i % 9, seed=seed * 1000 + tries)[0]
                if len(sub) < 4:
                    continue
            out.append([int(v) for v in sub])
        return out
    train, other, val = lists(N_TRAIN, 1), lists(N_TRAIN, 2), lists(N_VAL, 3)
    assert sum(_n_components(s, rowptr, col) > 1 for s in train) >= 10 and any(len(s) == 1 for s in train)
    assert train != other
    connected = [s for s in train if _n_components(s, rowptr, col) == 1]
    _CASE.update(rowptr=rowptr, col=col, train=train, other=other, val=val, connected=connected)
    return _CASE


def _model(train=None, keep=True, over=None, capturable=None):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
    from bench import ALL_DENSITY_HP
    from subgnn_amd import ops, optim
    from subgnn_amd.SubGNN import SubGNN
    c = _case()
    train = list(c['train'] if train is None else train)
    g = ops.DeviceGraph(c['rowptr'], c['col'], np.arange(1, N_NODES + 1, dtype=np.int32), DEV)
    hp = dict(ALL_DENSITY_HP, lin_dropout=0.0, lstm_dropout=0.0, keep_split_facts=keep)
    hp.update(over or {})
    assert hp['use_neighborhood'] and hp['use_structure'] and hp['use_position']
    emb = torch.randn(N_NODES, hp['node_embed_size'], generator=torch.Generator().manual_seed(0)).to(DEV)
    labels = torch.randint(0, 3, (max(len(train), N_VAL),), generator=torch.Generator().manual_seed(0))
    torch.manual_seed(0)
    m = SubGNN.from_memory(hp, g, {'train': train, 'val': list(c['val']), 'test': []},
                           {'train': labels[:len(train)], 'val': labels[:N_VAL], 'test': labels[:0]}, emb, num_classes=3)
    m.train()
    if capturable is None:
        return m
    return m, optim.ClipAdam(m.parameters(), hp['learning_rate'], max_norm=hp['grad_clip'], capturable=capturable)


def _same(x, y, where=''):
    if isinstance(x, torch.Tensor):
        assert isinstance(y, torch.Tensor) and torch.equal(x, y), where
    elif isinstance(x, dict):
        assert set(x) == set(y), where
        for k in x:
            _same(x[k], y[k], '%s/%s' % (where, k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), where
        for i, (p, q) in enumerate(zip(x, y)):
            _same(p, q, '%s/%d' % (where, i))
    elif hasattr(x, 'dense'):
        _same(x.dense(), y.dense(), where)
    elif isinstance(x, np.ndarray):
        assert np.array_equal(x, y), where
    else:
        assert x == y, where


def _same_pass(a, b, where):
    torch.cuda.synchronize()
    assert set(a.attrs) == set(b.attrs) and set(a.per_split) == set(b.per_split), where
    _same(a.attrs, b.attrs, where + ' attrs')
    _same(a.per_split, b.per_split, where + ' per_split')
    for nm in ('_int_struc_similarities', '_bor_struc_similarities'):
        assert a.attrs[a.split + nm] is not None
    for nm in ('_sgnn_ids32', '_sgnn_mask', '_sgnn_mask_u8'):
        cc_a, cc_b = a.attrs[a.split + '_cc_ids'], b.attrs[b.split + '_cc_ids']
        assert torch.equal(getattr(cc_a, nm), getattr(cc_b, nm)), where + nm


@pytest.mark.parametrize('variant', ['same epoch', 'resample epochs', 'dtw_exact'])
def test_passes_from_kept_facts_equal_recomputed_passes(variant):
    from subgnn_amd import hotpath
    over = {'structure_similarity_fn': 'dtw_exact'} if variant == 'dtw_exact' else {}
    kept_m, off_m = _model(keep=True, over=over), _model(keep=False, over=over)
    draws, facts = [], None
    for k in range(3):
        if variant == 'resample epochs':                    # resample_anchor_patches: the draws change, the facts do not
            for m in (kept_m, off_m):
                m.__dict__['_resample_epoch'] = k
        a, b = hotpath.prepare_pass(kept_m, 'train'), hotpath.prepare_pass(off_m, 'train')
        _same_pass(a, b, '%s, pass %d' % (variant, k))
        cc = a.attrs['train_cc_ids']
        assert cc.shape[0] == N_TRAIN and cc.shape[1] > 1 and bool((cc[:, 1:, 0] == 0).any())       # C > 1, padded rows
        now = kept_m.__dict__['_split_facts']['train']
        assert (facts is None or now is facts) and cc is now.cc_ids and now.sub_g is kept_m.train_sub_G
        off = off_m.__dict__['_split_facts']['train']            # its record holds none of the component tensors
        assert a.x_fixed and not b.x_fixed and off.tensors() == [] and off.nbytes == 0
        assert all(getattr(off, nm) is None for nm in ('cc_ids', 'cc_sets', 'real', 'has_pad_c', 'cc_canon', 'ci', 'ce'))
        facts = now
        draws.append(a.per_split['anchors_neigh_border'][0].clone())
        hotpath.install_pass(kept_m, a)
        hotpath.install_pass(off_m, b)
    assert facts.ci is not None and facts.cc_canon is not None and facts.nbytes > 0
    if variant == 'resample epochs':
        assert not torch.equal(draws[0], draws[1]) and not torch.equal(draws[1], draws[2])
    else:
        assert torch.equal(draws[0], draws[2])
    # the prepared x side of the DTW launches was built once the preparations settled, and is the one the last pass used
    rec = facts.dtw_rows
    assert all(s.prep.rows is not None and s.prep.fixed_src is f for s, f in ((rec.internal, facts.ci), (rec.external, facts.ce)))
    assert all(s.prep.rows is None for s in (lambda r: (r.internal, r.external))(off_m.__dict__['_split_facts']['train'].dtw_rows))
    # what readers outside hotpath see of the records (the benchmark's rooflines): dictionaries of the earlier shapes
    rows, k = facts.cc_sets.n, kept_m.hparams['neigh_sample_border_size']
    for m in (kept_m, off_m):
        r = m.__dict__['_split_facts']['train']
        assert list(m._degseq_order) == ['train'] and m._degseq_order['train'] is r.set_order and r.set_order.numel() == rows
        assert list(m._border_width) == [('train', k, rows, 1)] and m._border_width[('train', k, rows, 1)] is r.border_width[k]


def _counted(monkeypatch):
    from subgnn_amd import ops
    calls = {'cc_labels': 0, 'degree_sequence': 0}
    real_cc, real_ds = ops.cc_labels, ops.degree_sequence

    def cc_labels(*a, **k):
        calls['cc_labels'] += 1
        return real_cc(*a, **k)

    def degree_sequence(*a, **k):
        calls['degree_sequence'] += 1
        return real_ds(*a, **k)
    monkeypatch.setattr(ops, 'cc_labels', cc_labels)
    monkeypatch.setattr(ops, 'degree_sequence', degree_sequence)

    def take():
        got = (calls['cc_labels'], calls['degree_sequence'])
        calls['cc_labels'] = calls['degree_sequence'] = 0
        return got
    return take


def test_a_steady_pass_does_not_recompute(monkeypatch):
    from subgnn_amd import hotpath
    take = _counted(monkeypatch)
    kept_m, off_m = _model(keep=True), _model(keep=False)
    for m, want_first, want_steady in ((kept_m, (1, 2), (0, 1)), (off_m, (1, 2), (1, 2))):
        for k in range(3):
            timer = hotpath.StageTimer(True)
            hotpath.install_pass(m, hotpath.prepare_pass(m, 'train', timer))
            assert take() == (want_first if k == 0 else want_steady), (m is kept_m, k)
            names = [n for n, _ in timer.marks]
            if m is off_m:
                assert 'components' in names and 'degree_sequences' in names
            elif k == 0:                                     # the first pass says what it did once
                assert 'components(first pass only)' in names and 'degree_sequences(first pass only)' in names
            else:
                assert not any(n.startswith(('components', 'degree_sequences')) for n in names), names
    torch.cuda.synchronize()


def test_another_list_count_or_split_never_reads_kept_facts(monkeypatch):
    from subgnn_amd import hotpath
    c = _case()
    take = _counted(monkeypatch)
    m = _model(keep=True)
    hotpath.install_pass(m, hotpath.prepare_pass(m, 'train'))
    hotpath.install_pass(m, hotpath.prepare_pass(m, 'train'))
    first = m.__dict__['_split_facts']['train']
    assert first.sub_g is m.train_sub_G
    take()
    # the same count, other members: a new list object
    m.train_sub_G = list(c['other'])
    st = hotpath.prepare_pass(m, 'train')
    assert take() == (1, 2)
    second = m.__dict__['_split_facts']['train']
    assert second is not first and second.sub_g is m.train_sub_G and first.sub_g is not m.train_sub_G
    assert st.attrs['train_cc_ids'] is second.cc_ids and st.attrs['train_cc_ids'] is not first.cc_ids
    assert not first.matches(m.train_sub_G, len(m.train_sub_G), m.networkx_graph, None)
    fresh = _model(train=c['other'], keep=False)
    _same_pass(st, hotpath.prepare_pass(fresh, 'train'), 'other members')
    st = hotpath.prepare_pass(m, 'train')                    # ... and its steady pass, from the new facts
    assert take()[0] == 1 and m.__dict__['_split_facts']['train'] is second          # (1: the fresh model's pass above)
    _same_pass(st, hotpath.prepare_pass(fresh, 'train'), 'other members, steady')
    take()
    # another count
    m.train_sub_G = list(c['other'][:50])
    st = hotpath.prepare_pass(m, 'train')
    assert take() == (1, 2)
    third = m.__dict__['_split_facts']['train']
    assert third is not second and third.n == 50 and st.attrs['train_cc_ids'].shape[0] == 50
    _same_pass(st, hotpath.prepare_pass(_model(train=c['other'][:50], keep=False), 'train'), 'another count')
    take()
    # a list that grew in place is not the list the facts were made from either
    m.train_sub_G.append(list(c['other'][50]))
    st = hotpath.prepare_pass(m, 'train')
    assert take() == (1, 2) and m.__dict__['_split_facts']['train'] is not third and st.attrs['train_cc_ids'].shape[0] == 51
    # val and train keep separate facts
    train_facts = m.__dict__['_split_facts']['train']
    sv = hotpath.prepare_pass(m, 'val')
    val_facts = m.__dict__['_split_facts']['val']
    assert val_facts is not train_facts and val_facts.sub_g is m.val_sub_G and sv.attrs['val_cc_ids'].shape[0] == N_VAL
    assert m.__dict__['_split_facts']['train'] is train_facts
    take()
    hotpath.prepare_pass(m, 'val')
    hotpath.prepare_pass(m, 'train')
    assert take() == (0, 2) and m.__dict__['_split_facts']['val'] is val_facts and m.__dict__['_split_facts']['train'] is train_facts
    # forgotten facts are computed again
    hotpath.forget_split_facts(m, 'train')
    assert 'train' not in m.__dict__['_split_facts'] and m.__dict__['_split_facts']['val'] is val_facts
    st = hotpath.prepare_pass(m, 'train')
    assert take() == (1, 2) and m.__dict__['_split_facts']['train'] is not train_facts
    assert st.attrs['train_cc_ids'] is not train_facts.cc_ids and torch.equal(st.attrs['train_cc_ids'], train_facts.cc_ids)
    hotpath.forget_split_facts(m)
    assert not m.__dict__['_split_facts']
    torch.cuda.synchronize()


@pytest.mark.parametrize('deterministic', [False, True])
def test_lists_edited_in_place_are_read_again_once_forgotten(deterministic):
    """A change the record's key cannot see -- some of the split's lists overwritten in place: same list object, same length --
    followed by forget_split_facts: the next pass is the pass of a fresh model on the edited lists (device lists uploaded
    again, components, kept border, widths and orders computed again), not the pass the old record would have served."""
    from subgnn_amd import hotpath
    c = _case()
    m = _model(keep=True)
    m._deterministic = deterministic
    for _ in range(2):
        before = hotpath.prepare_pass(m, 'train')
        hotpath.install_pass(m, before)
    lists = m.train_sub_G
    for i in (1, 3, 4, 11, 40):                              # (3 and 11: lists of several disconnected pieces)
        assert lists[i] != c['other'][i]
        lists[i] = list(c['other'][i])
    assert m.train_sub_G is lists and len(lists) == N_TRAIN
    hotpath.forget_split_facts(m, 'train')
    after = hotpath.prepare_pass(m, 'train')
    fresh = _model(train=lists, keep=False)
    fresh._deterministic = deterministic
    _same_pass(after, hotpath.prepare_pass(fresh, 'train'), 'edited in place, then forgotten')
    # ... and not because the edit changed nothing
    cc0, cc1 = before.attrs['train_cc_ids'], after.attrs['train_cc_ids']
    assert cc0.shape != cc1.shape or not torch.equal(cc0, cc1)
    nb0, nb1 = before.per_split['anchors_neigh_border'], after.per_split['anchors_neigh_border']
    assert any(nb0[l].shape != nb1[l].shape or not torch.equal(nb0[l], nb1[l]) for l in nb0)


def test_facts_built_on_one_stream_serve_a_pass_on_another():
    from subgnn_amd import hotpath
    kept_m, off_m = _model(keep=True), _model(keep=False)
    want = hotpath.prepare_pass(off_m, 'train')
    torch.cuda.synchronize()
    second = torch.cuda.Stream()
    with torch.cuda.stream(second):
        a = hotpath.prepare_pass(kept_m, 'train')            # builds the facts on the second stream
    b = hotpath.prepare_pass(kept_m, 'train')                # (no synchronisation in between: the facts' event orders it)
    _same_pass(a, want, 'built on the second stream')
    _same_pass(b, want, 'read on the first stream')


def _eager_losses(m, opt, steps):
    from subgnn_amd import hotpath
    out = []
    for _ in range(steps):
        hotpath.prepare_sparse(m, 'train')
        res = m.training_step(hotpath.full_split_batch(m, 'train'), 0)
        res['loss'].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        out.append(float(res['loss']))
    return out


def test_recorded_training_half_trains_like_the_eager_schedule():
    """hotpath.CapturedTraining under PassPipeline (two passes in flight) on the model of the tests above: the kept tensors
    are what the recording reads; install_pass_static finds them in place."""
    from subgnn_amd import hotpath
    (seq, o_seq), (cap, o_cap) = _model(keep=False, capturable=False), _model(keep=True, capturable=True)
    cap.load_state_dict(seq.state_dict())
    want = _eager_losses(seq, o_seq, 4)
    trainer = hotpath.CapturedTraining(cap, o_cap, 'train', warmup=1)
    pipe = hotpath.PassPipeline(cap, 'train')
    pipe.start()
    pipe.start()
    got = []
    for _ in range(4):
        pipe.install(installer=trainer.install)
        ev = torch.cuda.Event()
        ev.record()
        loss, _ = trainer.step()
        pipe.start(after=ev)
        got.append(float(loss))
    torch.cuda.synchronize()
    assert trainer.recordings == 1, trainer.last_changed
    assert cap.train_cc_ids is cap.__dict__['_split_facts']['train'].cc_ids
    assert got == want
    for (name, a), (_, b) in zip(seq.named_parameters(), cap.named_parameters()):
        assert torch.equal(a, b), name


def test_recorded_passes_train_like_the_eager_schedule():
    """hotpath.GraphedPasses (the preparation recorded too) over the CONNECTED subgraphs of the same lists: a pass over
    multi-component subgraphs reads the distinct P-internal anchors back (torch.unique) and no preparation with a host round
    trip can be recorded, with or without kept facts.  Two eager passes build the facts, then a recording per slot, then two
    replays."""
    from subgnn_amd import hotpath
    c = _case()
    (seq, o_seq), (cap, o_cap) = (_model(train=c['connected'], keep=False, capturable=False),
                                  _model(train=c['connected'], keep=True, capturable=True))
    cap.load_state_dict(seq.state_dict())
    want = _eager_losses(seq, o_seq, 6)
    passes = hotpath.GraphedPasses(cap, o_cap, 'train', warmup=2)
    got = []
    for _ in range(6):
        loss, _ = passes.step()
        got.append(float(loss))
    torch.cuda.synchronize()
    assert passes.recordings == 2
    facts = cap.__dict__['_split_facts']['train']
    assert all(s.state.attrs['train_cc_ids'] is facts.cc_ids and s.state.x_fixed for s in passes.slots)
    assert got == want
    for (name, a), (_, b) in zip(seq.named_parameters(), cap.named_parameters()):
        assert torch.equal(a, b), name

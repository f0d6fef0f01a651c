"""CPU: what decides whether kept values may be read -- the key of hotpath.SplitFacts, ops.DtwRowPrep.fit and the header
checks of the DTW ``_rows`` entries -- needs no device."""
import ctypes
import types

import pytest
import torch


def _facts(sub_g, graph, shard=None):
    from subgnn_amd import hotpath
    cc = torch.zeros((len(sub_g), 1, 2), dtype=torch.int64)
    return hotpath.SplitFacts(sub_g, len(sub_g), graph, shard, cc, None, cc[:, :, 0] != 0)


_FIELDS = ('subs', 'dims', 'member_order', 'set_order', 'dtw_rows', 'cc_ids', 'cc_sets', 'real', 'has_pad_c', 'cc_canon', 'ci', 'ce')


def _filled(m, split, sub_g, graph, shard=None):
    """The split's record as a pass gets it, every field a sentinel of its own."""
    from subgnn_amd import hotpath
    rec = hotpath._split_record(m, split, sub_g, graph, shard)
    for nm in _FIELDS:
        setattr(rec, nm, (split, nm))
    rec.dims = (3, 7)
    rec.border_width, rec.borders = {1: (split, 'width')}, {(1, 4 << 30): (split, 'border'), (1, 1): None}
    return rec


def test_facts_are_those_of_one_list_object_count_graph_and_shard():
    from subgnn_amd import hotpath
    g, g2 = object(), object()
    subs = [[1, 2], [3]]
    f = _facts(subs, g)
    assert f.ready is None                                            # host tensors: nothing to order
    assert f.matches(subs, 2, g, None)
    assert not f.matches(list(subs), 2, g, None)                      # an equal list is another list
    assert not f.matches(subs, 2, g2, None)
    assert not f.matches(subs, 1, g, None)
    sh = types.SimpleNamespace(start=0, world=2)
    assert not f.matches(subs, 2, g, sh)
    fs = _facts(subs, g, sh)
    assert fs.matches(subs, 2, g, types.SimpleNamespace(start=0, world=2))
    assert not fs.matches(subs, 2, g, types.SimpleNamespace(start=1, world=2))
    assert not fs.matches(subs, 2, g, types.SimpleNamespace(start=0, world=4))
    assert not fs.matches(subs, 2, g, None)
    subs.append([4])                                                  # grown in place: not the list the facts were made from
    assert not f.matches(subs, 2, g, None) and not f.matches(subs, 3, g, None)
    # the list is HELD: its id cannot be handed to another list while the facts exist
    held = _facts([[7]], g)
    assert held.sub_g == [[7]] and not held.matches([[7]], 1, g, None)


def test_facts_are_kept_per_split_and_forgotten_on_request():
    from subgnn_amd import hotpath
    m = types.SimpleNamespace()
    g = object()
    train, val = [[1]], [[2]]
    ft, fv = _filled(m, 'train', train, g), _filled(m, 'val', val, g)
    assert m._split_facts == {'train': ft, 'val': fv} and ft is not fv
    assert hotpath._split_record(m, 'train', train, g, None) is ft and hotpath._split_record(m, 'val', val, g, None) is fv
    # replacing a split's record leaves no field of the old one reachable -- everything hangs on the one record; the other
    # split's stays
    other = [[3]]
    f2 = hotpath._split_record(m, 'train', other, g, None)
    assert f2 is not ft and f2.matches(other, 1, g, None) and m._split_facts == {'train': f2, 'val': fv}
    assert all(getattr(f2, nm) is None for nm in _FIELDS) and f2.border_width == {} and f2.borders == {} and f2.nbytes == 0
    assert all(getattr(fv, nm) == ('val', nm) for nm in _FIELDS if nm != 'dims') and fv.border_width == {1: ('val', 'width')}
    assert hotpath._split_record(m, 'train', other, g, None) is f2
    assert hotpath._split_record(m, 'train', other, g, types.SimpleNamespace(start=0, world=2)) is not f2      # another shard
    # a pass that is being recorded and finds no matching record works from a temporary one: nothing new is kept
    f3 = m._split_facts['train']
    tmp = hotpath._split_record(m, 'train', train, g, None, store=False)
    assert tmp is not f3 and tmp.matches(train, 1, g, None) and tmp.subs is None and m._split_facts == {'train': f3, 'val': fv}
    assert hotpath._split_record(m, 'val', val, g, None, store=False) is fv
    hotpath.forget_split_facts(m, 'train')
    assert m._split_facts == {'val': fv}
    hotpath.forget_split_facts(m)
    assert m._split_facts == {}
    hotpath.forget_split_facts(types.SimpleNamespace())               # (a model that never kept any)


def test_forgetting_a_split_leaves_nothing_of_it_and_all_of_the_other():
    from subgnn_amd import hotpath
    g = object()

    def model():
        m = types.SimpleNamespace()
        recs = {sp: _filled(m, sp, [[i + 1]], g) for i, sp in enumerate(('train', 'val'))}
        m._bfs_level_hint = {(kind, sp, l): 5 for kind in ('P_out', 'P_out_dealt') for sp in ('train', 'val') for l in (0, 1)}
        m._bfs_push_hint = {('P_out', sp, l): 2 for sp in ('train', 'val') for l in (0, 1)}
        m._bfs_status_pool, m._device_label_cache = ['buffer'], {'train': 'labels'}           # keyed by other things: they stay
        return m, recs
    m, recs = model()
    before = {k: v for k, v in vars(recs['val']).items()}
    hotpath.forget_split_facts(m, 'train')
    assert m._split_facts == {'val': recs['val']} and vars(recs['val']) == before
    assert m._bfs_level_hint == {(kind, 'val', l): 5 for kind in ('P_out', 'P_out_dealt') for l in (0, 1)}
    assert m._bfs_push_hint == {('P_out', 'val', l): 2 for l in (0, 1)}
    assert m._bfs_status_pool == ['buffer'] and m._device_label_cache == {'train': 'labels'}
    assert hotpath.split_facts_bytes(m, 'train') == (0, 0)
    # the next pass of the split starts from an empty record
    again = hotpath._split_record(m, 'train', recs['train'].sub_g, g, None)
    assert again is not recs['train'] and again.subs is None and again.borders == {} and again.dtw_rows is None
    m, recs = model()
    hotpath.forget_split_facts(m)
    assert m._split_facts == {} and m._bfs_level_hint == {} and m._bfs_push_hint == {} and m._bfs_status_pool == ['buffer']


def test_the_compatibility_views_have_the_shapes_of_the_dictionaries_they_replace():
    """What SubGNN._degseq_order and SubGNN._border_width return (hotpath.set_orders, hotpath.border_widths): {split: order}
    and {(split, k, component rows, world): width}, built from the records."""
    from subgnn_amd import hotpath
    m, g = types.SimpleNamespace(), object()
    assert hotpath.set_orders(m) == {} and hotpath.border_widths(m) == {}
    train = _filled(m, 'train', [[1], [2], [3], [4], [5]], g)                        # 5 subgraphs x dims[0] = 3 component rows each
    val = _filled(m, 'val', [[1], [2]], g, types.SimpleNamespace(start=2, world=4))
    val.border_width[2] = 'two hops'
    hotpath._split_record(m, 'test', [], g, None)                                    # (prepared by no pass yet: in neither view)
    assert hotpath.set_orders(m) == {'train': ('train', 'set_order'), 'val': ('val', 'set_order')}
    assert hotpath.border_widths(m) == {('train', 1, 15, 1): ('train', 'width'), ('val', 1, 6, 4): ('val', 'width'),
                                        ('val', 2, 6, 4): 'two hops'}
    assert train.n == 5 and val.shard_key == (2, 4)


def test_row_prep_forgets_on_another_shape_and_on_another_fixed_tensor():
    from subgnn_amd import ops
    ptr, val = torch.zeros(4, dtype=torch.int64), torch.zeros(9, dtype=torch.int32)
    p = ops.DtwRowPrep().fit(ptr, val)
    p.order = p.grouped_val = p.rows = 'kept'
    assert p.fit(ptr, val).rows == 'kept' and p.fixed_src is None
    assert p.fit(ptr, val, fixed=True).rows == 'kept' and p.fixed_src is val          # structure from unpromised calls stays
    assert p.fit(ptr, val, fixed=True).rows == 'kept'
    assert p.fit(ptr, val.clone()).rows == 'kept'                                     # no promise, no identity check
    twin = val.clone()
    assert p.fit(ptr, twin, fixed=True).rows is None and p.order is None and p.grouped_val is None and p.fixed_src is twin
    p.rows = 'kept'
    assert p.fit(torch.zeros(5, dtype=torch.int64), twin, fixed=True).rows is None and p.shape == (4, 9)
    assert ops.DtwRowPrep().nbytes == 0


@pytest.mark.parametrize('pre,plain', [('sgnn_dtw_', 'sgnn_dtw_'), ('sgnn_dtwx_', 'sgnn_dtw_exact_')])
def test_rows_entries_answer_sizes_and_refuse_bad_headers_on_the_host(pre, plain):
    from subgnn_amd import _lib
    lib = _lib.load()
    rows = getattr(lib, pre + 'rows_bytes')(130, 20)
    if pre == 'sgnn_dtw_':
        assert rows == 2 * 130 * (20 + 10 + 5 + 2 + 1) * 8 + 130 * 4             # value + reciprocal pyramids, lengths
    else:
        assert rows == 2 * 130 * 20 * 8 + 130 * 4
    whole = getattr(lib, plain + 'workspace_bytes')(130, 20, 3, 50)
    assert getattr(lib, pre + 'rows_workspace_bytes')(130, 20, 3, 50) == whole - rows > 0
    words = lib.sgnn_dtw_rows_header_words()
    assert words == 8
    header = (ctypes.c_int64 * words)()
    tie = [0] if pre == 'sgnn_dtw_' else []
    # nothing is launched for a header nobody filled (every pointer below is a dummy that is never read)
    dummy = ctypes.c_void_p(8)
    rc = getattr(lib, pre + 'similarity_rows')(ctypes.addressof(header), 130, 20, dummy, dummy, 3, 50, *tie, 0, None, dummy, dummy,
                                               1 << 40, None)
    assert rc == -1
    assert getattr(lib, pre + 'similarity_rows')(None, 130, 20, dummy, dummy, 3, 50, *tie, 0, None, dummy, dummy, 1 << 40, None) == -1
    assert getattr(lib, pre + 'prepare_rows')(None, None, 130, 20, 0, None, None, 0, ctypes.addressof(header), None) == -1
    assert getattr(lib, pre + 'prepare_rows')(dummy, dummy, 130, 20, 0, None, dummy, rows - 1, ctypes.addressof(header), None) == -1
    assert getattr(lib, pre + 'prepare_rows')(dummy, dummy, 130, 20, 0, None, dummy, rows, None, None) == -1
    live = getattr(lib, pre + 'similarity_rows_live')
    assert live(ctypes.addressof(header), 130, 20, dummy, dummy, 3, 50, *tie, 0, None, dummy, dummy, dummy, 1 << 40, None) == -1

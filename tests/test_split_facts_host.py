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
    assert hotpath._split_facts(m, 'train', train, 1, g, None) is None
    ft = hotpath._keep_split_facts(m, 'train', _facts(train, g))
    fv = hotpath._keep_split_facts(m, 'val', _facts(val, g))
    assert hotpath._split_facts(m, 'train', train, 1, g, None) is ft and hotpath._split_facts(m, 'val', val, 1, g, None) is fv
    assert hotpath._split_facts(m, 'train', val, 1, g, None) is None
    # replacing a split's facts drops what else was derived from the old components; the other split's stay
    m._dtw_group_rows, m._degseq_order = {'train': 1, 'val': 2}, {'train': 1, 'val': 2}
    m._border_width = {('train', 1, 5, 1): 3, ('val', 1, 5, 1): 4}
    other = [[3]]
    f2 = hotpath._keep_split_facts(m, 'train', _facts(other, g))
    assert hotpath._split_facts(m, 'train', train, 1, g, None) is None and hotpath._split_facts(m, 'train', other, 1, g, None) is f2
    assert m._dtw_group_rows == {'val': 2} and m._degseq_order == {'val': 2} and m._border_width == {('val', 1, 5, 1): 4}
    hotpath.forget_split_facts(m, 'train')
    assert hotpath._split_facts(m, 'train', other, 1, g, None) is None and hotpath._split_facts(m, 'val', val, 1, g, None) is fv
    hotpath.forget_split_facts(m)
    assert m._split_facts == {}
    hotpath.forget_split_facts(types.SimpleNamespace())               # (a model that never kept any)


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

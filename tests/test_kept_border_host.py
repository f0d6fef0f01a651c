"""CPU: the two entry points of the kept one-hop borders refuse bad arguments on the host, before anything touches a device."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    from subgnn_amd import _lib
    return _lib.load()


def _buf(n=64):
    b = (ctypes.c_int64 * n)()
    return b, ctypes.cast(b, ctypes.c_void_p)


def test_border_sorted_refuses_bad_arguments(lib):
    keep, p = _buf()
    good = dict(rowptr=p, col=p, col_sorted=p, nnz=8, max_id=7, set_ptr=p, set_nodes=p, n_sets=2, out_count=p, out_ptr=p, out_ids=p,
                workspace=p, workspace_bytes=16, bitmap_in_lds=1, stream=None)

    def call(**over):
        return lib.sgnn_khop1_border_sorted(*{**good, **over}.values())
    for name in ('rowptr', 'col', 'set_ptr', 'set_nodes', 'workspace'):
        assert call(**{name: None}) == -1, name
    assert call(out_count=None, out_ids=None) == -1            # nothing to write
    assert call(out_ptr=None) == -1                            # ids without their offsets
    assert call(n_sets=-1) == -1
    assert call(workspace_bytes=8) == -1
    assert call(nnz=1 << 31) == -3
    # where the one-hop kernel does not apply: an error code, not another kernel's answer
    assert call(bitmap_in_lds=0) == -2                         # no LDS bitmap
    assert call(max_id=3_000_000, col_sorted=None) == -2       # slices needed, rows not ascending
    assert call(max_id=1 << 40) == -2                          # no LDS plan at all
    assert call(n_sets=0) == 0                                 # nothing to do, nothing launched
    del keep


def test_border_draw_refuses_bad_arguments(lib):
    keep, p = _buf()
    good = dict(ptr=p, ids=p, counts=p, n_sets=2, width=p, n_slots=4, seed=1, stream_id=2, item_base=0, hop=1, out_anchor=p,
                out_sims=p, stream=None)

    def call(**over):
        return lib.sgnn_sample_border_anchors(*{**good, **over}.values())
    for name in ('ptr', 'ids', 'counts', 'width', 'out_anchor', 'out_sims'):
        assert call(**{name: None}) == -1, name
    assert call(n_sets=-1) == -1
    assert call(n_slots=-1) == -1
    assert call(item_base=-1) == -1
    assert call(n_sets=0) == 0 and call(n_slots=0) == 0        # nothing to do, nothing launched
    del keep

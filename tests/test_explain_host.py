"""CPU: the host side of the occlusion sets and of subgnn_amd/explain.py -- the numpy definition's cases reach every kernel path
in both modes, the incremental key identity, the CLI's argument rules and line format, the header's declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

import occlusion_cases as OC

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def test_the_cases_reach_every_path_in_both_modes():
    want = {'wave', 'lds', 'streamed'}
    node = {OC.path_of(len(s)) for sets in OC.node_cases().values() for s in sets}
    assert node == want
    for shape in OC.SHAPES:
        got = {OC.path_of(len(s)) for name, (sets, _l) in OC.component_cases().items() if name.startswith(shape) for s in sets}
        assert got == want, shape
    assert {OC.path_of(len(s)) for s in OC.component_cases()['mixed'][0]} == want
    # both sides of both thresholds, and the lengths without a variant
    for n in (0, 1, 2, 3, OC.WAVE_MAX - 1, OC.WAVE_MAX, OC.WAVE_MAX + 1, 200, OC.LDS_MAX, OC.LDS_MAX + 1):
        assert n in OC.LENGTHS
    assert OC.path_of(OC.WAVE_MAX) == 'wave' and OC.path_of(OC.WAVE_MAX + 1) == 'lds'
    assert OC.path_of(OC.LDS_MAX) == 'lds' and OC.path_of(OC.LDS_MAX + 1) == 'streamed'


def test_the_restated_thresholds_are_the_sources():
    txt = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'occlusion.hip')).read()
    assert int(re.search(r'#define SGNN_OCC_LDS_MAX (\d+)', txt).group(1)) == OC.LDS_MAX
    txt = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'id_table.h')).read()
    assert int(re.search(r'#define SGNN_SET_WAVE_MAX (\d+)', txt).group(1)) == OC.WAVE_MAX
    from subgnn_amd import ops
    assert ops.occlusion_lds_max() == OC.LDS_MAX                      # a host call of the built library


def test_the_definition_on_a_set_small_enough_to_read():
    ids = np.array([3, 5, 8, 13], dtype=np.int32)
    e = OC.expand([ids, ids[:1], ids[:0]], 'node')
    assert e['units'].tolist() == [4, 1, 0] and e['variants'].tolist() == [4, 0, 0]
    assert e['nodes'].tolist() == [5, 8, 13, 3, 8, 13, 3, 5, 13, 3, 5, 8] and e['ptr'].tolist() == [0, 3, 6, 9, 12]
    assert e['parent'].tolist() == [0] * 4 and e['unit'].tolist() == [0, 1, 2, 3] and e['lens'].tolist() == [3, 3, 3, 3, 0]
    lab = np.array([0, 1, 0, 1], dtype=np.int32)                      # {3, 8} and {5, 13}
    e = OC.expand([ids, ids], 'component', [lab, np.zeros(4, dtype=np.int32)])
    assert e['units'].tolist() == [2, 1] and e['variants'].tolist() == [2, 0]
    assert e['nodes'].tolist() == [5, 13, 3, 8] and e['ptr'].tolist() == [0, 2, 4] and e['unit'].tolist() == [0, 1]
    assert e['lens'].tolist() == [2, 2, 0, 0, 0, 0, 0, 0]


def test_the_incremental_key_is_the_key_of_the_variant():
    from subgnn_amd import tape
    wrapped = 0
    checked = 0
    for n in (2, 3, 17, 65, 200):
        ids = OC.make_set(n, 40 + n, id_range=2 ** 31 - 1)            # ids up to the largest int32
        for shape in OC.SHAPES:
            for gone in OC.units_of(n, 'component', OC.make_labels(n, shape)) + OC.units_of(n, 'node')[:5]:
                if len(gone) == n:
                    continue
                keep = np.ones(n, dtype=bool)
                keep[gone] = False
                key, wrap = OC.incremental_key(ids, gone)
                assert key == tape.set_key_np(ids[keep]), (n, shape, gone[:4])
                wrapped += wrap
                checked += 1
    assert checked > 100 and 0 < wrapped < checked                    # the subtraction wrapped in some and not in others
    # a case made to wrap: the parent's sum is small, the removed term is not
    ids = np.array([7, 11, 19], dtype=np.int32)
    mixed = tape.mix64_np(ids.astype(np.uint64))
    with np.errstate(over='ignore'):
        total = mixed.sum(dtype=np.uint64)
    gone = [int(np.argmax(mixed))] if total < mixed.max() else None
    if gone is not None:
        key, wrap = OC.incremental_key(ids, gone)
        assert wrap and key == tape.set_key_np(np.delete(ids, gone))


def test_the_new_symbols_are_declared_and_bound():
    from subgnn_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    for name in ('sgnn_occlusion_count', 'sgnn_occlusion_write', 'sgnn_occlusion_lds_max', 'sgnn_occlusion_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, txt), name
        assert name in _lib.SIGNATURES
    assert 'SGNN_OCC_NODE 0' in txt and 'SGNN_OCC_COMPONENT 1' in txt
    assert '#define SGNN_ABI_VERSION 14' in txt
    lib = _lib.load()
    assert lib.sgnn_occlusion_workspace_bytes(1000) == 16000 and lib.sgnn_occlusion_workspace_bytes(-1) == 0
    # refused on the host, before any launch: unknown mode, negative sizes, null pointers with non-zero counts
    assert lib.sgnn_occlusion_count(None, None, 1, 1, 0, None, None, None, None, 0, None, 0, None) == -1
    assert lib.sgnn_occlusion_count(None, None, 0, 0, 7, None, None, None, None, 0, None, 0, None) == -1
    assert lib.sgnn_occlusion_count(None, None, -1, 0, 0, None, None, None, None, 0, None, 0, None) == -1
    assert lib.sgnn_occlusion_write(None, None, 1, 1, 0, None, None, None, 3, None, None, None, None, None, 0, None, 0, None) == -1
    assert lib.sgnn_occlusion_write(None, None, 0, 0, 0, None, None, None, -1, None, None, None, None, None, 0, None, 0, None) == -1
    assert lib.sgnn_occlusion_count(None, None, 0, 0, 0, None, None, None, None, 0, None, 0, None) == 0      # nothing to do


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
BASE = ['-config_path', 'c.json', '-restoreModelPath', 'run', '-subgraphs', 'in.txt', '-out', 'out.txt']


def test_cli_argument_rules():
    from subgnn_amd import explain
    a = explain.parse_args(BASE)
    assert (a.unit, a.target, a.draws, a.top, a.batch_size, a.restoreModelName) == ('node', None, 1, None, None, None)
    a = explain.parse_args(BASE + ['-unit', 'component', '-target', 'lab', '-draws', '4', '-top', '3', '-batch_size', '8'])
    assert (a.unit, a.target, a.draws, a.top, a.batch_size) == ('component', 'lab', 4, 3, 8)
    for bad in (['-draws', '0'], ['-top', '0'], ['-batch_size', '-2'], ['-unit', 'edge'], ['-draws', 'x']):
        with pytest.raises(SystemExit):
            explain.parse_args(BASE + bad)
    with pytest.raises(SystemExit):                                   # distinct files
        explain.parse_args(BASE[:-1] + ['in.txt'])
    with pytest.raises(SystemExit):
        explain.parse_args(BASE[2:])


def test_cli_line_format_and_order():
    from subgnn_amd import explain
    assert explain.HEADER.split('\t') == ['request', 'unit', 'delta_logit', 'delta_std', 'delta_prob', 'label_without']
    x = np.float32(0.1)
    line = explain.format_line(3, [17], x, np.float32(0.0), np.float32(-0.25), ['a'])
    assert line == '3\t17\t0.100000001\t0\t-0.25\ta'
    assert np.float32(float(line.split('\t')[2])) == x                # 9 digits: a float32 survives the round trip
    assert explain.format_line(0, [4, 9, 12], 1.5, 0.5, 0.125, ['a', 'b']) == '0\t4-9-12\t1.5\t0.5\t0.125\ta-b'
    assert explain.format_line(1, [2], float('nan'), float('nan'), float('nan'), []) == '1\t2\tnan\tnan\tnan\t'
    # descending delta_logit, ties by ascending rank, invalid last (whatever they hold)
    nan = float('nan')
    assert explain.unit_order([0.5, 2.0, nan, 2.0, -1.0], [True, True, False, True, True]) == [1, 3, 0, 4, 2]
    assert explain.unit_order([nan], [False]) == [0] and explain.unit_order([], []) == []


def test_lines_of_writes_requests_in_order_units_sorted_and_top():
    import torch
    from subgnn_amd import explain

    class P:
        class model:
            multilabel = False

        @staticmethod
        def names_of(row):
            return ['L%d' % int(row)]

    nan = float('nan')
    res = {'ptr': torch.tensor([0, 3, 4]), 'valid': torch.tensor([True, True, True, False]),
           'delta_logit': torch.tensor([0.25, 1.0, -0.5, nan]), 'delta_std': torch.tensor([0., 0., 0., nan]), 'delta_prob': torch.tensor([0.1, 0.2, -0.1, nan]),
           'variant_logits': torch.tensor([[0., 1.], [2., 1.], [0., 3.], [nan, nan]]), 'unit_nodes': torch.tensor([5, 7, 9, 2])}
    lines = explain.lines_of(P, res)
    assert [l.split('\t')[:2] for l in lines] == [['0', '6'], ['0', '4'], ['0', '8'], ['1', '1']]
    assert [l.split('\t')[5] for l in lines] == ['L0', 'L1', 'L1', '']
    assert lines[3] == '1\t1\tnan\tnan\tnan\t'
    assert [l.split('\t')[1] for l in explain.lines_of(P, res, top=2)] == ['6', '4', '1']
    res['unit_nodes'] = (torch.tensor([0, 2, 3, 4, 5]), torch.tensor([5, 6, 7, 9, 2]))          # components
    assert [l.split('\t')[1] for l in explain.lines_of(P, res)] == ['6', '4-5', '8', '1']

"""CPU: the host side of the insertion sets and of subgnn_amd/suggest.py -- the numpy definition's cases reach every kernel tier,
candidate shape and candidate form, the incremental key identity for additions, the header's declarations, the argument checks
of ops.insertion_sets, the CLI's argument rules, line formats and pool reader, and grow's choice rule.  No GPU."""
import os
import re
import types

import numpy as np
import pytest

import insertion_cases as IC

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def test_the_cases_reach_every_tier_shape_and_form():
    want = {'wave', 'lds', 'streamed'}
    assert {IC.path_of(n) for n in IC.SET_LENGTHS} == want
    for n in (0, 1, 2, IC.WAVE_MAX - 1, IC.WAVE_MAX, IC.WAVE_MAX + 1, 200, IC.LDS_MAX, IC.LDS_MAX + 1):
        assert n in IC.SET_LENGTHS
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 1000):                 # the chunk edges of both workgroup sizes, several chunks
        assert m in IC.CAND_LENGTHS
    assert IC.path_of(IC.WAVE_MAX) == 'wave' and IC.path_of(IC.WAVE_MAX + 1) == 'lds'
    assert IC.path_of(IC.LDS_MAX) == 'lds' and IC.path_of(IC.LDS_MAX + 1) == 'streamed'
    names = list(IC.single_cases(lengths=(2,)))
    assert len(names) == len(IC.CAND_LENGTHS) * len(IC.SHAPES)
    for shape in IC.SHAPES:
        assert sum(name.endswith(shape) for name in names) == len(IC.CAND_LENGTHS)
    sets, rows = IC.mixed_case()
    assert len(rows) == len(sets) == 2 * len(IC.SET_LENGTHS) and {IC.path_of(len(s)) for s in sets} == want
    sets, pool = IC.pool_case()
    assert len(pool) == 1 and {IC.path_of(len(s)) for s in sets} == want
    e = IC.expand(sets, pool, shared=True)                            # members of every non-empty set are in the pool, and others
    assert all(0 < e['variants'][i] < len(pool[0]) for i, s in enumerate(sets) if len(s))
    assert all(e['variants'][i] == len(pool[0]) for i, s in enumerate(sets) if not len(s))


@pytest.mark.parametrize('shape', IC.SHAPES)
def test_the_candidate_shapes_are_what_they_say(shape):
    for n in (0, 1, 65, 200):
        ids = IC.make_set(n, 100 + n)
        for m in (0, 1, 65, 257):
            row = IC.make_candidates(ids, m, shape, 5)
            assert row.dtype == np.int32 and bool((np.diff(row) > 0).all()) and (row.size == 0 or row[0] >= 1)
            member = np.isin(row, ids)
            rank = np.searchsorted(ids, row)
            if shape == 'all_members':
                assert len(row) == min(m, n) and bool(member.all())
                continue
            assert len(row) == m
            if shape == 'mixed':
                assert int(member.sum()) == min((m + 2) // 3, n)
            else:
                assert not bool(member.any())
            if shape == 'below':
                assert bool((rank == 0).all())
            if shape == 'above':
                assert bool((rank == n).all())
            if shape == 'interleaved' and n >= 65 and m:
                assert bool(((rank > 0) & (rank < n)).all()) and (m == 1 or len(set(rank.tolist())) > 1)


def test_the_restated_thresholds_are_the_sources():
    txt = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'insertion.hip')).read()
    assert int(re.search(r'#define SGNN_INS_LDS_MAX (\d+)', txt).group(1)) == IC.LDS_MAX
    # the grid of a tier's launch: sgnn_grid_for(n_sets, 1, 256 * 32) for the one-wavefront tier
    assert re.search(r'sgnn_grid_for\(a\.n_sets, 1, 256 \* \(THREADS == 64 \? 32 : 16\)\)', txt)
    assert IC.WAVE_GRID_CAP == 256 * 32 == 8192 and IC.MANY > IC.WAVE_GRID_CAP
    sets, rows = IC.many_case()
    assert len(sets) == len(rows) == IC.MANY and all(len(s) == 1 and len(r) == 1 for s, r in zip(sets, rows))
    txt = open(os.path.join(REPO, 'subgnn_amd', 'csrc', 'id_table.h')).read()
    assert int(re.search(r'#define SGNN_SET_WAVE_MAX (\d+)', txt).group(1)) == IC.WAVE_MAX


def test_the_definition_on_a_set_small_enough_to_read():
    ids = np.array([3, 5, 8, 13], dtype=np.int32)
    row = np.array([1, 5, 6, 20], dtype=np.int32)
    e = IC.expand([ids, ids[:0], ids[:1]], [row, row[1:3], ids[:1]])
    assert e['variants'].tolist() == [3, 2, 0]
    assert e['nodes'].tolist() == [1, 3, 5, 8, 13, 3, 5, 6, 8, 13, 3, 5, 8, 13, 20, 5, 6] and e['ptr'].tolist() == [0, 5, 10, 15, 16, 17]
    assert e['parent'].tolist() == [0, 0, 0, 1, 1] and e['cand'].tolist() == [1, 6, 20, 5, 6]
    s = IC.expand([ids, ids[:0]], [row], shared=True)                 # one row for both
    assert s['variants'].tolist() == [3, 4] and s['nodes'].tolist() == e['nodes'].tolist()[:15] + [1, 5, 6, 20]
    assert s['cand'].tolist() == [1, 6, 20, 1, 5, 6, 20] and s['parent'].tolist() == [0, 0, 0, 1, 1, 1, 1]


def test_the_incremental_key_is_the_key_of_the_variant():
    from subgnn_amd import tape
    rng = np.random.default_rng(3)
    wrapped = checked = 0
    for n in (0, 1, 2, 17, 65, 200):
        ids = np.unique(rng.integers(1, 2 ** 31 - 1, size=n)).astype(np.int32)      # ids up to the largest int32
        for v in [1, 2 ** 31 - 1] + rng.integers(1, 2 ** 31 - 1, size=20).tolist():
            if v in ids:
                continue
            key, wrap = IC.incremental_key(ids, v)
            assert key == tape.set_key_np(np.sort(np.append(ids.astype(np.int64), v))), (n, v)
            wrapped += wrap
            checked += 1
    assert checked > 100 and 0 < wrapped < checked                    # the addition wrapped in some and not in others
    # a case made to wrap: one entry whose term is large, and the first candidate whose term carries the sum past 2^64
    ids = np.array([7], dtype=np.int32)
    total = int(tape.mix64_np(np.uint64(7)))
    v = next(v for v in range(8, 200) if total + int(tape.mix64_np(np.uint64(v))) >= 2 ** 64)
    key, wrap = IC.incremental_key(ids, v)
    assert wrap and key == tape.set_key_np([7, v])
    v = next(v for v in range(8, 200) if total + int(tape.mix64_np(np.uint64(v))) < 2 ** 64)
    key, wrap = IC.incremental_key(ids, v)
    assert not wrap and key == tape.set_key_np([7, v])
    # the empty set: its variants are the singletons
    assert IC.incremental_key(np.zeros(0, dtype=np.int32), 9)[0] == tape.set_key_np([9])


def test_the_new_symbols_are_declared_and_bound():
    from subgnn_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'subgnn_hip.h')).read()
    for name in ('sgnn_insertion_count', 'sgnn_insertion_write'):
        assert re.search(r'\bint %s\s*\(' % name, txt), name
        assert name in _lib.SIGNATURES
    assert '#define SGNN_ABI_VERSION 14' in txt
    lib = _lib.load()
    assert lib.sgnn_abi_version() == 14
    # refused on the host, before any launch: negative sizes, sizes past 2^31 - 1, shared outside {0, 1}, null pointers with work
    assert lib.sgnn_insertion_count(None, None, -1, 0, None, None, 0, None, None) == -1
    assert lib.sgnn_insertion_count(None, None, 2 ** 31, 0, None, None, 0, None, None) == -1
    assert lib.sgnn_insertion_count(None, None, 0, -1, None, None, 0, None, None) == -1
    assert lib.sgnn_insertion_count(None, None, 0, 0, None, None, 2, None, None) == -1
    assert lib.sgnn_insertion_count(None, None, 0, 0, None, None, -1, None, None) == -1
    assert lib.sgnn_insertion_count(None, None, 1, 1, None, None, 0, None, None) == -1
    assert lib.sgnn_insertion_write(None, None, 0, 0, None, None, 0, None, None, -1, None, None, None, None, None, None) == -1
    assert lib.sgnn_insertion_write(None, None, 0, 0, None, None, 0, None, None, 2 ** 31, None, None, None, None, None, None) == -1
    assert lib.sgnn_insertion_write(None, None, 0, 0, None, None, 0, None, None, 3, None, None, None, None, None, None) == -1
    assert lib.sgnn_insertion_write(None, None, 0, 0, None, None, 3, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.sgnn_insertion_count(None, None, 0, 0, None, None, 0, None, None) == 0                      # nothing to do
    assert lib.sgnn_insertion_write(None, None, 0, 0, None, None, 1, None, None, 0, None, None, None, None, None, None) == 0


def _fake(dtype, n):
    """What ops._req reads of a tensor, without a device."""
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, is_contiguous=lambda: True, numel=lambda: n)


def _fake_ragged(n, ptr_dtype=None, nodes_dtype=None):
    import torch
    return types.SimpleNamespace(ptr=_fake(ptr_dtype or torch.int64, n + 1), nodes=_fake(nodes_dtype or torch.int32, 5), n=n, max_len=3)


def test_insertion_sets_checks_its_arguments_before_any_library_call(monkeypatch):
    import torch
    from subgnn_amd import ops, _lib

    def no_call():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_call)
    good = _fake_ragged(4)
    for bad in (_fake_ragged(4, ptr_dtype=torch.int32), _fake_ragged(4, nodes_dtype=torch.int64)):
        with pytest.raises(TypeError):
            ops.insertion_sets(bad, good)
        with pytest.raises(TypeError):
            ops.insertion_sets(good, bad)
    with pytest.raises(ValueError, match='3 rows for 4 sets'):
        ops.insertion_sets(good, _fake_ragged(3))
    with pytest.raises(ValueError, match='4 rows for 4 sets'):
        ops.insertion_sets(good, good, shared=True)
    with pytest.raises(ValueError, match='1 rows for 4 sets'):
        ops.insertion_sets(good, _fake_ragged(1))
    with pytest.raises(AssertionError, match='the library was loaded'):       # what is well formed goes on to the library
        ops.insertion_sets(good, _fake_ragged(1), shared=True)
    assert ops.Insertion._fields == ('sets', 'parent', 'cand', 'keys', 'variants')


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
BASE = ['-config_path', 'c.json', '-restoreModelPath', 'run', '-subgraphs', 'in.txt', '-out', 'out.txt']


def test_cli_argument_rules():
    from subgnn_amd import suggest
    a = suggest.parse_args(BASE)
    assert (a.candidates, a.hops, a.target, a.draws, a.top, a.batch_size, a.grow, a.min_gain, a.restoreModelName) == \
        ('border', 1, None, 1, None, None, None, 0.0, None)
    a = suggest.parse_args(BASE + ['-candidates', 'pool.txt', '-hops', '2', '-target', 'lab', '-draws', '4', '-top', '3',
                                   '-batch_size', '8'])
    assert (a.candidates, a.hops, a.target, a.draws, a.top, a.batch_size) == ('pool.txt', 2, 'lab', 4, 3, 8)
    a = suggest.parse_args(BASE + ['-grow', '5', '-min_gain', '0.25'])
    assert (a.grow, a.min_gain) == (5, 0.25)
    assert suggest.parse_args(BASE + ['-grow', '2', '-min_gain', '-1']).min_gain == -1.0
    for bad in (['-draws', '0'], ['-top', '0'], ['-batch_size', '-2'], ['-hops', '0'], ['-grow', '0'], ['-draws', 'x'],
                ['-min_gain', '0.5'], ['-grow', '2', '-top', '3'], ['-grow', '2', '-min_gain', 'nan'], ['-candidates', 'out.txt']):
        with pytest.raises(SystemExit):
            suggest.parse_args(BASE + bad)
    with pytest.raises(SystemExit):                                   # distinct files
        suggest.parse_args(BASE[:-1] + ['in.txt'])
    with pytest.raises(SystemExit):
        suggest.parse_args(BASE[2:])


def test_cli_line_format_and_order():
    from subgnn_amd import suggest
    assert suggest.HEADER == 'request\tcandidate\tgain_logit\tgain_std\tgain_prob\tlabel_with'
    assert suggest.GROW_HEADER == 'request\tstep\tadded\tgain_logit\tgain_std\tlabel_after'
    x = np.float32(0.1)
    line = suggest.format_line(3, 17, x, np.float32(0.0), np.float32(-0.25), ['a'])
    assert line == '3\t17\t0.100000001\t0\t-0.25\ta'
    assert np.float32(float(line.split('\t')[2])) == x                # 9 digits: a float32 survives the round trip
    assert suggest.format_line(0, np.int64(4), 1.5, 0.5, 0.125, ['a', 'b']) == '0\t4\t1.5\t0.5\t0.125\ta-b'
    assert suggest.format_grow_line(2, 0, 31, x, 0.5, ['b']) == '2\t0\t31\t0.100000001\t0.5\tb'
    # descending gain_logit, ties by ascending id
    assert suggest.candidate_order([0.5, 2.0, 2.0, -1.0, 2.0], [9, 30, 20, 1, 25]) == [2, 4, 1, 0, 3]
    assert suggest.candidate_order([], []) == []


def test_lines_of_writes_requests_in_order_candidates_sorted_and_top():
    import torch
    from subgnn_amd import suggest

    class P:
        class model:
            multilabel = False

        @staticmethod
        def names_of(row):
            return ['L%d' % int(row)]

    res = {'ptr': torch.tensor([0, 3, 3, 4]), 'candidate_nodes': torch.tensor([5, 7, 9, 2]),
           'gain_logit': torch.tensor([0.25, 1.0, 1.0, -0.5]), 'gain_std': torch.zeros(4), 'gain_prob': torch.tensor([0.1, 0.2, 0.2, -0.1]),
           'variant_logits': torch.tensor([[0., 1.], [2., 1.], [0., 3.], [4., 3.]])}
    lines = suggest.lines_of(P, res)
    assert [l.split('\t')[:2] for l in lines] == [['0', '6'], ['0', '8'], ['0', '4'], ['2', '1']]      # (dataset ids: model id - 1)
    assert [l.split('\t')[5] for l in lines] == ['L0', 'L1', 'L1', 'L0']
    assert lines[0] == '0\t6\t1\t0\t0.200000003\tL0'
    assert [l.split('\t')[1] for l in suggest.lines_of(P, res, top=1)] == ['6', '1']
    grown = {'added': [[4, 9], [], [1]], 'gain_logit': [[0.5, 0.25], [], [2.0]], 'gain_std': [[0.0, 0.0], [], [0.125]],
             'step_logits': [[torch.tensor([0., 1.]), torch.tensor([3., 1.])], [], [torch.tensor([1., 0.])]]}
    assert suggest.grow_lines_of(P, grown) == ['0\t0\t4\t0.5\t0\tL1', '0\t1\t9\t0.25\t0\tL0', '2\t0\t1\t2\t0.125\tL0']


def test_the_pool_file_reader(tmp_path):
    from subgnn_amd import suggest
    f = tmp_path / 'pool.txt'
    f.write_text('3 17\n\n 4\t99\n8\n')
    assert suggest.read_pool(f) == [3, 17, 4, 99, 8]
    f.write_text('')
    assert suggest.read_pool(f) == []
    f.write_text('3 x7\n')
    with pytest.raises(ValueError, match="'x7' is no node id"):
        suggest.read_pool(f)


def test_grows_choice_the_tie_rule_and_the_stopping_rule():
    from subgnn_amd import suggest
    nan = float('nan')
    ptr = [0, 3, 3, 6, 8, 9]
    ids = [10, 20, 30, 40, 50, 60, 12, 11, 5]
    gain = [0.5, 2.0, 1.0, 0.0, -1.0, 0.0, 0.75, 0.75, nan]
    # the largest gain; no candidate; none above 0; a tie: the smaller id; NaN is never taken
    assert suggest.choose(ptr, ids, gain) == [1, -1, -1, 7, -1]
    assert suggest.choose(ptr, ids, gain, min_gain=-0.5) == [1, -1, 3, 7, -1]          # (0 > -0.5; the tie 40 / 60 goes to 40)
    assert suggest.choose(ptr, ids, gain, min_gain=0.75) == [1, -1, -1, -1, -1]        # strictly above
    assert suggest.choose(ptr, ids, gain, min_gain=2.0) == [-1] * 5                    # above every gain: nothing is added
    assert suggest.choose(ptr, np.array(ids), np.array(gain, dtype=np.float32)) == [1, -1, -1, 7, -1]
    assert suggest.choose([0], [], []) == []
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            suggest.grow(None, [[1]], bad)

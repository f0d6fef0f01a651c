"""Host side of prediction on subgraphs outside the dataset: the content key's formula (tape.set_key_np, twin of
sgnn_set_keys), the additive split code, the CLI's argument rules and the file formats.  No GPU."""
import numpy as np
import pytest

MASK64 = (1 << 64) - 1


def _mix64(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def _key(ids):
    """The formula of include/subgnn_hip.h (sgnn_set_keys) in Python integers."""
    return _mix64((sum(_mix64(v) for v in ids) + (len(ids) + 1) * 0x8CB92BA72F3D8DD7) & MASK64)


def test_set_key_formula_order_repeats_and_the_empty_set():
    from subgnn_amd import tape
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 63, 64, 65, 200):
        ids = [int(v) for v in rng.integers(1, 1 << 31, n)]
        k = tape.set_key_np(ids)
        assert isinstance(k, int) and 0 <= k <= MASK64 and k == _key(ids)
        assert tape.set_key_np(ids[::-1]) == k and tape.set_key_np(np.asarray(ids)[rng.permutation(n)]) == k
    assert len({tape.set_key_np(s) for s in ([1, 2], [1, 2, 2], [1, 2, 3])}) == 3
    assert tape.set_key_np([2, 1, 2]) == tape.set_key_np([1, 2, 2])
    assert tape.set_key_np([]) == _mix64(0x8CB92BA72F3D8DD7) == tape.set_key_np(np.zeros(0, dtype=np.int64))
    assert tape.set_key_np([]) != tape.set_key_np([0])
    assert any(tape.set_key_np([v]) >= 1 << 63 for v in range(1, 9))            # keys use all 64 bits
    assert int(tape.mix64_np(np.uint64(12345))) == _mix64(12345)


def test_split_codes_are_additive():
    from subgnn_amd import tape
    from oracle import tape as T
    assert tape.SPLIT_CODE['predict'] == 3
    assert {k: tape.SPLIT_CODE[k] for k in ('train', 'val', 'test')} == {'train': 0, 'val': 1, 'test': 2} == T.SPLIT_CODE
    assert len(set(tape.SPLIT_CODE.values())) == 4
    assert tape.stream_id(tape.STREAM_N_INT, 'predict', 1, 2) == T.stream_id(T.STREAM_N_INT, 3, 1, 2)
    assert tape.stream_id(tape.STREAM_N_INT, 'test', 1, 2) == T.stream_id(T.STREAM_N_INT, 'test', 1, 2)


def test_cli_argument_rules(capsys):
    from subgnn_amd import predict
    base = ['-config_path', 'c.json', '-restoreModelPath', 'run', '-subgraphs', 'in.txt', '-out', 'out.txt']
    a = predict.parse_args(base)
    assert (a.config_path, a.restoreModelPath, a.subgraphs, a.out) == ('c.json', 'run', 'in.txt', 'out.txt')
    assert a.restoreModelName is None and a.embeddings is None and a.batch_size is None and a.project_root is None
    a = predict.parse_args(base + ['-restoreModelName', 'last.ckpt', '-embeddings', 'e.npy', '-batch_size', '7'])
    assert (a.restoreModelName, a.embeddings, a.batch_size) == ('last.ckpt', 'e.npy', 7)
    for drop in ('-config_path', '-restoreModelPath', '-subgraphs', '-out'):        # the four required arguments
        i = base.index(drop)
        with pytest.raises(SystemExit):
            predict.parse_args(base[:i] + base[i + 2:])
    for bad in (['-batch_size', '0'], ['-batch_size', '-3'], ['-embeddings', 'e.txt'], ['-embeddings', 'out.txt'],
                ['-noSuchFlag']):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
    with pytest.raises(SystemExit):
        predict.parse_args(base[:-1] + ['in.txt'])                                  # -out over the request file
    capsys.readouterr()


def test_label_names_and_request_files(tmp_path):
    from subgnn_amd import predict
    from subgnn_amd.subgraph_utils import label_names, read_subgraphs
    f = tmp_path / 'subgraphs.pth'
    f.write_text('0-1-2\tliver\ttrain\t\n3-4\tbrain-liver\tval\t\n5\theart\ttest\t\n')
    assert label_names(f) == ['liver', 'brain', 'heart']
    tr, tr_lab, va, va_lab, te, te_lab = read_subgraphs(f)                          # the numbering read_subgraphs gives
    assert tr_lab == [[0]] and va_lab == [[1, 0]] and te_lab == [[2]] and tr == [[0, 1, 2]]
    r = tmp_path / 'requests.txt'
    r.write_text('7-8-9\n\n10\tsome-label\ttrain\t\n11-12-\n')
    assert predict.read_requests(r) == [[7, 8, 9], [10], [11, 12]]


def test_output_line_format():
    from subgnn_amd import predict
    p = np.asarray([0.25, 1.0 / 3.0, 1e-8], dtype=np.float32)
    line = predict.format_line([7, 8, 9], ['brain', 'liver'], p)
    nodes, labels, probs = line.split('\t')
    assert nodes == '7-8-9' and labels == 'brain-liver' and '\n' not in line
    assert np.array_equal(np.asarray([float(x) for x in probs.split(',')], dtype=np.float32), p)      # float32 round trip
    assert predict.format_line([3], ['2'], p[:1]) == '3\t2\t0.25'
    assert predict.format_line([3], [], p[:1]).split('\t') == ['3', '', '0.25']     # a multi-label row with nothing above 0.5

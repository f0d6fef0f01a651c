"""CPU: subgnn_amd/scoring.py and subgnn_amd/cli.py, what explain, suggest and discover share -- the target rule and its
refusals, the statistics over draws at the shapes where they branch, the target's column, the CLI prelude.  CPU tensors, no GPU."""
import argparse

import numpy as np
import pytest
import torch

from subgnn_amd import cli, scoring


def _stand_in(multilabel, label_names=('a', 'b', 'c')):
    class P:
        class model:
            pass

        @staticmethod
        def _probabilities(z):
            return torch.sigmoid(z) if multilabel else torch.softmax(z, dim=-1)

        @staticmethod
        def names_of(row):
            return ['L%s' % row.tolist()]
    P.model.multilabel = multilabel
    P.label_names = None if label_names is None else list(label_names)
    return P


# ---- scoring --------------------------------------------------------------------------------------------------------------------
def test_positive_takes_whole_positive_numbers_only():
    assert scoring.positive(3, 'draws') == 3 and scoring.positive(2.0, 'draws') == 2 and scoring.positive(np.int64(5), 'x') == 5
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='draws must be a positive integer'):
            scoring.positive(bad, 'draws')


def test_class_targets_default_is_the_argmax_of_the_mean_over_draws():
    E, R, K = 2, 3, 4
    base = torch.zeros(E, R, K)
    base[0, :, 1] = 1.0                                               # draw 0 alone says class 1 everywhere
    base[1, 0, 2], base[1, 1, 3], base[1, 2, 0] = 3.0, 3.0, 3.0       # the mean says 2, 3, 0
    assert base[0].argmax(dim=-1).tolist() == [1, 1, 1]
    tgt = scoring.class_targets(None, base, R, K, base.device)
    assert tgt.dtype == torch.int64 and tgt.tolist() == [2, 3, 0]


def test_class_targets_given_and_refused():
    E, R, K = 2, 3, 4
    base, dev = torch.zeros(E, R, K), torch.device('cpu')
    for given, want in ((2, [2, 2, 2]), (np.int32(0), [0, 0, 0]), ([3, 0, 1], [3, 0, 1]), (np.array([0, 3, 3]), [0, 3, 3])):
        tgt = scoring.class_targets(given, base, R, K, dev)
        assert tgt.dtype == torch.int64 and tgt.shape == (R,) and tgt.tolist() == want
    for bad in ([0, 1], [0, 1, 2, 3], 1.0, [0.0, 1.0, 2.0], [[0, 1, 2]], np.zeros((3, 1), dtype=np.int64)):
        with pytest.raises(ValueError, match='^target: an int or 3 ints$'):
            scoring.class_targets(bad, base, R, K, dev)
    for bad in (-1, K, [0, -1, 1], [0, 1, K]):
        with pytest.raises(ValueError, match=r'^target outside the classes 0 \.\. 3$'):
            scoring.class_targets(bad, base, R, K, dev)


def test_mean_std_at_one_draw_no_column_and_the_plain_case():
    x = torch.tensor([[1.5, -2.0]])
    mean, std = scoring.mean_std(x)
    assert torch.equal(mean, x[0]) and std.dtype == torch.float32 and torch.equal(std, torch.zeros(2))
    mean, std = scoring.mean_std(torch.zeros(3, 0))
    assert mean.shape == (0,) and std.shape == (0,) and mean.dtype == std.dtype == torch.float32
    x = torch.tensor([[1.0, 4.0], [2.0, 4.5], [4.0, 8.0]])
    mean, std = scoring.mean_std(x)
    assert torch.equal(mean, x.mean(dim=0)) and torch.equal(std, torch.std(x, dim=0, unbiased=True))
    assert std.tolist() == pytest.approx([np.std([1, 2, 4], ddof=1), np.std([4, 4.5, 8], ddof=1)], rel=1e-6)


@pytest.mark.parametrize('multilabel', [False, True])
def test_target_columns_are_plain_indexing(multilabel):
    E, n, K = 2, 3, 4
    z = torch.randn(E, n, K, generator=torch.Generator().manual_seed(5))
    tgt = torch.tensor([3, 0, 2])
    zt, pt = scoring.target_columns(_stand_in(multilabel), z, tgt)
    prob = torch.sigmoid(z) if multilabel else torch.softmax(z, dim=-1)
    assert zt.shape == pt.shape == (E, n)
    for e in range(E):
        for i in range(n):
            assert zt[e, i] == z[e, i, tgt[i]] and pt[e, i] == prob[e, i, tgt[i]]


def test_a_difference_of_equal_columns_prints_a_plain_zero():
    from subgnn_amd import explain
    z = torch.tensor([[[0.5, -1.25]], [[2.0, 0.75]]])                 # (E = 2, n = 1, K = 2)
    zt, pt = scoring.target_columns(_stand_in(False), z, torch.tensor([1]))
    d_logit, d_std = scoring.mean_std(zt - zt)                        # explain's base - var
    d_prob = (pt - pt).mean(dim=0)
    assert explain.format_line(0, [7], d_logit[0], d_std[0], d_prob[0], ['a']) == '0\t7\t0\t0\t0\ta'
    assert explain.format_line(0, [7], -d_logit[0], 0.0, 0.0, ['a']).split('\t')[2] == '-0'          # what a flipped sign would print


# ---- cli ------------------------------------------------------------------------------------------------------------------------
def _parser():
    ap = argparse.ArgumentParser()
    cli.add_run_arguments(ap)
    for name in ('draws', 'top', 'batch_size'):
        ap.add_argument('-' + name, type=int, default=None)
    return ap


def test_the_run_arguments_and_their_defaults():
    a = _parser().parse_args(['-config_path', 'c.json', '-restoreModelPath', 'run'])
    assert (a.config_path, a.project_root, a.restoreModelPath, a.restoreModelName) == ('c.json', None, 'run', None)
    a = _parser().parse_args(['-config_path', 'c.json', '-restoreModelPath', 'run', '-project_root', '/p', '-restoreModelName', 'last.ckpt'])
    assert (a.project_root, a.restoreModelName) == ('/p', 'last.ckpt')
    for missing in (['-config_path', 'c.json'], ['-restoreModelPath', 'run']):
        with pytest.raises(SystemExit):
            _parser().parse_args(missing)


def test_require_positive_refuses_zero_and_negatives_and_skips_none(capsys):
    ap = _parser()
    names = ('draws', 'top', 'batch_size')
    cli.require_positive(ap, argparse.Namespace(draws=1, top=None, batch_size=None), names)
    for bad in (0, -2):
        with pytest.raises(SystemExit) as e:
            cli.require_positive(ap, argparse.Namespace(draws=3, top=bad, batch_size=None), names)
        assert e.value.code == 2 and '-top must be positive' in capsys.readouterr().err


def test_parse_splits(capsys):
    ap = _parser()
    assert cli.parse_splits(ap, 'train,val,test') == ('train', 'val', 'test') and cli.parse_splits(ap, 'val,,') == ('val',)
    for bad in ('', ',', 'train,dev'):
        with pytest.raises(SystemExit):
            cli.parse_splits(ap, bad)
        assert '-splits takes a comma-separated list of train, val, test' in capsys.readouterr().err


def test_label_index():
    P = _stand_in(False)
    assert cli.label_index(P, 'b') == 1 and cli.label_index(P, None) is None
    with pytest.raises(SystemExit, match=r"-target: 'z' is no label of the dataset \(\['a', 'b', 'c'\]\)"):
        cli.label_index(P, 'z')
    with pytest.raises(SystemExit, match=r"-target: 'a' is no label of the dataset \(None\)"):
        cli.label_index(_stand_in(False, None), 'a')


def test_predicted_names_follow_the_models_kind():
    row = torch.tensor([-1.0, 2.0, 0.5])
    assert cli.predicted_names(_stand_in(False), row) == ['L1']
    assert cli.predicted_names(_stand_in(True), row) == ['L[False, True, True]']


def test_write_lines_with_and_without_a_header(tmp_path):
    f = tmp_path / 'out.txt'
    cli.write_lines(f, ['a\t1', 'b\t2'], 'h\tk')
    assert f.read_text() == 'h\tk\na\t1\nb\t2\n'
    cli.write_lines(f, (s for s in ('x', 'y')))
    assert f.read_text() == 'x\ny\n'
    cli.write_lines(f, [], 'h')
    assert f.read_text() == 'h\n'
    cli.write_lines(f, [])
    assert f.read_text() == ''

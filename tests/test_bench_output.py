"""bench.py's outputs without a GPU: the one stdout line built from recorded full results (short, strict JSON, the headline
fields), and --dump-outputs on a small CPU model (float32 / float64 files, the same files twice, the size budget)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, REPO)
import bench                                                                     # noqa: E402


def _strict_loads(s):
    def bad(c):
        raise ValueError(c)
    return json.loads(s, parse_constant=bad)


@pytest.mark.parametrize('name', ['r06_final_bench_default.json', 'r06_final_bench_graph.json'])
def test_result_line_is_short_strict_json_with_the_headline(name):
    with open(os.path.join(REPO, 'profiles', name)) as f:
        result = json.load(f)
    line = bench.result_line(result, 'bench_details.json')
    assert '\n' not in line and len(line.encode()) < bench.LINE_MAX_BYTES
    d = _strict_loads(line)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'dtype', 'loss'):
        assert d[k] == result[k], k
    assert d['config']['workload'] == result['config']['workload']
    assert d['config']['schedule'] == result['config']['schedule']
    assert d['roofline']['frac'] == result['roofline']['frac'] and d['roofline']['kernel'] == result['roofline']['kernel']
    if 'cpu_baseline' in result:
        assert d['cpu_baseline']['value'] == result['cpu_baseline']['value']
    assert d['details'] == 'bench_details.json'


def test_result_line_writes_non_finite_numbers_as_null():
    d = _strict_loads(bench.result_line({'metric': 'm', 'value': float('nan'), 'ms_per_step': float('inf'),
                                         'config': {'workload': 'w'}, 'loss': 1.5}))
    assert d['value'] is None and d['ms_per_step'] is None and d['loss'] == 1.5 and 'details' not in d


class _Model(torch.nn.Module):
    def __init__(self, rows, dim):
        super().__init__()
        self.node_embeddings = torch.nn.Embedding(rows, dim)
        self.lin = torch.nn.Linear(dim, 3)


def test_dump_outputs_is_reproducible_and_within_budget(tmp_path):
    torch.manual_seed(0)
    m = _Model(300_000, 64)                                        # 77 MB table: written as a sample of its rows
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(1.25), torch.tensor(0.5), m)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b'))
    assert {'loss.npy', 'accuracy.npy', 'param.lin.weight.npy', 'param.lin.bias.npy', 'param.node_embeddings.weight.npy',
            'param.node_embeddings.weight.sample_rows.npy'} == set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= bench.DUMP_TOTAL_BYTES
    rows = np.load(tmp_path / 'a' / 'param.node_embeddings.weight.sample_rows.npy').astype(np.int64)
    assert len(rows) == bench.DUMP_SAMPLE_BYTES // (4 * 64) and np.all(np.diff(rows) > 0)
    table = np.load(tmp_path / 'a' / 'param.node_embeddings.weight.npy')
    assert np.array_equal(table, m.node_embeddings.weight.detach().numpy()[rows])
    assert np.array_equal(np.load(tmp_path / 'a' / 'param.lin.weight.npy'), m.lin.weight.detach().numpy())
    assert float(np.load(tmp_path / 'a' / 'loss.npy')[0]) == 1.25 and float(np.load(tmp_path / 'a' / 'accuracy.npy')[0]) == 0.5

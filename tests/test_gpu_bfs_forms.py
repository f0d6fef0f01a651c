"""-m gpu: every form the multi-source BFS kernels (msbfs_* in csrc/similarity.hip) take, against the CPU oracle
(oracle.integer_half.bfs_hops_numpy per source; per set the min over its members, 0 where any member is unreached -- the rule
at msbfs_set_finalize_kernel).  One graph with a list the pull levels park for the workgroup (degree >= 512), one only the push
levels park (128 <= degree < 512), short lists, 8+ levels and isolated ids; source counts at every row form: 1 word, a full word,
2 words, 3 words padded to a stride of 4, 4 words unpadded, 5 words (two register chunks; 257 sources leave the second one valid
bit).  Each count runs pushing only (pull_alpha 0), with the default switch (-1) and pulling from level 2 on (1 << 30).
The graph has 1828 ids, the sum of its parts: 1 + 600 and 1 + 200 for the stars, a path of 6, 1000 sparse ids, 20 isolated.
Every source list holds a centre, a leaf and an isolated id -- except the list of one source, which is the centre alone.
Not reachable at this size, and not pinned here: more than 128 parked lists in one workgroup."""
import numpy as np
import pytest
import torch

from oracle.integer_half import bfs_hops_numpy

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CENTRE_A, LEAVES_A = 1, range(2, 602)                      # 600 leaves: degree 601 with the path
CENTRE_B, LEAVES_B = 602, range(603, 803)                  # 200 leaves: degree 201
PATH = range(803, 809)                                     # CENTRE_A - 803 - ... - 808 - CENTRE_B
SPARSE = range(809, 1809)                                  # hung on leaf 2
ISOLATED = range(1809, 1829)
N = 1828
MAX_HOPS = 64
SOURCE_COUNTS = (1, 64, 65, 129, 193, 257, 300)
ALPHAS = (0, -1, 1 << 30)

_cache = {}


def _graph():
    """-> (rowptr, col, sets as lists)"""
    if 'graph' not in _cache:
        from subgnn_amd import synthetic
        rng = np.random.default_rng(21)
        pairs = [(CENTRE_A, v) for v in LEAVES_A] + [(CENTRE_B, v) for v in LEAVES_B]
        chain = [CENTRE_A] + list(PATH) + [CENTRE_B]
        pairs += list(zip(chain[:-1], chain[1:]))
        first = SPARSE[0]
        pairs.append((LEAVES_A[0], first))
        for k in range(1, len(SPARSE)):                    # a random tree over a window of earlier ids, then some chords
            pairs.append((first + k, first + int(rng.integers(max(0, k - 100), k))))
        pairs += [(int(a), int(b)) for a, b in rng.integers(first, SPARSE[-1] + 1, (300, 2)) if abs(int(a) - int(b)) < 50 and a != b]
        rowptr, col = synthetic.sorted_csr(np.asarray(pairs, dtype=np.int64) - 1, N)
        deg = np.diff(rowptr)
        assert deg[CENTRE_A] >= 512 and 128 <= deg[CENTRE_B] < 512
        assert all(deg[v] == 0 for v in ISOLATED) and 1 <= np.median(deg[first:SPARSE[-1] + 1]) <= 4
        srng = np.random.default_rng(22)
        sets = [[CENTRE_A], [CENTRE_B],
                list(LEAVES_A[5:40]),                                           # leaves of one centre
                [LEAVES_A[7], LEAVES_B[3], LEAVES_B[150], CENTRE_A, PATH[2]],   # across both stars
                [LEAVES_B[9], SPARSE[500], ISOLATED[4]],                        # an isolated member: the row is 0
                [ISOLATED[0], ISOLATED[7], ISOLATED[19]],
                []]
        sets += [srng.integers(1, N + 1, int(srng.integers(1, 31))).tolist() for _ in range(60)]
        _cache['graph'] = (rowptr, col, sets)
    return _cache['graph']


def _hops_from(src):
    """The oracle's hops from id ``src`` to ids 0..N, once per distinct id."""
    rowptr, col, _ = _graph()
    memo = _cache.setdefault('hops', {})
    if src not in memo:
        memo[src] = bfs_hops_numpy(rowptr, col, int(src), N)
    return memo[src]


def _case(n_src):
    """-> (sources int32[n_src], hop table uint8 (n_src, N + 1), set values float32 (n_sets, n_src), depth) -- all from the oracle"""
    key = ('case', n_src)
    if key not in _cache:
        _, _, sets = _graph()
        rng = np.random.default_rng(100 + n_src)
        fixed = [CENTRE_A, LEAVES_A[11], ISOLATED[2]][:n_src]                   # (one source: the centre)
        src = np.concatenate([rng.integers(1, N + 1, n_src - len(fixed)), fixed]).astype(np.int32)      # duplicates allowed
        src = src[rng.permutation(n_src)]
        hops = np.stack([_hops_from(int(s)) for s in src])
        want = np.zeros((len(sets), n_src), dtype=np.float32)
        for r, members in enumerate(sets):
            if members:
                h = hops[:, members]
                want[r] = np.where((h == 255).any(1), 0, h.min(1))
        depth = int(hops[hops != 255].max())
        if n_src >= 3:
            assert 8 <= depth < MAX_HOPS - 1                                    # 8+ levels, and the level cap is not met
            assert len(set(want[2].tolist())) > 3 and not want[4].any() and not want[6].any()
        _cache[key] = (src, hops, want, depth)
    return _cache[key]


def _device_graph():
    if 'dg' not in _cache:
        from subgnn_amd import ops
        rowptr, col, sets = _graph()
        _cache['dg'] = (ops.DeviceGraph(rowptr, col, np.arange(1, N + 1, dtype=np.int32), DEV), ops.Ragged.from_lists(sets, DEV))
    return _cache['dg']


@pytest.mark.parametrize('n_src', SOURCE_COUNTS)
def test_hop_table_equals_the_oracle_in_both_layouts(n_src):
    from subgnn_amd import ops
    dg, _ = _device_graph()
    src, hops, _, _ = _case(n_src)
    dsrc = torch.from_numpy(src).to(DEV)
    for alpha in ALPHAS:
        got = ops.bfs_hops(dg, dsrc, max_hops=MAX_HOPS, pull_alpha=alpha).cpu().numpy()
        assert np.array_equal(got, hops), alpha
        got = ops.bfs_hops(dg, dsrc, max_hops=MAX_HOPS, node_major=True, pull_alpha=alpha).cpu().numpy()
        assert np.array_equal(got, hops.T), alpha


@pytest.mark.parametrize('n_src', SOURCE_COUNTS)
def test_set_hops_equal_the_oracle_in_either_form(n_src):
    from subgnn_amd import ops
    dg, dsets = _device_graph()
    src, _, want, depth = _case(n_src)
    dsrc = torch.from_numpy(src).to(DEV)
    for until in ('nodes', 'sets'):
        for alpha in ALPHAS:
            for push_levels in (-1, 1, 2):
                got, st = ops.bfs_min_hops_to_sets(dg, dsrc, dsets, max_hops=MAX_HOPS, want_status=True, pull_alpha=alpha,
                                                   push_levels=push_levels, until=until)
                where = (until, alpha, push_levels)
                st = st.tolist()
                assert np.array_equal(got.cpu().numpy(), want), where
                assert st[1] == 0, where
                if until == 'nodes':
                    assert st[0] == depth, where

"""-m gpu: scoring.variant_logits, the chunked draw loop under explain, suggest and discover, against a stand-in predictor whose
"logits" say what every call was given: a set's content and draw, the chunk's ``max_len``, the set's key.  Whatever the chunk
size, every set keeps its row, its key and its draw, and a chunk carries its own largest length.  Small integers held in
float32: every comparison is exact.  No model."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = (1, 3, 2, 4, 1)
K = 3


class _StandIn:
    """``draw_logits`` -> per set [sum of ids + draw, chunk.max_len, low 20 bits of its key]; checks that a chunk is a Ragged of
    its own (ptr from 0, its own nodes, one key per set) and keeps what it was called with."""

    def __init__(self):
        self.calls = []

    def draw_logits(self, chunk, draw, batch_size=None, sub_keys=None):
        assert chunk.ptr.is_contiguous() and chunk.nodes.is_contiguous() and sub_keys.is_contiguous()
        assert int(chunk.ptr[0]) == 0 and int(chunk.ptr[-1]) == chunk.nodes.numel() and sub_keys.shape == (chunk.n,)
        self.calls.append((chunk.n, draw, batch_size))
        run = torch.zeros(chunk.nodes.numel() + 1, dtype=torch.int64, device=chunk.nodes.device)
        torch.cumsum(chunk.nodes.long(), 0, out=run[1:])
        sums = run[chunk.ptr[1:]] - run[chunk.ptr[:-1]]
        return torch.stack((sums + draw, torch.full_like(sums, chunk.max_len), sub_keys & 0xFFFFF), dim=1).float()


@pytest.fixture(scope='module')
def case():
    from subgnn_amd import ops
    lists, v = [], 1
    for n in LENGTHS:
        lists.append(list(range(v, v + n)))
        v += n + 7
    sets = ops.Ragged.from_lists(lists, DEV)
    return sets, ops.set_keys(sets), lists


@pytest.mark.parametrize('draws', [1, 3])
@pytest.mark.parametrize('max_variants', [1, 2, 5, 6])
def test_chunks_keep_rows_keys_and_draws_and_carry_their_own_max_len(case, max_variants, draws):
    from subgnn_amd import ops, scoring
    sets, keys, lists = case
    V = len(LENGTHS)
    whole = ops.Ragged(sets.ptr, sets.nodes[:sum(LENGTHS)].contiguous(), max_len=max(LENGTHS))
    ref = torch.stack([_StandIn().draw_logits(whole, d, None, sub_keys=keys) for d in range(draws)])
    p = _StandIn()
    got = scoring.variant_logits(p, sets, keys, K, draws, 7, max_variants)
    assert got.shape == (draws, V, K) and got.dtype == torch.float32 and got.device == ref.device
    assert torch.equal(got[:, :, 0], ref[:, :, 0]) and torch.equal(got[:, :, 2], ref[:, :, 2])
    # written out: the sums with their draw, the largest length of every set's chunk, the keys' low bits
    want0 = [[float(sum(s) + d) for s in lists] for d in range(draws)]
    want1 = [float(max(LENGTHS[lo:lo + max_variants])) for lo in range(0, V, max_variants) for _ in LENGTHS[lo:lo + max_variants]]
    assert got[:, :, 0].tolist() == want0
    assert got[:, :, 1].tolist() == [want1] * draws
    assert got[0, :, 2].tolist() == [float(k & 0xFFFFF) for k in keys.tolist()]
    assert len(set(got[0, :, 2].tolist())) == V                       # (the keys tell the sets apart)
    assert p.calls == [(min(max_variants, V - lo), d, 7) for lo in range(0, V, max_variants) for d in range(draws)]


@pytest.mark.parametrize('draws', [1, 3])
def test_no_set_no_call(draws):
    from subgnn_amd import ops, scoring
    empty = ops.Ragged(torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    p = _StandIn()
    got = scoring.variant_logits(p, empty, torch.empty(0, dtype=torch.int64, device=DEV), K, draws, None, 4)
    assert got.shape == (draws, 0, K) and got.dtype == torch.float32 and p.calls == []

"""What ``explain``, ``suggest`` and ``discover`` share: variants of requests are sent through the model at every draw, and the
target class's column of the answer is reduced over the draws.  One copy of the argument rules, of the chunked draw loop and
of the statistics; each caller builds its variants, scores them here and lays its own result out."""
import numpy as np
import torch

from . import ops


def positive(value, name):
    if isinstance(value, bool) or int(value) != value or int(value) <= 0:
        raise ValueError('%s must be a positive integer' % name)
    return int(value)


def class_targets(target, base, R, K, device):
    """The class per request -> (R,) int64: the argmax of the mean of the base logits ``base`` (E, R, K), or the given int or
    sequence of R ints inside 0 .. K - 1."""
    if target is None:
        return base.mean(dim=0).argmax(dim=-1)
    t = np.asarray(target)
    if t.dtype.kind not in 'iu' or t.ndim > 1 or (t.ndim == 1 and t.shape[0] != R):
        raise ValueError('target: an int or %d ints' % R)
    t = np.broadcast_to(t.astype(np.int64), (R,)).copy()
    if t.min() < 0 or t.max() >= K:
        raise ValueError('target outside the classes 0 .. %d' % (K - 1))
    return torch.from_numpy(t).to(device)


def variant_logits(p, sets, keys, K, draws, batch_size, max_variants):
    """The float32 logits (draws, V, K) of the V device sets ``sets`` (a Ragged; ``keys``: their content keys) at the draws
    0 .. draws - 1, prepared and forwarded in chunks of at most ``max_variants`` sets.  Every chunk carries its own largest
    length; ``sets.ptr`` is read to the host once.  No set: no forward pass."""
    V, dev = sets.n, sets.ptr.device
    out = torch.empty((draws, V, K), dtype=torch.float32, device=dev)
    if V == 0:
        return out
    vptr = sets.ptr.cpu().numpy()
    for lo in range(0, V, max_variants):
        hi = min(lo + max_variants, V)
        a, b = int(vptr[lo]), int(vptr[hi])
        chunk = ops.Ragged((sets.ptr[lo:hi + 1] - a).contiguous(), sets.nodes[a:b].contiguous(),
                           max_len=int((vptr[lo + 1:hi + 1] - vptr[lo:hi]).max()))
        sub = keys[lo:hi].contiguous()
        for d in range(draws):
            out[d, lo:hi] = p.draw_logits(chunk, d, batch_size, sub_keys=sub)
    return out


def target_columns(p, z, tgt):
    """Of the logits ``z`` (E, n, K) the column ``tgt`` (n,) of every row, and the same column of their probabilities
    (softmax; sigmoid for a multi-label model) -> two (E, n) tensors."""
    pick = tgt.view(1, -1, 1).expand(z.shape[0], -1, 1)
    return z.gather(2, pick).squeeze(2), p._probabilities(z).gather(2, pick).squeeze(2)


def mean_std(x):
    """Of ``x`` (E, n) the mean over draws and the sample standard deviation (zeros for one draw) -> two (n,) tensors."""
    E, n = x.shape
    if E > 1 and n > 0:
        return x.mean(dim=0), x.std(dim=0, unbiased=True)
    return x.mean(dim=0), torch.zeros(n, dtype=torch.float32, device=x.device)

"""Counter-based draw tape, host side (twin of the device functions in csrc/common.h).

Randomness in the sampling kernels is a pure function  draw64(seed, stream, item, j):
``seed`` the run seed, ``stream`` which sampler / split / layer is drawing, ``item`` the
independent unit (walk number, row * slots + slot, subgraph number), ``j`` that unit's own
draw counter (the neighbourhood anchors use two: draw 0 = rank of the pick among the row's
ascending entries, draw 1 = the "every variate negative" event of the PAD rule).  It replaces the three global
serial RNG streams of the reference (anchor_patch_samplers.py:70-106,177,189,206-222,326),
which cannot be consumed in parallel; see DESIGN.md "Draw tape".
"""
MASK64 = (1 << 64) - 1

STREAM_STRUCT_START = 1
STREAM_STRUCT_PATCH = 2
STREAM_WALK_INT = 3
STREAM_WALK_BOR = 4
STREAM_N_INT = 5
STREAM_N_BOR = 6
STREAM_P_INT = 7
STREAM_P_EXT = 8
STREAM_S_PICK = 9
# node-embedding pre-training (train_node_emb.py): edge split, negative pairs, dropout masks
STREAM_NE_SPLIT = 10
STREAM_NE_NEG = 11
STREAM_NE_DROP = 12
# candidate subgraphs around seed nodes (discover.py, ops.seeded_walk_sets): the item is the candidate's number
STREAM_DISCOVER = 13

# 'predict': requests outside the dataset (predict.py); their draws are keyed by content (set_key_np), not by row number
SPLIT_CODE = {'train': 0, 'val': 1, 'test': 2, 'predict': 3}


def stream_id(kind, split=0, layer=0, epoch=0):
    """``epoch``: resample epoch (resample_anchor_patches draws fresh anchors after every validation
    epoch, SubGNN.py:453-460); 0 for the draws of prepare_data / prepare_test_data."""
    if isinstance(split, str):
        split = SPLIT_CODE[split]
    assert 0 <= layer < 256 and 0 <= epoch < 65536
    return (kind << 32) | (split << 24) | (epoch << 8) | layer


def draw64_np(seed, stream, item, j):
    """draw64 over numpy arrays of ``item`` / ``j`` (uint64 wrap-around arithmetic): host-side draws of one-time set-up work
    (the node-embedding trainer's edge split)."""
    import numpy as np
    K_STREAM, K_ITEM, K_DRAW = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7

    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over='ignore'):
        h0 = mix(np.uint64((seed & MASK64) ^ ((stream * K_STREAM) & MASK64)))
        h = mix(h0 + np.asarray(item).astype(np.uint64) * np.uint64(K_ITEM))
        return mix(h + np.asarray(j).astype(np.uint64) * np.uint64(K_DRAW))


def mix64_np(z):
    """sgnn_mix64 (csrc/common.h) over a numpy uint64 array."""
    import numpy as np
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def set_key_np(ids):
    """Content key of a set of node ids (twin of sgnn_set_keys, include/subgnn_hip.h): independent of the order of the entries,

        key = mix64( sum_v mix64(v)  +  (n + 1) * 0x8CB92BA72F3D8DD7 )      (uint64 wrap-around; n = number of entries)

    so a repeated entry changes the key (sum and n both move) and the empty set has the key mix64(0x8CB92BA72F3D8DD7)."""
    import numpy as np
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    with np.errstate(over='ignore'):
        total = mix64_np(ids.astype(np.uint64) & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64) if ids.size else np.uint64(0)
        return int(mix64_np(np.uint64(total) + np.uint64(ids.size + 1) * np.uint64(0x8CB92BA72F3D8DD7)))

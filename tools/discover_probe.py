#!/usr/bin/env python3
"""The seeded walk kernel and ``Predictor.discover``, timed on the benchmark's synthetic graph (BA 1M nodes / m = 10; the model
of tools/suggest_probe.py, prepared on the benchmark's 50k training subgraphs).

  * the kernel alone: 2^20 items (65536 seeds x 16) at target sizes 8, 16 and 64, restart 0.15, 16 x size steps at most.  The
    entry is called on outputs allocated once; device events around every launch on an otherwise idle stream; after a warm-up
    the median of ``reps`` launches.  Steps per second = the sum of out_steps over that time.
  * resident wavefronts per SIMD, from the registers and LDS the code object declares (tools/kernel_resources.py);
  * one ``discover`` call over 4096 seeds x 16 candidates of size 8: wall clock around device synchronisations, split into
    sampling (ops.seeded_walk_sets), preparation (Predictor.prepare_sets) and forward (Predictor.forward_prepared);
  * the numpy / Python-int definition (tests/discover_cases.py) on this machine's CPU for the first ``host_items`` items of the
    size-8 launch, checked against the kernel's rows bit for bit.  A sanity figure, not a target.
No threshold: nobody had measured any of these numbers.
    python tools/discover_probe.py [reps] [out.json] [host_items]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import numpy as np
import torch
import bench
import discover_cases as DC
import kernel_resources as KR
from subgnn_amd import _lib, build, hotpath, ops, synthetic, tape
from subgnn_amd.SubGNN import SubGNN
from subgnn_amd.predict import Predictor

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
host_items = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
n, m, S, D = 1_000_000, 10, 50_000, 64
N_SEEDS, PER_SEED, SIZES = 65536, 16, (8, 16, 64)
CHUNK = 16384             # candidates per prepared chunk, as tools/suggest_probe.py: a chunk's borders go through one device sort
dev = torch.device('cuda:0')
STREAM = tape.stream_id(tape.STREAM_DISCOVER, 'predict')


def stage(what):
    print('[discover_probe] ' + what, file=sys.stderr, flush=True)


def occupancy():
    """Wavefronts per SIMD the kernel's registers and LDS allow (MI355X: 512 VGPRs per SIMD lane allocated in eights, 8
    wavefronts at most, 160 KiB of LDS per compute unit of four SIMDs; a workgroup of this kernel is one wavefront)."""
    obj = os.path.join(build.LIBDIR, 'seeded_sets.o')
    with tempfile.TemporaryDirectory() as tmp:
        if not os.path.exists(obj):                                   # (a tree with the library but not its objects: this one file again)
            obj = os.path.join(tmp, 'seeded_sets.o')
            subprocess.check_call([build._hipcc(), '--offload-arch=' + build.ARCH, '-O3', '-fPIC', '-std=c++17', '-c',
                                   os.path.join(build.CSRC, 'seeded_sets.hip'), '-o', obj])
        k = next(k for k in KR.kernels(obj) if 'seeded_walk_kernel' in k['demangled'])
    alloc = -(-k['vgpr_count'] // 8) * 8
    lds = k['group_segment_fixed_size']
    by_lds = (160 * 1024 // lds) // 4 if lds else 8
    return {'vgprs': k['vgpr_count'], 'sgprs': k['sgpr_count'], 'lds_bytes': lds, 'vgpr_spills': k['vgpr_spill_count'],
            'scratch_bytes': k['private_segment_fixed_size'], 'waves_per_simd': min(8, 512 // alloc, by_lds)}


stage('building the graph')
edges = synthetic.barabasi_albert_edges(n, m, seed=42)
rowptr, col = synthetic.sorted_csr(edges, n)
g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), dev)
res = {'graph_nodes': n, 'graph_m': m, 'seeds': N_SEEDS, 'per_seed': PER_SEED, 'items': N_SEEDS * PER_SEED, 'restart': 0.15,
       'reps': reps, 'kernel': occupancy()}

stage('the kernel alone')
lib = _lib.load()
seeds_np = np.random.default_rng(7).choice(np.arange(1, n + 1), size=N_SEEDS, replace=False).astype(np.int32)
seeds = torch.from_numpy(seeds_np).to(dev)
V = N_SEEDS * PER_SEED
thr = ops.restart_threshold(0.15)
first_rows = None
for size in SIZES:
    sizes = torch.full((PER_SEED,), size, dtype=torch.int32, device=dev)
    nodes = torch.empty((V, size), dtype=torch.int32, device=dev)
    lens, steps = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    keys = torch.empty(V, dtype=torch.int64, device=dev)

    def launch():
        ops.check(lib.sgnn_seeded_walk_sets(ops._ptr(g.rowptr), ops._ptr(g.col_sorted), g.max_id, ops._ptr(seeds), N_SEEDS,
                                            ops._ptr(sizes), PER_SEED, size, thr, 16 * size, 0, STREAM, 0, None, V, ops._ptr(nodes),
                                            ops._ptr(lens), ops._ptr(steps), ops._ptr(keys), ops._stream()), 'sgnn_seeded_walk_sets')
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = statistics.median(times)
    total_steps = int(steps.sum(dtype=torch.int64))
    res['size_%d' % size] = {'kernel_ms': round(ms, 3), 'kernel_ms_min': round(min(times), 3), 'kernel_ms_max': round(max(times), 3),
                             'steps': total_steps, 'steps_per_s': round(total_steps / (ms * 1e-3)), 'items_per_s': round(V / (ms * 1e-3)),
                             'mean_len': round(float(lens.float().mean()), 3), 'full_size_share': round(float((lens == size).float().mean()), 4)}
    stage('size %d: %s' % (size, res['size_%d' % size]))
    if first_rows is None:
        first_rows = {'nodes': nodes[:host_items].cpu().numpy(), 'len': lens[:host_items].cpu().numpy(),
                      'steps': steps[:host_items].cpu().numpy(), 'keys': keys[:host_items].cpu().numpy().view(np.uint64)}

stage('the definition on the host, %d items' % host_items)
t0 = time.perf_counter()
want = DC.sample(rowptr, g.col_sorted.cpu().numpy(), seeds_np, np.full(PER_SEED, SIZES[0], dtype=np.int32), PER_SEED, SIZES[0], thr,
                 16 * SIZES[0], 0, STREAM, n_items=host_items)
host_s = time.perf_counter() - t0
assert all(np.array_equal(first_rows[k], want[k]) for k in want), 'the kernel and the definition differ'
res['host_definition'] = {'items': host_items, 'seconds': round(host_s, 3), 'steps': int(want['steps'].sum()),
                          'steps_per_s': round(int(want['steps'].sum()) / host_s), 'bit_equal': True}

stage('preparing the model')
train = synthetic.bfs_subgraphs(rowptr, col, S, 20, seed=1000)
torch.manual_seed(0)
hp = dict(bench.ALL_DENSITY_HP)
hp['node_embed_size'] = D
labels = torch.randint(0, 3, (S,), generator=torch.Generator().manual_seed(0))
model = SubGNN.from_memory(hp, g, {'train': train, 'val': [], 'test': []},
                           {'train': labels, 'val': labels[:0], 'test': labels[:0]}, torch.randn(n, D, device=dev), num_classes=3)
hotpath.prepare_sparse(model, 'train')
torch.cuda.synchronize()
P = Predictor(model)
spent = {}


def timed(name, fn):
    def wrapped(*a, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        spent[name] = spent.get(name, 0.0) + (time.perf_counter() - t) * 1e3
        return out
    return wrapped


stage('discover over 4096 seeds x 16')
pick = [int(v) - 1 for v in seeds_np[:4096]]
call = lambda: P.discover(pick, sizes=(8,), per_seed=16, target=0, top=100, max_variants=CHUNK)
call()                                                                # the freeze, the known keys, the code objects
walk, prep, fwd = ops.seeded_walk_sets, P.prepare_sets, P.forward_prepared
ops.seeded_walk_sets, P.prepare_sets, P.forward_prepared = timed('sampling_ms', walk), timed('preparation_ms', prep), timed('forward_ms', fwd)
try:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = call()
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
finally:
    ops.seeded_walk_sets = walk
    del P.prepare_sets, P.forward_prepared
res['discover_4096x16'] = dict({k: round(v, 3) for k, v in spent.items()}, total_ms=round(total, 3), n_sampled=got['n_sampled'],
                               n_distinct=got['n_distinct'], max_variants=CHUNK, rest_ms=round(total - sum(spent.values()), 3))
print(json.dumps(res))
if out_file:
    with open(out_file, 'w') as f:
        f.write(json.dumps(res, indent=1) + '\n')

#!/usr/bin/env python3
"""Benchmark of the SubGNN hot path on MI355X.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[3], the one the 1/2/4/8-GPU metric is quoted on): synthetic
DENSITY-style base graph, Barabasi-Albert n = 1M, m = 10 (10M undirected edges), BFS subgraphs
of 20 nodes, embeddings (N, 64) fp32 random, hyper-parameters
best_model_hyperparameters/density/all_density_hyperparams.json (all three channels, 1 layer,
N 10/43, P 57/183, S 42) with max_sim_epochs = 5 and a 1-hop neighbourhood border (what the
reference effectively uses when ego_graphs.txt is present).
  --scaling weak   (default) 50k subgraphs PER GPU: the shard is the unit, per-GPU work is fixed;
  --scaling strong 50k subgraphs IN TOTAL, dealt to the ranks in contiguous blocks; the shared
                   per-layer work (the position channel's BFS sources) is dealt across ranks too.

One step = one full pass of the hot path over the rank's shard, everything on the GPU:
  anchor-patch sampling + similarities (connected components, k-hop border BFS, N/P/S anchor
  draws, structure patches + triangular walks, degree sequences, DTW, multi-source BFS
  position similarities)  ->  three channels forward  ->  read-out + MLP head + loss  ->  backward  ->
  [N>1: all-reduce of the small gradients; reduce-scatter of the embedding-table gradient,
   owner-computes Adam, all-gather of the updated rows under the next pass]  ->  Adam step.
  N>1, --head sharded (default): every rank runs the head on ITS subgraphs; the loss is the mean over the global
       batch (equal shards: the mean of the ranks' means), so all gradients are averaged over ranks.
  N>1, --head replicated: north_star's exchange -- an RCCL all-gather of the per-component channel embeddings
       (84 MB per rank) and the head replicated on the global batch; what batch_norm / a consumer that needs
       every rank's embeddings requires, at world x the head work per rank.
value = subgraphs processed by all ranks / max-over-ranks step time.

Prints ONE short JSON line on rank 0: metric, value, ms_per_step, config, roofline and cpu_baseline in brief (result_line).
The full result object is written to --details (default bench_details.json).  A plain run only sets up, primes, warms up, times
the --steps steps, writes --dump-outputs and prints the line; --full also measures, after the timed steps, these extra objects
(and the north_star exchange of ``collectives`` at N > 1):
  roofline      the structure-channel CSR gather (sgnn_degree_sequence, the kernel BASELINE.json's target names) AS THE PASS RUNS
                IT (lists of >= 512 entries answered from their membership bitmaps): the bytes that launch reads / its time inside the timed region, peak
                8 TB/s; streaming_form beside it = the launch that moves SURVEY.md 8(d)'s algorithmic bytes (every neighbour list
                streamed), 20 launches back to back, HIP events on the launching stream, with the memory-side counter traffic
                (hbm_frac) from the committed rocprofv3 passes.
  rooflines     the other HBM-class kernels of the pass priced the same way (one-hop border + draw, position BFS).
  projection    N = 1 only: 8-GPU estimates from THIS run's measurements + bytes / link rate; not a measurement.  weak_*: from the
                sequential two-stream schedule N > 1 runs by default, timed live (sequential_ms_per_step); strong_*: from shard6250.
  shard6250     N = 1 only: rank 0's 6 250-subgraph block of the 50k (BASELINE configs[3] as worded), timed in this process.
  configs       N = 1 only: the batch-sized training steps of the BASELINE configs[0,1,2,4] stand-ins (replayed + eager ms, kernels).
  cpu_baseline  the oracle (plain C + numpy + torch-CPU restatement of the same algorithm) timed on this box's host cores on a
                bounded sample (rank 0, N = 1 only; Python stages on worker processes forked before the GPU is initialised), with
                its calibration against the imported reference (profiles/r06_cpu_calibration.json; round 4: r04_cpu_calibration.json).
--dump-outputs DIR writes what the last timed step computed (loss, accuracy, the updated parameters) as .npy files, so that
two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0

ALL_DENSITY_HP = {          # reference best_model_hyperparameters/density/all_density_hyperparams.json
    "use_neighborhood": True, "use_structure": True, "use_position": True, "seed": 0,
    "node_embed_size": 64, "structure_patch_type": "triangular_random_walk", "lstm_aggregator": "last",
    "n_processes": 4, "resample_anchor_patches": False, "freeze_node_embeds": False,
    "use_mpn_projection": True, "compute_similarities": True, "sample_walk_len": 50,
    "n_triangular_walks": 5, "random_walk_len": 10, "rw_beta": 0.65, "batch_size": 64,
    "learning_rate": 0.0002951850045886519, "grad_clip": 0.1929946246623414, "n_layers": 1,
    "neigh_sample_border_size": 1, "n_anchor_patches_pos_out": 183, "n_anchor_patches_pos_in": 57,
    "n_anchor_patches_N_in": 10, "n_anchor_patches_N_out": 43, "n_anchor_patches_structure": 42,
    "linear_hidden_dim_1": 64, "linear_hidden_dim_2": 64, "lin_dropout": 0.2522849803237359,
    "lstm_dropout": 0.0, "lstm_n_layers": 1, "cc_aggregator": "max", "trainable_cc": False,
    "max_sim_epochs": 5, "embedding_type": "gin",
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--subgraphs', type=int, default=50_000, help='subgraphs per GPU (weak) / in total (strong)')
    ap.add_argument('--scaling', choices=['weak', 'strong'], default='weak')
    ap.add_argument('--no-pipeline', action='store_true',
                    help='prepare every pass after the previous one has finished training (default: the sampling + similarity '
                         'half of pass k+1 runs on a second HIP stream while pass k trains: hotpath.PassPipeline)')
    ap.add_argument('--pipeline-depth', type=int, default=2,
                    help='prepared passes in flight under the pipeline: with 2 the preparation stream (the longer chain) is '
                         'never idle while the host installs a pass and queues its training half')
    ap.add_argument('--graph', choices=['auto', 'off', 'train', 'both'], default='auto', nargs='?', const='train',
                    help='N=1: what is replayed from hipGraphs.  train: the training half (hotpath.CapturedTraining; every prepared pass '
                         'is copied into the recording\'s tensors); both: preparation AND training half, two alternating slots, no '
                         'copies (hotpath.GraphedPasses: bit-equal, but a recorded two-stream preparation replays SLOWER than the eager one '
                         'on this runtime -- 4.5 ms); off: everything queued eagerly; auto (default): train for shards of up to 16 384 '
                         'subgraphs -- where the pass is bound by the host\'s ~265 launches (6 250 subgraphs: 4.4-4.7 ms eager) -- and off '
                         'above (50k subgraphs: the device is the bound, 9.5 ms either way).  '
                         'All forms are bit-equal (tests/test_gpu_hotpath.py)')
    ap.add_argument('--pipeline-multi', action='store_true',
                    help='N>1, weak scaling: pipeline the passes as at N=1 (the prepared pass reduces its padded widths on its '
                         'own communicator while the pass in training exchanges gradients)')
    ap.add_argument('--head', choices=['sharded', 'replicated'], default='sharded',
                    help='N>1: the read-out + MLP head on the rank\'s own rows (gradients averaged), or replicated on the '
                         'all-gathered channel embeddings')
    ap.add_argument('--subgraph-nodes', type=int, default=20)
    ap.add_argument('--embed', type=int, default=64)
    ap.add_argument('--embedding-dtype', choices=['fp32', 'fp16'], default='fp32',
                    help="fp16: the fused kernels read an IEEE-half copy of the embedding table (fp32 accumulate, fp32 master)")
    ap.add_argument('--full', action='store_true',
                    help='measure everything beside the headline too: the rooflines, the N>1 north_star exchange, and at N=1 the '
                         'extras, the projection and the CPU baseline (without it a run sets up, warms up, times the steps, '
                         'dumps its outputs if asked and prints the line)')
    ap.add_argument('--no-extras', action='store_true',
                    help='with --full, N=1: skip what is measured beside the headline in the same run -- the sequential two-stream '
                         'schedule (what N>1 runs by default: the projection is computed from it), the live 6 250-subgraph '
                         'strong-scaling shard, and the batch-sized training steps of the BASELINE configs[0,1,2,4] stand-ins (the '
                         '``configs`` object)')
    ap.add_argument('--extras-budget-s', type=float, default=100.0, help='wall-clock budget of the stand-in configurations')
    ap.add_argument('--strong-rank-only', type=int, default=-1, metavar='RANK',
                    help='print ONLY the strong_rank8 object of this rank of 8 (the N = 1 line embeds it: measured in a fresh child '
                         'process, as a real rank is its own process -- inside the long-lived bench process the same loop is bound by a '
                         'slower host: 3.4 ms against 2.5)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--cpu-sample', type=int, default=2048)
    ap.add_argument('--details', metavar='FILE', default='bench_details.json',
                    help='where the full result object goes (every measurement beside the headline); the stdout line keeps the '
                         'headline fields only ("": not written)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step handed its caller to DIR/<name>.npy (float32 / '
                         'float64): loss, accuracy and every parameter after its update -- tables larger than '
                         'DUMP_SAMPLE_BYTES as a fixed seeded sample of rows, with their row numbers (rank 0 writes)')
    return ap.parse_args()


DUMP_SAMPLE_BYTES = 32 << 20         # per sampled table; everything else is written whole (64 MB in all at most)
DUMP_TOTAL_BYTES = 64 << 20


def dump_outputs(out_dir, loss, acc, model):
    """The last timed step's results as .npy files: what a caller of the training step receives (loss, accuracy) and the
    parameters it updated in place.  A parameter of more than DUMP_SAMPLE_BYTES keeps a sample of its rows drawn with a fixed
    seed (same arguments -> same rows), written beside it as <name>.sample_rows (float64 row numbers)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {'loss': np.asarray([float(loss)], dtype=np.float64),
              'accuracy': np.asarray([float(acc)], dtype=np.float64)}
    for name, p in model.named_parameters():
        t = p.detach()
        if t.numel() * 4 > DUMP_SAMPLE_BYTES and t.dim() >= 2:
            row_bytes = 4 * (t.numel() // t.shape[0])
            k = min(t.shape[0], max(1, DUMP_SAMPLE_BYTES // row_bytes))
            rows = np.sort(np.random.default_rng(0).choice(t.shape[0], k, replace=False))
            arrays['param.%s.sample_rows' % name] = rows.astype(np.float64)
            t = t.index_select(0, torch.from_numpy(rows).to(t.device))
        arrays['param.' + name] = t.float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_TOTAL_BYTES:
        raise SystemExit('--dump-outputs: %d bytes exceed the %d-byte budget' % (total, DUMP_TOTAL_BYTES))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)


# the stdout line: the headline and what the tests / tools read from it.  It stays short (a reader that keeps only the end of
# the output must still get all of it) and strict JSON; the full result object goes to --details
LINE_KEYS = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
             'dtype', 'data', 'loss', 'priming_passes_before_warmup', 'first_pass_ms', 'second_pass_ms', 'sequential_ms_per_step',
             'collectives', 'checksums')
LINE_CONFIG_KEYS = ('workload', 'subgraphs_per_gpu', 'subgraphs_total', 'schedule')
LINE_ROOFLINE_KEYS = ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'algorithmic_bytes_per_launch', 'ms_per_launch')
LINE_CPU_KEYS = ('value', 'unit', 'cores', 'kind', 'error')
LINE_MAX_BYTES = 4096                # (without the opt-in SGNN_BENCH_CHECKSUMS lists)


def _strict(o):
    """JSON-safe copy: non-finite floats become null (json.dumps would write NaN / Infinity)."""
    if isinstance(o, dict):
        return {k: _strict(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_strict(v) for v in o]
    if isinstance(o, float) and not np.isfinite(o):
        return None
    return o


def result_line(result, details=None):
    """The one JSON line bench.py prints: the headline fields of ``result``, the structure-channel roofline and the CPU
    baseline in short, and the name of the file that holds everything (``details``)."""
    line = {k: result[k] for k in LINE_KEYS if k in result}
    line['config'] = {k: result['config'][k] for k in LINE_CONFIG_KEYS if k in result.get('config', {})}
    if result.get('roofline'):
        line['roofline'] = {k: result['roofline'].get(k) for k in LINE_ROOFLINE_KEYS}
    if result.get('cpu_baseline'):
        cb = result['cpu_baseline']
        line['cpu_baseline'] = {k: cb[k] for k in LINE_CPU_KEYS if k in cb}
        if isinstance(cb.get('calibration'), dict):
            line['cpu_baseline']['calibration_ratio'] = cb['calibration'].get('ratio')
            line['cpu_baseline']['value_calibrated_to_reference'] = cb['calibration'].get('value_calibrated_to_reference')
    if details:
        line['details'] = details
    return json.dumps(_strict(line), allow_nan=False)


def build_inputs(args, rank, world):
    """Graph (identical on every rank) and this rank's subgraphs.  weak: rank r draws its own
    ``--subgraphs`` subgraphs (seed 1000 + r); strong: every rank draws the same ``--subgraphs`` subgraphs
    (seed 1000) and keeps its contiguous block."""
    from subgnn_amd import synthetic
    from subgnn_amd.dist import shard_range
    t0 = time.time()
    edges = synthetic.barabasi_albert_edges(args.nodes, args.m, seed=42)
    rowptr, col = synthetic.sorted_csr(edges, args.nodes)
    if args.scaling == 'strong':
        a, b = shard_range(args.subgraphs, rank, world)
        subs = synthetic.bfs_subgraphs(rowptr, col, args.subgraphs, args.subgraph_nodes, seed=1000)[a:b]
        total = args.subgraphs
    else:
        subs = synthetic.bfs_subgraphs(rowptr, col, args.subgraphs, args.subgraph_nodes, seed=1000 + rank)
        total = args.subgraphs * world
    return rowptr, col, subs, total, time.time() - t0


DS_SEARCH = 512      # csrc/degree_sequence.hip: with row-sorted CSR, lists of >= DS_SEARCH entries are searched, not streamed


def degseq_algorithmic_bytes(rowptr, sets_lists, search=False):
    """per set  sum_v (16 + 4 deg(v)) + 4|S| (ids in) + 4|S| (degrees out);
    internal and external computed in one pass (the external output adds 4|S|).
    ``search``: the byte count of the shipped launch -- a list of >= DS_SEARCH entries is not read: each
    of the |S| members binary-searches it, floor(log2 deg) + 1 probes and one verifying read of 4 bytes."""
    deg = np.diff(rowptr)
    total = 0
    for s in sets_lists:
        d = deg[np.asarray(s, dtype=np.int64)].astype(np.int64)
        per_list = 4 * d
        if search == 'bits':
            # round 6 (sgnn_degree_sequence_hub_bitmaps): such a list has a membership bitmap and each of the |S| members reads ONE
            # 4-byte word of it; every member also reads its hub_index entry
            per_list = np.where(d >= DS_SEARCH, 4 * len(d), per_list) + 4
        elif search:
            steps = np.floor(np.log2(np.maximum(d, 1))).astype(np.int64) + 2
            per_list = np.where(d >= DS_SEARCH, np.minimum(4 * d, 4 * steps * len(d)), per_list)
        total += int((16 + per_list).sum()) + 12 * len(d)
    return total


XGMI_LINK_GBS = 153.0          # per direction and link; 7 links per GPU (MI355X_MICROARCH.md)


def projection(args, result, model, S, sequential_ms=None, shard_line=None, strong_line=None):
    """8-GPU estimates from THIS run's measurements + bytes / link rate, so that a SCALE run can be read against them.  Not a
    measurement.  BASELINE.json words configs[3] as "50k subgraphs, sharded across 8": that is the STRONG form (--scaling
    strong, 6 250 subgraphs per GPU); the tier's multi-GPU contract (per-GPU work fixed) and bench.py's default are the WEAK
    form (50k subgraphs per GPU) -- both are projected.
    weak_*: from the schedule ``--gpus 8`` RUNS by default -- sequential passes, two-stream preparation (N > 1 pipelines only
    with --pipeline-multi) -- timed live in this process (``sequential_ms``); the pipelined figure is beside it.
    strong_*: from the 6 250-subgraph shard timed live in this process (``shard_line``), not from a committed file."""
    W = 8
    step_pipelined = result['ms_per_step']
    step = sequential_ms if sequential_ms else step_pipelined
    table_bytes = int(model.node_embeddings.weight.numel() * 4)
    small_bytes = int(sum(p.numel() for p in model.parameters() if p.requires_grad and p is not model.node_embeddings.weight) * 4)
    per_link = table_bytes / W                                   # a reduce-scatter / all-gather moves 1/W of the buffer per peer
    direct_ms = per_link / (XGMI_LINK_GBS * 1e9) * 1e3            # all 7 links busy at once (direct exchange)
    ring_ms = (W - 1) * per_link / (XGMI_LINK_GBS * 1e9) * 1e3    # one link per step (ring)
    adam_ms = result['stages_ms'].get('optimizer', 0.5)
    out = {'n_gpus': W, 'not_a_measurement': True,
           'what_gpus_8_runs_by_default': 'weak form (50k subgraphs per GPU), sequential passes with the two-stream preparation, head on '
                                          'the rank\'s own rows; --pipeline-multi pipelines the passes as at N = 1, --scaling strong is '
                                          'BASELINE configs[3] as worded',
           'collective_bytes_per_step': {'table_gradient_reduce_scatter': table_bytes, 'table_all_gather(hidden under the next preparation)': table_bytes,
                                         'small_gradients_all_reduce': small_bytes},
           'reduce_scatter_ms': {'direct_7_links': round(direct_ms, 3), 'ring': round(ring_ms, 3)},
           'one_gpu_ms_per_step': {'pipelined(this line\'s value)': round(step_pipelined, 3),
                                   'sequential_two_stream(what N>1 runs; timed live beside it)': round(sequential_ms, 3) if sequential_ms else None}}
    # weak: every rank runs the sequential step on its own 50k subgraphs; + the exposed reduce-scatter + a latency-bound small
    # all-reduce (~0.1 ms); - 7/8 of the table's Adam (owner-computes on 1/8 of the rows).  Speed-up against THIS line's value
    # (the pipelined one-GPU step): what SCALE's N = 8 over N = 1 ratio would show.
    for name, rs in (('direct', direct_ms), ('ring', ring_ms)):
        ms = step + rs + 0.1 - adam_ms * (W - 1) / W
        out['weak_' + name] = {'ms_per_step': round(ms, 2), 'subgraphs_per_s': round(W * S / ms * 1e3), 'speedup_vs_1gpu': round(W * step_pipelined / ms, 2)}
        msp = step_pipelined + rs + 0.1 - adam_ms * (W - 1) / W
        out['weak_' + name + '_with_--pipeline-multi'] = {'ms_per_step': round(msp, 2), 'speedup_vs_1gpu': round(W * step_pipelined / msp, 2)}
    # strong: the step of ONE rank of eight as that rank runs it, timed live in this process (strong_rank8: its own share of every
    # dealt stage, one BFS word, Adam on its eighth of the table; peers' shares from recorded buffers) + what the links add: the
    # table gradient's reduce-scatter, the small all-reduce (~0.1 ms, latency-bound), the bytes the dealt exchanges deliver at
    # 7 links' rate + ~20 us of latency each.  (The table's all-gather travels under the next preparation.)
    if strong_line and S == 50_000:
        exchanges = max(1, len(strong_line['received_bytes_per_pass']))
        dealt_ms = strong_line['received_bytes_total'] / (7 * XGMI_LINK_GBS * 1e9) * 1e3 + 0.02 * exchanges
        for name, rs in (('direct', direct_ms), ('ring', ring_ms)):
            ms = strong_line['ms_per_step_device'] + rs + 0.1 + dealt_ms
            out['strong_' + name] = {'ms_per_step': round(ms, 2), 'subgraphs_per_s': round(S / ms * 1e3),
                                     'speedup_vs_1gpu': round(step_pipelined / ms, 2)}
        out['strong_source'] = ('this run: %.2f ms of device time per pass of rank %d of %d (strong_rank8 object of this line) + %.3f ms '
                                'for the dealt exchanges\' %d bytes + reduce-scatter + 0.1 ms small all-reduce'
                                % (strong_line['ms_per_step_device'], strong_line['rank'], strong_line['world'], dealt_ms,
                                   strong_line['received_bytes_total']))
    elif shard_line and S == 50_000:
        for name, rs in (('direct', direct_ms), ('ring', ring_ms)):
            ms = shard_line['ms_per_step'] + rs + 0.1 - shard_line['stages_ms'].get('optimizer', adam_ms) * (W - 1) / W
            out['strong_' + name] = {'ms_per_step': round(ms, 2), 'subgraphs_per_s': round(S / ms * 1e3),
                                     'speedup_vs_1gpu': round(step_pipelined / ms, 2)}
        out['strong_source'] = 'this run: %.2f ms per 6 250-subgraph pass on one GPU (shard6250 object of this line; strong_rank8 was not measured)' % shard_line['ms_per_step']
    out['note'] = ('BASELINE.json configs[3] ("50k subgraphs, sharded across 8") is the strong form.  strong_* is priced from ONE rank of '
                   'eight run as that rank runs it (strong_rank8: its eighth of the dealt work, one BFS word over all ranks\' components, '
                   'Adam on its eighth of the table, forward + backward replayed from a hipGraph): what does not shrink with the shard -- '
                   'the position search (one 64-source word still walks the whole graph), the per-pass host work of ~130 eager '
                   'preparation launches, the dense 256 MB table gradient on the links -- bounds it near 3x; the >= 6x target is reachable '
                   'in the weak form (50k per GPU: what `bench.py --gpus 8` runs by default)')
    return out


def time_shard(g, subs, labels, emb, hp, steps, warmup, depth=2):
    """The strong-scaling shard (BASELINE configs[3] as worded: 50k subgraphs dealt to 8 GPUs = 6 250 per GPU) timed on THIS GPU in
    THIS process: rank 0's block of the benchmark's subgraphs, the schedule `bench.py --subgraphs 6250` picks (training half
    replayed from a hipGraph, passes pipelined, two prepared passes in flight).  -> dict for the line's ``shard6250`` object."""
    from subgnn_amd import hotpath, optim
    from subgnn_amd.SubGNN import SubGNN
    S = len(subs)
    model = SubGNN.from_memory(dict(hp), g, {'train': subs, 'val': [], 'test': []},
                               {'train': labels, 'val': labels[:0], 'test': labels[:0]}, emb, num_classes=3)
    model.train()
    opt = optim.ClipAdam(model.parameters(), hp['learning_rate'], max_norm=hp['grad_clip'], capturable=True)
    trainer = hotpath.CapturedTraining(model, opt, 'train', warmup=1)
    pipe = hotpath.PassPipeline(model, 'train', None)
    side_timers = []

    def step(timed):
        timer = hotpath.StageTimer(timed)
        timer.mark('start')
        pipe.install(timer, installer=trainer.install)
        if timed:
            side_timers.append(pipe.timer)
        installed = torch.cuda.Event()
        installed.record()
        loss, _acc = trainer.step()
        timer.mark('training_half(hipGraph)')
        pipe.start(timed, after=installed)
        return timer, loss
    torch.cuda.synchronize()
    t_cold = time.perf_counter()
    for _ in range(depth):
        pipe.start()
    step(False)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t_cold) * 1e3
    for _ in range(1 + warmup):
        step(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    timers = []
    for _ in range(steps):
        tm, loss = step(True)
        timers.append(tm)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    stage, cnt = {}, {}
    for tm in timers + side_timers:
        for k, v in tm.summary().items():
            stage[k] = stage.get(k, 0.0) + v
            cnt[k] = cnt.get(k, 0) + 1
    host, hcnt = {}, {}
    for tm in timers + side_timers:
        for k, v in tm.host_summary().items():
            host[k] = host.get(k, 0.0) + v
            hcnt[k] = hcnt.get(k, 0) + 1
    # the table's Adam inside the recorded half is not a stage of its own: priced from the 50k run's optimizer stage by the caller
    out = {'subgraphs': S, 'ms_per_step': ms, 'subgraphs_per_s': S / ms * 1e3, 'steps': steps, 'warmup': warmup,
           'host_ms_per_stage(time the host needs to queue it)': {k: round(v / hcnt[k], 3) for k, v in host.items()},
           'schedule': 'training half replayed from a hipGraph, passes pipelined, %d prepared passes in flight' % depth,
           'first_pass_ms': round(first_ms, 1), 'recordings': trainer.recordings,
           'stages_ms': {k: round(v / cnt[k], 3) for k, v in stage.items()}, 'loss': float(loss)}
    del trainer, pipe, opt, model
    torch.cuda.empty_cache()
    return out


def dp_tail(small, opt, table, table_opt, clip, average, all_reduce_small=None, all_reduce_scalar=None, timer=None):
    """What a data-parallel rank runs behind its backward pass (N > 1, and the emulated rank of ``strong_rank8``): all-reduce of
    the small gradients, reduce-scatter of the table's, clip_grad_norm_'s rule on the GLOBAL norm (one multi-tensor norm launch
    for the small gradients), torch's fused Adam on the small parameters, owner-computes Adam on the rank's slice of the table
    (its all-gather is waited for before the next reader of the table), gradients dropped."""
    t = timer
    if all_reduce_small is not None:
        all_reduce_small(small, average)
    if t is not None:
        t.mark('coll_small_gradients_all_reduce')
    sq = table_opt.reduce_grad()
    if t is not None:
        t.mark('coll_table_gradient_reduce_scatter')
    if all_reduce_scalar is not None:
        all_reduce_scalar(sq)
    grads = [p.grad for p in small if p.grad is not None]
    if grads:
        sq = sq + torch.stack(torch._foreach_norm(grads)).float().pow(2).sum()
    coef = torch.clamp(clip / (torch.sqrt(sq) + 1e-6), max=1.0)         # clip_grad_norm_'s rule on the global norm
    if t is not None:
        t.mark('coll_norm_all_reduce')
    if grads:
        torch._foreach_mul_(grads, coef)
    opt.step()
    table_opt.step(grad_scale=coef)                              # its all-gather is waited for before the next reader of the table
    for p in small:
        p.grad = None
    table.grad = None
    if t is not None:
        t.mark('optimizer')


def time_strong_rank(g, subs, all_labels, emb, hp, full_model, steps, warmup, rank=3, world=8, depth=2):
    """BASELINE configs[3] as worded -- 50k subgraphs dealt to 8 GPUs -- as ONE of those ranks runs it, timed on this GPU in this
    process: rank ``rank`` of ``world`` of `bench.py --gpus 8 --scaling strong --pipeline-multi`, with the
    collectives' results supplied by dist.EmulatedPeers (recorded on the first pass: the values are those of the real sharded
    run; what a link would carry is priced by the caller from ``received_bytes``).  The rank's work per pass:
      preparation (side stream)  its 6 250 subgraphs' components, border search + N draws, degree sequences; ITS eighth of the
                                 210 structure patches and of their walks (all-gathered); ONE 64-source BFS word (its 23 of the
                                 183 position anchors) over ALL ranks' 50k components (all-to-all); DTW of its 6 250 x 210 pairs;
      training half (main)       forward + backward replayed from a hipGraph (hotpath.CapturedTraining(optimizer=None):
                                 collectives are not recorded), then eagerly: gradient exchange, global-norm clip, fused Adam on the
                                 small parameters, Adam on ITS eighth of the embedding table (dist.ShardedTableAdam).
    -> dict for the line's ``strong_rank8`` object."""
    from subgnn_amd import hotpath
    from subgnn_amd import dist as sdist
    from subgnn_amd.SubGNN import SubGNN
    total = len(subs)
    a, b = sdist.shard_range(total, rank, world)
    dev = emb.device
    emu = sdist.EmulatedPeers(rank, world)
    cc_all = full_model.train_cc_ids
    emu.provided['cc_ids_all'] = cc_all.reshape(-1, cc_all.shape[-1])
    emu.maxima[2] = torch.tensor([cc_all.shape[1], cc_all.shape[2]], dtype=torch.int32, device=dev)
    widths = [v for k_, v in full_model._border_width.items() if k_[0] == 'train']
    if widths:
        emu.maxima[1] = widths[0]
    shard = sdist.Shard(total, rank, world, deal_shared=True, emulator=emu)
    labels = all_labels[a:b].clone()
    model = SubGNN.from_memory(dict(hp), g, {'train': subs[a:b], 'val': [], 'test': []},
                               {'train': labels, 'val': labels[:0], 'test': labels[:0]}, emb, num_classes=3)
    model.train()
    table = model.node_embeddings.weight
    small = [p for p in model.parameters() if p.requires_grad and p is not table]
    opt = torch.optim.Adam(small, lr=hp['learning_rate'], fused=True)
    table_opt = sdist.ShardedTableAdam(table, hp['learning_rate'], average=True, emulate=(rank, world))
    model._table_sync = table_opt.wait
    trainer = hotpath.CapturedTraining(model, None, 'train', warmup=1)
    pipe = hotpath.PassPipeline(model, 'train', shard)
    side_timers = []

    def step(timed):
        timer = hotpath.StageTimer(timed)
        timer.mark('start')
        pipe.install(timer, installer=trainer.install)
        if timed:
            side_timers.append(pipe.timer)
        installed = torch.cuda.Event()
        installed.record()
        loss, _acc = trainer.step()
        timer.mark('forward+backward(hipGraph)')
        # the gradient exchange + optimizer are queued BEFORE the host starts on the next preparation (its ~130 eager launches take
        # the host longer than the device needs for them: queued behind them the tail started 2.7 ms late)
        dp_tail(small, opt, table, table_opt, hp['grad_clip'], True, timer=timer)
        pipe.start(timed, after=installed)
        timer.mark('(host: next pass queued)')
        return timer, loss
    torch.cuda.synchronize()
    t_cold = time.perf_counter()
    for _ in range(depth):
        pipe.start()
    step(False)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t_cold) * 1e3
    for _ in range(1 + warmup):
        step(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    timers = []
    for _ in range(steps):
        tm, loss = step(True)
        timers.append(tm)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    stage, cnt = {}, {}
    for tm in timers + side_timers:
        for k, v in tm.summary().items():
            stage[k] = stage.get(k, 0.0) + v
            cnt[k] = cnt.get(k, 0) + 1
    host, hcnt = {}, {}
    for tm in timers + side_timers:
        for k, v in tm.host_summary().items():
            host[k] = host.get(k, 0.0) + v
            hcnt[k] = hcnt.get(k, 0) + 1
    recv = {str(k): int(v) for k, v in emu.received_bytes.items()}
    out = {'rank': rank, 'world': world, 'subgraphs_of_the_rank': b - a, 'subgraphs_total': total, 'ms_per_step_device': ms,
           'steps': steps, 'warmup': warmup,
           'schedule': 'rank %d of %d of --scaling strong --pipeline-multi: dealt preparation on a second stream (%d passes in flight), '
                       'forward + backward replayed from a hipGraph, gradient exchange + sharded optimizer eager behind it; the peers\' '
                       'shares of every exchange come from recorded buffers (dist.EmulatedPeers), no byte crosses a link' % (rank, world, depth),
           'first_pass_ms': round(first_ms, 1), 'recordings': trainer.recordings,
           'stages_ms': {k: round(v / cnt[k], 3) for k, v in stage.items()},
           'host_ms_per_stage(time the host needs to queue it)': {k: round(v / hcnt[k], 3) for k, v in host.items()},
           'received_bytes_per_pass': recv, 'received_bytes_total': int(sum(recv.values())),
           'table_gradient_bytes': int(table.numel() * 4), 'loss_of_the_rank': float(loss)}
    del trainer, pipe, opt, table_opt, model
    torch.cuda.empty_cache()
    return out


def strong_rank_only(args):
    """`bench.py --strong-rank-only R`: the benchmark's graph and subgraphs, one unsharded preparation (it supplies what only the
    other ranks could compute: all ranks' component ids, the global padded widths), then time_strong_rank -> one JSON line."""
    from subgnn_amd import ops, hotpath
    from subgnn_amd.SubGNN import SubGNN
    rowptr, col, subs, total, _ = build_inputs(args, 0, 1)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    g = ops.DeviceGraph(rowptr, col, np.arange(1, args.nodes + 1, dtype=np.int32), dev)
    torch.manual_seed(0)
    emb = torch.randn(args.nodes, args.embed, device=dev)
    hp = dict(ALL_DENSITY_HP)
    hp['node_embed_size'] = args.embed
    if os.environ.get('SGNN_BENCH_HP'):
        hp.update(json.loads(os.environ['SGNN_BENCH_HP']))
    all_labels = torch.randint(0, 3, (total,), generator=torch.Generator().manual_seed(0))
    all_labels[:3] = torch.tensor([0, 1, 2])
    full = SubGNN.from_memory(dict(hp), g, {'train': subs, 'val': [], 'test': []},
                              {'train': all_labels, 'val': all_labels[:0], 'test': all_labels[:0]}, emb, num_classes=3)
    hotpath.prepare_sparse(full, 'train')
    torch.cuda.synchronize()
    import gc
    gc.collect()
    gc.freeze()
    line = time_strong_rank(g, subs, all_labels, emb, hp, full, steps=max(10, args.steps), warmup=3, rank=args.strong_rank_only,
                            depth=max(1, args.pipeline_depth))
    line['measured_in'] = 'a fresh child process of bench.py (--strong-rank-only): one process per rank, as under torch.distributed.run'
    print(json.dumps(line))


def measure_rooflines(args, model, g, rowptr, hp, stage_ms, stage_each, elapsed, S, rank):
    """--full: the roofline of the structure-channel CSR gather and of the other HBM-class kernels of the pass, priced from
    launches of their own after the timed steps (``stage_ms`` / ``stage_each``: the timed passes' stage times), and the
    committed counters of the longest kernel -> the ``roofline``, ``rooflines`` and ``longest_kernel`` objects."""
    from subgnn_amd import ops, hotpath
    n = args.nodes
    # ---- roofline of the structure-channel CSR gather, measured live ------------------------
    cc_ids = model.train_cc_ids
    Sx, C, Lc = cc_ids.shape
    cc_sets = ops.Ragged.from_padded(cc_ids.reshape(Sx * C, Lc))
    set_lists = cc_sets.to_lists()
    alg_bytes = degseq_algorithmic_bytes(rowptr, set_lists)                      # every list read in full
    ds_bits = g.hub_tables() is not None                                          # (the lists of >= 512 entries have membership bitmaps)
    alg_bytes_search = degseq_algorithmic_bytes(rowptr, set_lists, search='bits' if ds_bits else True)   # what the shipped launch reads
    reps = 20
    ds_order = model._degseq_order['train']
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def back_to_back(**kw):
        ops.degree_sequence(g, cc_sets, order=ds_order, **kw)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            ops.degree_sequence(g, cc_sets, order=ds_order, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    # The roofline figure is a bandwidth, so it is taken on the launch that MOVES the algorithmic bytes: the
    # streaming form of the kernel (every neighbour list read in full; sgnn_degree_sequence without the
    # row-sorted CSR), 20 launches back to back on the launching stream.  The shipped launch (lists of
    # >= 512 entries binary-searched for the set's members: same results, fewer bytes) is timed inside the
    # timed region by the 'degree_sequences' stage events and priced with its own byte count.
    ds_ms_stream = back_to_back(search_long_lists=False)
    ds_ms_b2b = back_to_back()
    # in the timed region the launch shares the chip with the other stream's kernels (the training half of the pass before):
    # its event-to-event time there varies from pass to pass with what it happens to run beside (0.21-0.26 ms typically, the
    # odd pass twice that) -- the figure is the MEDIAN over the timed passes, the mean and the extremes are reported beside it
    ds_each = sorted(stage_each.get('degree_sequences', []))
    ds_ms = (ds_each[len(ds_each) // 2] if len(ds_each) % 2 else 0.5 * (ds_each[len(ds_each) // 2 - 1] + ds_each[len(ds_each) // 2])) \
        if ds_each else ds_ms_b2b
    achieved = alg_bytes / (ds_ms_stream * 1e-3) / 1e9

    # ---- the other HBM-class kernels of the pass, same recipe: SURVEY 8(d) bytes / live HIP-event time / 8 TB/s --------------
    from subgnn_amd import tape as _tape

    def timed(fn, reps_=10):
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps_):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps_
    deg_np = np.diff(rowptr)
    list_bytes = int(sum(int((16 + 4 * deg_np[np.asarray(s_, dtype=np.int64)].astype(np.int64)).sum()) for s_ in set_lists))
    n_members = int(sum(len(s_) for s_ in set_lists))
    rooflines = []
    if hp['use_neighborhood']:
        k1_seed, k1_stream = int(hp.get('seed', 0)), _tape.stream_id(_tape.STREAM_N_BOR, 'train', 0)
        _, _, k1_counts = ops.khop_border_sample(g, cc_sets, hp['neigh_sample_border_size'], hp['n_anchor_patches_N_out'], k1_seed, k1_stream)
        k1_ms = timed(lambda: ops.khop_border_sample(g, cc_sets, hp['neigh_sample_border_size'], hp['n_anchor_patches_N_out'],
                                                     k1_seed, k1_stream, width=model._border_width.get(('train', hp['neigh_sample_border_size'], cc_sets.n, 1))))
        # 8(d) a8, k = 1: the frontier's lists + 4 (|CC| + |border|).  The kernel never writes the border (the draw is a rank query
        # on the bitmap): achieved / frac price what it has to READ (lists + members); the formula with the border the reference
        # materialises is beside it
        k1_bytes = list_bytes + 4 * n_members
        k1_bytes_8d = k1_bytes + 4 * int(k1_counts.sum())
        rooflines.append({'kernel': 'khop1_sample_kernel<false> (sgnn_khop_border_sample: one-hop border + N-border draw, a8 + a4)',
                          'bound': 'hbm', 'algorithmic_bytes_per_launch': k1_bytes, 'ms_per_launch': k1_ms,
                          'achieved': k1_bytes / (k1_ms * 1e-3) / 1e9, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                          'frac': k1_bytes / (k1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          'survey_8d_bytes_with_the_border_written': k1_bytes_8d,
                          'frac_on_survey_8d_bytes': k1_bytes_8d / (k1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          'stage_ms_in_timed_region': stage_ms.get('border_bfs+N_anchors'),
                          'note': 'issue- and barrier-bound on one 1024-thread workgroup per CU around a 125 KB LDS bitmap (r04 counters: 26 % of wave-cycles issuing, 57 % waiting; r05: its load phase runs at the fabric\'s rate, DESIGN 4), '
                                  'not memory-bound; the lists come from L2 / Infinity Cache (the CSR is 88 MB)'})
    if hp['use_position']:
        src = model.anchors_pos_ext[0].to(torch.int32).contiguous()
        nlev = hotpath._bfs_levels(model, ('P_out', 'train', 0), hp.get('max_bfs_hops', 32))
        _, st_ = ops.bfs_min_hops_to_sets(g, src, cc_sets, max_hops=nlev, want_status=True)
        levels = int(st_[0]) + 1
        bfs_ms = timed(lambda: ops.bfs_min_hops_to_sets(g, src, cc_sets, max_hops=nlev))
        words = (src.numel() + 63) // 64
        nnz_dir = int(rowptr[-1])
        # the bit-parallel search reads, per level and 64-source word, every node's row pointers and neighbour list once;
        # 8(d) a9 as worded (one BFS per source: sum over visited nodes of 16 + 4 deg) would be n_sources x (16 N + 4 E)
        bfs_bytes = levels * words * (16 * n + 4 * nnz_dir) + 4 * cc_sets.n * src.numel()
        rooflines.append({'kernel': 'msbfs_* (sgnn_bfs_min_hops_to_sets: position-channel multi-source BFS + min over members, a9 sparse form)',
                          'bound': 'hbm', 'algorithmic_bytes_per_launch': bfs_bytes, 'ms_per_launch': bfs_ms,
                          'achieved': bfs_bytes / (bfs_ms * 1e-3) / 1e9, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                          'frac': bfs_bytes / (bfs_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          'levels': levels, 'source_words': words, 'sources': int(src.numel()),
                          'per_source_8d_bytes': int(src.numel()) * (16 * n + 4 * nnz_dir),
                          'note': 'all kernels of one search (init, expand / commit per level, set reduce) between two events; bytes = levels x '
                                  'words x (16 N + 4 E): the pull levels gather a 32-byte row per edge out of 128-byte lines (DESIGN 4)'})
    traffic = traffic_src = hbm_frac = traffic_shipped = None
    out_of_cache = None
    tf = next((f_ for f_ in (os.path.join(REPO, 'profiles', t_ + '_degseq_traffic.json') for t_ in ('r06', 'r05', 'r04', 'r02')) if os.path.exists(f_)), None)
    tf_name = 'profiles/' + os.path.basename(tf) if tf else None
    if tf:
        # PMC passes cannot run inside this process; these are the committed rocprofv3 measurements
        # (tools/run_hbm_probe.sh: separate --pmc passes, FETCH_SIZE calibrated on a copy of known size)
        with open(tf) as f:
            tj = json.load(f)
        if args.nodes == 1_000_000 and S == 50_000 and args.m == 10 and rank == 0:
            traffic = tj['benchmark_graph']['streaming']['memory_side_bytes_per_launch']
            traffic_shipped = tj['benchmark_graph']['shipped_search']['memory_side_bytes_per_launch']
            traffic_src = tf_name + ' (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; ' \
                          'FETCH_SIZE x2 per the 4 B/lane calibration copy)'
            hbm_frac = traffic / (ds_ms_stream * 1e-3) / 1e9 / HBM_PEAK_GBS
        out_of_cache = {'graph': tj['out_of_cache']['bfs_sets']['graph'], 'csr_bytes': tj['out_of_cache']['bfs_sets']['csr_bytes'],
                        'source': tf_name + ' (committed measurement, not re-run here)'}
        for fam, c in tj['out_of_cache'].items():
            out_of_cache[fam] = {form: {k: c[form][k] for k in ('ms_per_launch', 'algorithmic_frac_of_8TBs',
                                                                'memory_side_frac_of_8TBs', 'traffic_over_algorithmic')}
                                 for form in ('streaming', 'shipped_search')}
    # the kernel that dominates the pass by TIME is not an HBM kernel: the DTW launch is bound by fp64 vector issue.  Its
    # counters are a committed measurement (tools/run_dtw_pmc.sh), quoted beside the roofline of the HBM-class kernel.
    longest = None
    pj = next((f_ for f_ in (os.path.join(REPO, 'profiles', t_ + '_dtw_pmc.json') for t_ in ('r05', 'r04', 'r03')) if os.path.exists(f_)), None)
    if pj:
        pm = json.load(open(pj))
        kk = [k for k in pm if 'dtw_similarity' in k]
        if kk and stage_ms.get('dtw'):
            c = pm[kk[0]]
            wps = int(c.get('wavefronts_per_simd', 3))
            longest = {'kernel': kk[0].split('(')[0], 'bound': 'fp64 vector issue (not HBM, not MFMA)',
                       'share_of_step': round(stage_ms['dtw'] / (1e3 * elapsed / args.steps), 3),
                       'simd_valu_busy': round(c.get('simd_valu_busy_from_grbm', min(1.0, wps * c['frac_wave_cycles_valu_active'])), 3),
                       'wave_cycles': {'issuing': round(c['frac_wave_cycles_issuing'], 3),
                                       'waiting_on_memory_or_barrier': round(c['frac_wave_cycles_waiting_waitcnt_or_barrier'], 3),
                                       'issue_stalled': round(c['frac_wave_cycles_issue_stalled'], 3)},
                       'valu_instructions_per_64_pairs': round(c['valu_instructions_per_64_pairs']),
                       'source': 'profiles/' + os.path.basename(pj) + ' (rocprofv3 --pmc, committed measurement of the external-side launch; '
                                 '%d wavefronts per SIMD; SIMD busy = 4 x SQ_ACTIVE_INST_VALU / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs))' % wps}
    return {
        # the kernel BASELINE.json's target names, as the pass RUNS it (lists of >= 512 entries binary-searched, not streamed):
        # its own bytes / its time inside the timed region.  The streaming form (every list read in full: the launch that moves
        # SURVEY 8(d)'s bytes) is beside it as streaming_form -- that is the figure the >= 40 % target is quoted on.
        'roofline': {'kernel': ('degseq_wave_kernel<true, false, true> (sgnn_degree_sequence_hub_bitmaps: structure-channel CSR gather as '
                                'the pass runs it; lists of >= %d entries answered from their membership bitmaps)' % DS_SEARCH) if ds_bits else
                               ('degseq_wave_kernel<true, false, true> (sgnn_degree_sequence_sorted_rows: structure-channel CSR gather as '
                                'the pass runs it; lists of >= %d entries searched)' % DS_SEARCH),
                     'bound': 'hbm', 'achieved': alg_bytes_search / (ds_ms * 1e-3) / 1e9, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                     'frac': alg_bytes_search / (ds_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     # BASELINE.json's target (>= 40 % of the HBM roofline on the structure-channel CSR gather) is quoted on SURVEY 8(d)'s
                     # algorithmic bytes: the figure of the launch that moves them (streaming_form below), repeated here at the top level
                     'frac_of_roofline_on_survey_8d_bytes(streaming_form)': achieved / HBM_PEAK_GBS,
                     'traffic': traffic_shipped, 'traffic_source': traffic_src,
                     'algorithmic_bytes_per_launch': alg_bytes_search, 'ms_per_launch': ds_ms,
                     'ms_per_launch_is': 'median over the %d timed passes of the HIP-event time of the launch on its stream' % len(ds_each),
                     'ms_per_launch_mean_min_max': [round(sum(ds_each) / len(ds_each), 4), round(ds_each[0], 4), round(ds_each[-1], 4)] if ds_each else None,
                     'ms_per_launch_back_to_back': ds_ms_b2b, 'sets_per_launch': cc_sets.n,
                     'survey_8d_bytes_per_launch': alg_bytes,
                     'survey_8d_bytes_over_this_time_GBs': alg_bytes / (ds_ms * 1e-3) / 1e9,
                     'speedup_vs_streaming': ds_ms_stream / ds_ms,
                     'streaming_form': {'kernel': 'degseq_wave_kernel<true, false, false> (every neighbour list streamed: moves SURVEY 8(d)\'s bytes)',
                                        'achieved': achieved, 'frac': achieved / HBM_PEAK_GBS, 'ms_per_launch': ds_ms_stream,
                                        'algorithmic_bytes_per_launch': alg_bytes, 'traffic': traffic, 'hbm_frac': hbm_frac,
                                        'in_the_timed_pass': False},
                     'out_of_cache': out_of_cache,
                     'note': 'achieved = the bytes THIS launch reads (a list of >= 512 entries: 16 + 4 |S| -- one word of its membership bitmap per '
                             'member, round 6; rounds 3-5 searched it: 16 + 4 min(deg, (floor(log2 deg) + 2) |S|)) / its time '
                             'inside the timed region: it is latency-bound, and faster than the form that streams SURVEY 8(d)\'s bytes '
                             '(survey_8d_bytes_over_this_time_GBs exceeds the peak: the launch does not move them).  streaming_form: 8(d) bytes / '
                             'time of the launch that streams them, 20 launches back to back after the timed region (HIP events); on the '
                             'benchmark graph an ON-DIE rate -- the CSR (88 MB) fits the 256 MiB Infinity Cache: hbm_frac = memory-side '
                             'counter traffic over the same time.  out_of_cache: the same kernel on BA n=8M m=16 (CSR 1.09 GB)'},
        'rooflines': rooflines,
        'longest_kernel': longest}


def main():
    args = parse()
    if args.strong_rank_only >= 0:
        return strong_rank_only(args)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit('launch with torch.distributed.run --nproc-per-node %d' % args.gpus)
    # N = 1: the inputs are generated first (numpy only) and the worker processes of the cpu_baseline leg are forked HERE, before
    # anything initialises the GPU (a forked child must not inherit HIP state; they idle until the timed region is over)
    early = None
    if world == 1 and 'RANK' not in os.environ:
        early = build_inputs(args, 0, 1)
        if args.full and not args.no_cpu_baseline:
            try:
                from oracle import cpu_baseline
                cpu_baseline.start_pool(early[0], early[1])
            except Exception as ex:                      # no pool: the Python stages run in this process
                print('cpu_baseline worker pool not started: %r' % (ex,), file=sys.stderr)
    # SGNN_DIST_BACKEND=gloo: functional check of the multi-rank path on a box with fewer GPUs than ranks
    # (ranks then share GPUs and the collectives go through host memory); never a measurement
    backend = os.environ.get('SGNN_DIST_BACKEND', 'nccl')
    local = local % max(torch.cuda.device_count(), 1) if backend != 'nccl' else local
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    dist = None
    if world > 1 or 'RANK' in os.environ:            # launched by torch.distributed.run: one rank per GPU over RCCL
        import torch.distributed as dist
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev)
        else:
            dist.init_process_group(backend)

    from subgnn_amd import ops, hotpath, build
    from subgnn_amd import dist as sdist
    from subgnn_amd.SubGNN import SubGNN
    if rank == 0 and build.needs_build():
        build.build(verbose=False)
    if dist:
        dist.barrier()

    rowptr, col, subs, total_subgraphs, t_gen = early if early is not None else build_inputs(args, rank, world)
    n = args.nodes
    g = ops.DeviceGraph(rowptr, col, np.arange(1, n + 1, dtype=np.int32), dev)
    torch.manual_seed(0)
    emb = torch.randn(n, args.embed, device=dev)
    hp = dict(ALL_DENSITY_HP)
    hp['node_embed_size'] = args.embed
    hp['embedding_dtype'] = args.embedding_dtype
    if os.environ.get('SGNN_OVERLAP_STREAMS'):                   # '0': one stream (stage times then add up)
        hp['overlap_streams'] = os.environ['SGNN_OVERLAP_STREAMS'] != '0'
    if os.environ.get('SGNN_BENCH_HP'):                          # functional checks only (e.g. '{"lin_dropout": 0.0}')
        hp.update(json.loads(os.environ['SGNN_BENCH_HP']))
    S = len(subs)
    multi = dist is not None and world > 1
    # Multi-rank runs keep the sequential schedule unless asked (--pipeline-multi): the pipelined one issues the prepared
    # pass's width reductions on a second stream beside the gradient exchange -- two communicators in flight, which a
    # one-GPU functional check over gloo cannot validate for RCCL over xGMI
    pipelined = not args.no_pipeline and (not multi or args.pipeline_multi)
    # the prepared pass's width reductions run beside the gradient exchange of the pass in training: own communicator
    shard_group = dist.new_group() if (multi and pipelined) else None
    shard = sdist.Shard(total_subgraphs, rank, world, deal_shared=(args.scaling == 'strong'), group=shard_group) if multi else None
    if multi and shard.size != S:
        raise SystemExit('shard size mismatch')
    # labels of the GLOBAL batch (a function of the global subgraph number): the replicated head needs them all
    all_labels = torch.randint(0, 3, (total_subgraphs,), generator=torch.Generator().manual_seed(0))
    all_labels[:3] = torch.tensor([0, 1, 2])
    first = shard.start if multi else 0
    labels = all_labels[first:first + S].clone()
    replicated = multi and args.head == 'replicated'
    if multi:
        if total_subgraphs % world:
            raise SystemExit('equal shards needed (mean of means / replicated head): %d subgraphs over %d ranks' % (total_subgraphs, world))
        hp['dp_gather_embeddings'] = replicated
    model = SubGNN.from_memory(hp, g, {'train': subs, 'val': [], 'test': []},
                               {'train': labels, 'val': labels[:0], 'test': labels[:0]}, emb, num_classes=3)
    model.train()
    if multi and not replicated:
        torch.cuda.manual_seed(0x5eed + rank)                    # dropout masks of the ranks' own rows: independent streams
    table = model.node_embeddings.weight
    head = {id(p) for m_ in (model.lin, model.lin2, model.lin3) for p in m_.parameters()}
    if multi:
        # table: reduce-scatter + owner-computes Adam (dist.ShardedTableAdam); everything else: torch's fused Adam
        small = [p for p in model.parameters() if p.requires_grad and p is not table]
        opt = torch.optim.Adam(small, lr=hp['learning_rate'], fused=True)
        table_opt = sdist.ShardedTableAdam(table, hp['learning_rate'], average=not replicated)
        model._table_sync = table_opt.wait
        channel_params = [p for p in small if id(p) not in head]
        labels_dev = all_labels.to(dev)
    else:
        # clip + Adam with the 256 MB table in one HIP pass (optim.ClipAdam; torch's fused Adam for the small parameters)
        from subgnn_amd import optim
        graph_mode = args.graph
        if graph_mode == 'auto':
            graph_mode = 'train' if S <= 16384 else 'off'
        opt = optim.ClipAdam(model.parameters(), hp['learning_rate'], max_norm=hp['grad_clip'], capturable=graph_mode != 'off')
    params = [p for p in model.parameters() if p.requires_grad]
    # N = 1: the training half (component embeddings .. Adam) is recorded into a hipGraph on the second priming pass and
    # replayed: same kernels, one launch
    if multi:
        # N > 1: what can be recorded is forward + backward (collectives are not): shards of up to 16 384 subgraphs (--scaling strong),
        # with the sharded head; the gradient exchange and the sharded optimizer run eagerly behind every replay.  The default
        # (weak) form keeps everything eager, as before
        graph_mode = args.graph
        if graph_mode == 'auto':
            graph_mode = 'train' if (S <= 16384 and not replicated) else 'off'
        if graph_mode == 'both' or (graph_mode == 'train' and replicated):
            graph_mode = 'off'
    trainer = hotpath.CapturedTraining(model, None if multi else opt, 'train', warmup=1) if graph_mode == 'train' else None
    graphed = hotpath.GraphedPasses(model, opt, 'train', warmup=2) if graph_mode == 'both' else None

    stage_ms = {}
    kept_passes = []
    hooked = {}
    if os.environ.get('SGNN_BENCH_CHECKSUMS') == '2':
        # gradients flowing INTO every head layer / the subgraph embedding, cloned by autograd hooks (no sync): names the first
        # operation of the backward whose result differs between processes
        real_linear, real_embed = ops.linear, ops.subgraph_embedding
        counter = {'n': 0}

        def _tap(y, name):
            if torch.is_tensor(y) and y.requires_grad:
                y.register_hook(lambda g_, name=name: hooked.__setitem__(name, g_.detach().clone()))
            return y

        def linear_tapped(x, w, b):
            counter['n'] += 1
            return _tap(real_linear(x, w, b), 'hook/d_out_of_linear_%dx%d' % (w.shape[0], w.shape[1]))

        def embed_tapped(*a, **k):
            return _tap(real_embed(*a, **k), 'hook/d_subgraph_embedding')
        ops.linear, ops.subgraph_embedding = linear_tapped, embed_tapped
        real_ce, real_cc = ops.cross_entropy_with_accuracy, ops.cc_embed

        def ce_tapped(logits, labels_):
            hooked['fwd/logits'] = logits.detach().clone()
            return real_ce(logits, labels_)

        def cc_tapped(*a, **k):
            y = real_cc(*a, **k)
            hooked['fwd/cc_embed_%d' % len([1 for n_ in hooked if n_.startswith('fwd/cc_embed')])] = y.detach().clone()
            return y
        ops.cross_entropy_with_accuracy, ops.cc_embed = ce_tapped, cc_tapped

        def embed_tapped2(*a, **k):
            y = real_embed(*a, **k)
            hooked['fwd/subgraph_embedding'] = y.detach().clone()
            return _tap(y, 'hook/d_subgraph_embedding')
        ops.subgraph_embedding = embed_tapped2

        def snapshot_prepared():
            def walk(prefix, o):
                if isinstance(o, torch.Tensor):
                    hooked['prep/' + prefix] = o.detach().clone()
                elif isinstance(o, dict):
                    for k_, v_ in o.items():
                        walk('%s[%r]' % (prefix, k_), v_)
                elif isinstance(o, (list, tuple)):
                    for i_, v_ in enumerate(o):
                        walk('%s[%d]' % (prefix, i_), v_)
            for nm in ('train_cc_ids', 'train_neigh_pos_similarities', 'train_int_struc_similarities', 'train_bor_struc_similarities',
                       'anchors_neigh_int', 'anchors_neigh_border', 'anchors_pos_int', 'anchors_pos_ext', 'anchors_structure',
                       'structure_anchors', '_mpn_edge_plans'):
                walk(nm, getattr(model, nm, None))
            for k_, p_ in model.named_parameters():
                hooked['param_before/' + k_] = p_.detach().clone()

    pipe = pipe_main = hotpath.PassPipeline(model, 'train', shard) if (pipelined and graphed is None) else None
    side_timers = []
    last_acc = [None]                                            # the latest step's accuracy (--dump-outputs reads it)

    def step(timed, sequential=False):
        # ``sequential``: this step in the schedule N > 1 runs by default (the pass prepared after the previous one has trained)
        timer = hotpath.StageTimer(timed)
        pipe = None if sequential else pipe_main
        if graphed is not None and not sequential:
            timer.mark('start')
            loss, last_acc[0] = graphed.step()                   # two graph launches: this pass's training half, the next pass's preparation
            timer.mark('pass(hipGraphs: training half; the next preparation beside it)')
            return timer, loss
        if trainer is not None:
            timer.mark('start')
            if pipe is not None:
                pipe.install(timer, installer=trainer.install)   # the pass prepared during the previous step
                if timed:
                    side_timers.append(pipe.timer)
            else:
                trainer.install(hotpath.prepare_pass(model, 'train', timer, shard), timer)
            installed = torch.cuda.Event()
            installed.record()
            loss, last_acc[0] = trainer.step()                   # one graph launch: on the device before the host queues anything else
            timer.mark('training_half(hipGraph)' if not multi else 'forward+backward(hipGraph)')
            if multi:
                multi_tail(timer)                                # gradient exchange + sharded optimizer: eager (collectives are not recorded),
                #                                                  queued before the host starts on the next preparation
            if pipe is not None:
                pipe.start(timed, after=installed)               # the next pass: side stream, beside this step's training
                timer.mark('(host: next pass queued)')
            return timer, loss
        if pipe is not None:
            timer.mark('start')
            pipe.install(timer)                                  # the pass prepared during the previous step
            if timed:
                side_timers.append(pipe.timer)
            pipe.start(timed)                                    # the next one: side stream, beside this step's training
        else:
            hotpath.prepare_sparse(model, 'train', timer, shard)
        if os.environ.get('SGNN_BENCH_CHECKSUMS') == '2':
            snapshot_prepared()
        batch = hotpath.full_split_batch(model, 'train')
        if replicated:
            batch['label'] = labels_dev                          # the head runs on the gathered global batch
        out = model.training_step(batch, 0)
        last_acc[0] = out['log']['train_acc']
        timer.mark('forward')
        model.backward(None, out['loss'], None, 0)
        timer.mark('backward')
        if os.environ.get('SGNN_BENCH_CHECKSUMS') == '2':        # every pass's loss and gradients, cloned on the device (no sync)
            grads_ = {k_: p_.grad.detach().clone() for k_, p_ in model.named_parameters() if p_.grad is not None}
            grads_.update(hooked)
            hooked.clear()
            kept_passes.append((out['loss'].detach().clone(), grads_))
        if not multi:
            opt.step()                                           # (clips first: ClipAdam)
            opt.zero_grad(set_to_none=True)
            timer.mark('optimizer')
            return timer, out['loss'].detach()
        multi_tail(timer)
        return timer, out['loss'].detach()

    def multi_tail(timer):
        if replicated:
            # The loss is the mean over the GLOBAL batch and the head is replicated: head gradients are already
            # complete and identical on every rank; channel parameters (message-passing layers, LSTM, the table)
            # hold this rank's share of the sum.
            reduce_small = lambda ps, avg: sdist.all_reduce_gradients(channel_params, average=False)
        else:
            # every rank's loss is the mean over its own (equally many) subgraphs: the global mean is the mean of
            # those, and so are all gradients (the table's: ShardedTableAdam(average=True))
            reduce_small = lambda ps, avg: sdist.all_reduce_gradients(ps, average=True)
        dp_tail(small, opt, table, table_opt, hp['grad_clip'], not replicated, all_reduce_small=reduce_small,
                all_reduce_scalar=torch.distributed.all_reduce, timer=timer)

    if dist:
        # communicator set-up happens lazily at the first collective of each kind and size class: do it
        # here, with the shapes the step uses, so that it never lands in a timed step
        sdist.all_gather_rows(torch.zeros((S, 8), device=dev), equal_rows=True)
        dist.all_reduce(torch.zeros(1024, device=dev))
        torch.cuda.synchronize()
    # one-time work is kept out of the W warm-up steps the caller asked for: the first pass computes what is
    # kept per split (dispatch order, row-grouping decision), the second is the first to run the steady
    # path and grows the caching allocator to its final footprint (with --warmup 1 the timed steps were
    # 30 ms instead of 20)
    PRIMING_PASSES = 2 if graphed is None else 4                 # (graphed: two eager passes, then one recording per slot)
    torch.cuda.synchronize()
    t_cold = time.perf_counter()
    if pipe is not None:
        for k_ in range(max(1, args.pipeline_depth if not multi else 1)):
            pipe.start(timed=(k_ == 0))                          # the first pass(es); every step starts another one
    priming_ms = []
    first_breakdown = None
    for k_ in range(PRIMING_PASSES):
        tm_ = step(k_ == 0)[0]
        torch.cuda.synchronize()
        priming_ms.append((time.perf_counter() - t_cold) * 1e3)  # cumulative: [cold first pass, + the second]
        if k_ == 0:
            # where the cold pass's time goes (HIP events per stage; the preparation stages of a pipelined run come from the
            # preparation stream's timer).  Kept out of the timed region's stage averages.
            first_breakdown = {k: round(v, 2) for k, v in tm_.summary().items()}
            if side_timers:
                first_breakdown.update({k: round(v, 2) for k, v in side_timers.pop().summary().items()})
    first_pass_ms = priming_ms[0]                                # cold: no kept orders / hints / shapes, allocator empty
    second_pass_ms = priming_ms[1] - priming_ms[0]
    for _ in range(args.warmup):
        step(False)
    # the process holds millions of small Python objects by now (50k subgraph lists, the CSR's numpy views ...): a generation-2
    # collection in the middle of a timed region would walk all of them.  Everything alive here stays alive: moved out of the
    # collector's sight.  (The 30-60 ms holes that single steps and epochs show on this pool's boxes are the DEVICE's, not the
    # collector's: tools/device_stall_probe.py, tools/epoch_stall_probe.py.)
    import gc
    gc.collect()
    gc.freeze()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    timers = []
    kept_losses = []
    for _ in range(args.steps):
        tm, loss = step(True)
        timers.append(tm)
        if os.environ.get('SGNN_BENCH_CHECKSUMS'):
            kept_losses.append(loss.clone())
    if multi:
        table_opt.wait()                                         # the last step's table all-gather belongs to the timed region
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    loss = float(loss)                                           # (read once, after the timed region: no host round trip per step)
    if dist:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    # (hinted BFS searches are verified inside install_pass, before a pass is consumed)
    if multi and not replicated:                                 # the reported loss: mean over the global batch = mean of the ranks' means
        lt = torch.tensor([loss], device=dev, dtype=torch.float64)
        dist.all_reduce(lt)
        loss = float(lt.item()) / world
    if args.dump_outputs and rank == 0:                          # before anything below trains the model further
        dump_outputs(args.dump_outputs, loss, last_acc[0], model)
    stage_n, stage_each = {}, {}
    for tm in timers + side_timers:                              # (passes prepared before the timed region carry no marks)
        for k, v in tm.summary().items():
            stage_ms[k] = stage_ms.get(k, 0.0) + v
            stage_n[k] = stage_n.get(k, 0) + 1
            stage_each.setdefault(k, []).append(v)
    for k in stage_ms:                                           # mean over the passes that were timed
        stage_ms[k] /= stage_n[k]
    if os.environ.get('SGNN_BENCH_PER_STEP') and len(side_timers) > 2:
        # how long the preparation stream sat idle between one pass's last kernel and the next pass's first
        for a, b in zip(side_timers[1:-1], side_timers[2:]):
            if a.marks and b.marks:
                print('prep stream: pass %.3f ms, then idle %.3f ms' % (a.marks[0][1].elapsed_time(a.marks[-1][1]),
                                                                          a.marks[-1][1].elapsed_time(b.marks[0][1])), file=sys.stderr)
    if os.environ.get('SGNN_BENCH_PER_STEP'):
        for i, tm in enumerate(timers):
            print('step', i, {k: round(v, 3) for k, v in tm.summary().items()}, file=sys.stderr)
            print('     host', {k: round(v, 3) for k, v in tm.host_summary().items()}, file=sys.stderr)

    # ---- N > 1: what crossed the links, and (--full) north_star's exchange timed in this very run -------------------
    collectives = None
    if multi:
        collectives = {
            'rccl_ranks': dist.get_world_size(), 'backend': dist.get_backend(),
            'per_step_ms': {k[5:]: round(v, 3) for k, v in stage_ms.items() if k.startswith('coll_')},
            'table_all_gather_wait_ms': round(stage_ms.get('table_all_gather_wait', 0.0), 3),
            'table_bytes': int(table.numel() * 4)}
    if multi and args.full:
        # "RCCL all-gather of per-channel embeddings over xGMI" (BASELINE.json north_star): the (components, hid_dim) fp32
        # embeddings of this rank's shard gathered from every rank -- the collective the replicated head consumes inside
        # the step (--head replicated); with the default sharded head nothing needs it, so it is timed here on its own,
        # same shapes, same communicator, right after the timed steps
        rows = int(model.train_cc_ids.shape[0] * model.train_cc_ids.shape[1])
        x = torch.randn(rows, model.hid_dim, device=dev)
        sdist.all_gather_rows(x, equal_rows=True)
        torch.cuda.synchronize()
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g0.record()
        for _ in range(5):
            gathered = sdist.all_gather_rows(x, equal_rows=True)
        g1.record()
        torch.cuda.synchronize()
        ns = torch.tensor([g0.elapsed_time(g1) / 5], device=dev, dtype=torch.float64)
        dist.all_reduce(ns, op=dist.ReduceOp.MAX)
        ns_ms = float(ns.item())
        per_rank = rows * model.hid_dim * 4
        collectives['north_star_exchange'] = {
            'what': 'all-gather of the per-component channel embeddings (rows_per_rank, hid_dim) fp32 from every rank '
                    '(dist.all_gather_rows: what dist.gather_rows_replicated issues for the replicated head)',
            'rows_per_rank': rows, 'hid_dim': int(model.hid_dim), 'bytes_per_rank': per_rank,
            'gathered_rows': int(gathered.shape[0]), 'ms': round(ns_ms, 3),
            'algbw_GBs': round(per_rank * (world - 1) / (ns_ms * 1e-3) / 1e9, 1) if ns_ms > 0 else None,
            'inside_the_timed_step': bool(replicated)}
        del x, gathered

    # ---- --full: roofline of the structure-channel CSR gather and the other HBM-class kernels, measured live ------------------
    figures = measure_rooflines(args, model, g, rowptr, hp, stage_ms, stage_each, elapsed, S, rank) if args.full else {}

    # ---- --full, N = 1: measured beside the headline, in this process ----------------------------------
    sequential_ms = shard_line = strong_line = configs_obj = pool_reuse_ms = None
    if args.full and world == 1 and not args.no_extras and graphed is None:
        # (1) the schedule `--gpus 8` runs by default: sequential passes, two-stream preparation -- what projection.weak_* uses
        for _ in range(2):
            step(False, sequential=True)
        torch.cuda.synchronize()
        t_s = time.perf_counter()
        n_seq = max(5, min(args.steps, 10))
        for _ in range(n_seq):
            step(False, sequential=True)
        torch.cuda.synchronize()
        sequential_ms = 1e3 * (time.perf_counter() - t_s) / n_seq
        # (1b) the reference's own amortisation (NOT the headline): the structure-patch pool -- patches, walks,
        # degree sequences, DTW rows of all max_sim_epochs x 42 patches -- rebuilt every max_sim_epochs passes only, the passes
        # in between re-pick their 42 from it (hotpath.PassPipeline(pool_epochs=...)); same pipelined schedule otherwise
        if pipe_main is not None and trainer is None and hp['use_structure'] and hp.get('max_sim_epochs', 1) > 1:
            try:
                pe = int(hp['max_sim_epochs'])
                pool_pipe = hotpath.PassPipeline(model, 'train', shard, pool_epochs=pe)
                for _ in range(max(1, args.pipeline_depth)):
                    pool_pipe.start()

                def pool_step():
                    pool_pipe.install()
                    pool_pipe.start()
                    out = model.training_step(hotpath.full_split_batch(model, 'train'), 0)
                    model.backward(None, out['loss'], None, 0)
                    opt.step()
                    opt.zero_grad(set_to_none=True)
                for _ in range(pe):
                    pool_step()
                torch.cuda.synchronize()
                t_p = time.perf_counter()
                for _ in range(2 * pe):
                    pool_step()
                torch.cuda.synchronize()
                pool_reuse_ms = 1e3 * (time.perf_counter() - t_p) / (2 * pe)
                del pool_pipe
            except Exception as ex:
                print('pool-reuse schedule not measured: %r' % (ex,), file=sys.stderr)
        # (2) the strong-scaling shard of BASELINE configs[3] as worded (50k subgraphs over 8 GPUs): rank 0's 6 250, live
        if S == 50_000:
            try:
                shard_line = time_shard(g, subs[:S // 8], labels[:S // 8].clone(), emb, hp, steps=max(10, args.steps), warmup=3,
                                        depth=max(1, args.pipeline_depth))
                shard_line['stages_ms'].setdefault('optimizer', stage_ms.get('optimizer', 0.5))
            except Exception as ex:
                shard_line = None
                print('shard6250 not measured: %r' % (ex,), file=sys.stderr)
            # (2b) ... and one rank of eight AS THAT RANK RUNS IT (dealt shared work, one BFS word, an eighth of the table's Adam)
            try:
                # in a FRESH child process (a rank is its own process; this one's host loop runs 30-40 % slower by now -- a heap of
                # millions of objects, 256 idle workers of the CPU baseline -- and the emulated rank is bound by its host: 3.4 ms here,
                # 2.5 in a process of its own); falls back to this process if the child fails
                import subprocess
                cmd = [sys.executable, os.path.abspath(__file__), '--strong-rank-only', '3', '--steps', str(max(10, args.steps)),
                       '--nodes', str(args.nodes), '--m', str(args.m), '--subgraphs', str(args.subgraphs),
                       '--subgraph-nodes', str(args.subgraph_nodes), '--embed', str(args.embed), '--pipeline-depth', str(args.pipeline_depth)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                    strong_line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
                except Exception as ex:
                    print('strong_rank8 child process failed (%r): measuring in this process' % (ex,), file=sys.stderr)
                    strong_line = time_strong_rank(g, subs, all_labels, emb, hp, model, steps=max(10, args.steps), warmup=3,
                                                   depth=max(1, args.pipeline_depth))
                    strong_line['measured_in'] = 'the bench process itself (the child process failed)'
            except Exception as ex:
                strong_line = None
                import traceback
                traceback.print_exc()
                print('strong_rank8 not measured: %r' % (ex,), file=sys.stderr)
        # (3) the batch-sized training steps of the other BASELINE configurations (stand-ins: SURVEY 8, statistics unverified),
        # replayed from a hipGraph and eager, with the kernels one step launches
        from subgnn_amd import standins
        configs_obj = {'note': 'BASELINE.json configs[0,1,2,4] as stand-in datasets in the reference\'s file formats (subgnn_amd/standins.py), each '
                               'built, prepared and trained in THIS process after the timed region: ms per batch-sized training step (fwd + '
                               'bwd + clip + Adam), replayed from a hipGraph (the trainer\'s default) and eager; kernels_per_step by torch\'s '
                               'profiler on one eager step (None if the profiler could not run)'}
        t_x = time.perf_counter()
        for key, name in (('configs[0]', 'density_n'), ('configs[1]', 'ppi_bp'), ('configs[2]', 'hpo_metab'), ('configs[4]', 'em_user')):
            if time.perf_counter() - t_x > args.extras_budget_s:
                configs_obj[key] = {'skipped': 'extras budget of %.0f s used up' % args.extras_budget_s}
                continue
            try:
                t_c = time.perf_counter()
                line = standins.bench_config(name, steps=20, warmup=5, also_atomics=True, epochs=9)
                configs_obj[key] = {'standin': name, 'workload': line['config']['workload'], 'batch': line['config']['cc_ids_shape'],
                                    'ms_per_step_replayed': round(line['ms_per_step'], 3), 'ms_per_step_eager': round(line['eager']['ms_per_step'], 3),
                                    'subgraphs_per_s': round(line['value']), 'kernels_per_step': line['kernels_per_step'],
                                    'epoch': line.get('epoch'),
                                    'with_float_atomics(hparams deterministic=False; not the default)': None if not line.get('atomics') else {
                                        'ms_per_step_replayed': round(line['atomics']['ms_per_step'], 3), 'kernels_per_step': line['atomics']['kernels_per_step']},
                                    'prepare_data_s': line['prepare_data_s'], 'wall_s': round(time.perf_counter() - t_c, 1)}
            except Exception as ex:
                configs_obj[key] = {'standin': name, 'error': repr(ex)[:300]}
        torch.cuda.empty_cache()
    result = {
        'metric': 'subgraphs/sec fwd+bwd (all 3 channels on) + achieved HBM GB/s',
        'value': total_subgraphs * args.steps / elapsed, 'unit': 'subgraphs/s', 'n_gpus': world, 'steps': args.steps,
        'warmup': args.warmup, 'ms_per_step': 1e3 * elapsed / args.steps, 'higher_is_better': True,
        'scaling': args.scaling, 'vs_baseline': None,
        'dtype': 'f32' if args.embedding_dtype == 'fp32' else 'f32 (embedding table stored fp16, fp32 accumulate)',
        'data': 'synthetic' if backend == 'nccl' else 'synthetic (FUNCTIONAL CHECK over %s, not a measurement)' % backend,
        'config': {'workload': 'synthetic DENSITY-style BA base graph n=%d m=%d (%d undirected edges), %d BFS '
                               'subgraphs x %d nodes %s, all_density hparams (N 10/43, P 57/183, S 42, 1 layer), '
                               'D=%d, full pass = sampling + similarities + fwd + bwd + Adam' %
                               (n, args.m, int(rowptr[-1]) // 2, args.subgraphs, args.subgraph_nodes,
                                'per GPU (weak form; BASELINE configs[3] "50k sharded across 8" as worded is --scaling strong)' if args.scaling == 'weak' else 'in total (strong form: BASELINE configs[3] as worded)', args.embed),
                   'subgraphs_per_gpu': S, 'subgraphs_total': total_subgraphs,
                   'schedule': {'passes_pipelined': pipe is not None or graphed is not None, 'hipgraphs': graph_mode, 'training_half_from_hipgraph': trainer is not None or graphed is not None,
                                'prepared_passes_in_flight': (max(1, args.pipeline_depth) if not multi else 1) if pipe is not None else 0, 'two_stream_preparation': bool(hp.get('overlap_streams', True)) and not (shard is not None and shard.deal_shared)},
                   'parallelism': ('dp%d (subgraph shards; head on the rank\'s own rows, all-reduce of the small gradients, '
                                   'reduce-scatter / all-gather of the embedding table)' % world) if not replicated else
                                  ('dp%d (subgraph shards; RCCL all-gather of the channel embeddings into a replicated head, '
                                   'all-reduce of channel gradients, reduce-scatter / all-gather of the embedding table)' % world)},
        **figures,
        'collectives': collectives,
        'stages_ms': {k: round(v, 3) for k, v in stage_ms.items()},
        'stages_note': ('HIP-event time per stage on the stream it runs on; ' + ('pipelined: the preparation stages (components ... dtw) of later passes '
                        'run on a second stream beside cc_embed (which includes the wait for the prepared pass) / forward / backward / optimizer of pass k, which stretch each other -- '
                        'the stage times do not add up to the step (--no-pipeline with SGNN_OVERLAP_STREAMS=0: they do)' if pipe is not None
                        else 'sequential passes')),
        'loss': loss, 'setup_s': round(t_gen, 1), 'priming_passes_before_warmup': PRIMING_PASSES,
        # value / ms_per_step are STEADY-STATE figures: the timed passes reuse what the first pass of a split computes and keeps
        # (dispatch orders, the DTW row grouping + processing order, padded shapes, BFS level hints, the allocator's blocks).
        # The cold first pass (nothing kept, allocator empty, kernels' first launch) and the second one, host-timed with a
        # device synchronisation after each:
        'first_pass_ms': round(first_pass_ms, 2), 'second_pass_ms': round(second_pass_ms, 2),
        'first_pass_breakdown_ms': first_breakdown,
        # one-time start-up paid at model construction instead of inside the first pass (ops.warm_up: this library's code objects,
        # BLAS handles, the torch kernels of the preparation)
        'warm_up_ms_at_construction': round(1e3 * getattr(model, 'warm_up_s', 0.0), 1),
    }
    if args.full and world == 1 and args.scaling == 'weak':
        result['projection'] = projection(args, result, model, S, sequential_ms, shard_line, strong_line)
    if sequential_ms is not None:
        result['sequential_ms_per_step'] = round(sequential_ms, 3)
    if pool_reuse_ms is not None:
        result['extra'] = {'pool_reuse_ms_per_step': round(pool_reuse_ms, 3), 'pool_reuse_subgraphs_per_s': round(S / pool_reuse_ms * 1e3),
                           'pool_epochs': int(hp['max_sim_epochs']),
                           'note': 'NOT the headline: the structure-patch pool (210 patches: walks, degree sequences, DTW rows) rebuilt every '
                                   'max_sim_epochs passes, re-picked from in between (the reference samples and scores the pool once so that '
                                   're-picking is free: SubGNN.py:783-833, anchor_patch_samplers.py:316-328); mean over two pool cycles, '
                                   'pipelined schedule; bit-equal per consumed column (tests/test_gpu_hotpath.py::test_pool_reuse_pass_equals_a_full_pass)'}
    if shard_line is not None:
        result['shard6250'] = shard_line
    if strong_line is not None:
        result['strong_rank8'] = strong_line
    if configs_obj is not None:
        result['configs'] = configs_obj
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            from oracle import cpu_baseline
            result['cpu_baseline'] = cpu_baseline.run(rowptr, col, subs, hp, emb.cpu(), labels, args.cpu_sample, S)
        except Exception as ex:                      # the baseline must never hide the GPU number
            result['cpu_baseline'] = {'error': repr(ex)}
        finally:
            try:
                cpu_baseline.stop_pool()
            except Exception:
                pass
    if os.environ.get('SGNN_BENCH_CHECKSUMS'):
        # reproducibility across processes (tools/cross_process_probe.py --bench): every timed step's loss, bit for bit, and a
        # checksum of every parameter at the end -- read only here, after the timed region
        def _ck(t):
            v = t.detach().reshape(-1).contiguous().view(torch.int32).long()
            return [int(v.sum()), int((v * ((torch.arange(v.numel(), device=v.device) % 65521) + 1)).sum())]
        result['checksums'] = {'losses': [float(x) for x in kept_losses], 'loss_bits': [_ck(x) for x in kept_losses],
                               'params': {k: _ck(p_) for k, p_ in model.named_parameters()},
                               'passes': [{'loss': _ck(l_), 'grads': {k: _ck(g_) for k, g_ in gr_.items()}} for l_, gr_ in kept_passes]}
    if rank == 0:
        details = args.details
        if details:
            try:
                with open(details, 'w') as f:
                    f.write(json.dumps(_strict(result), allow_nan=False) + '\n')
            except OSError as ex:                    # the details must never hide the headline
                print('--details: %s not written: %r' % (details, ex), file=sys.stderr)
                details = None
        print(result_line(result, details))
    if dist:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

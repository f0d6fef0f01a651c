// Seeded walk sets (subgnn_hip.h, sgnn_seeded_walk_sets): connected candidate subgraphs around seed nodes, each the set of
// nodes a random walk with restarts visits until it holds its target size or runs out of steps.  Every draw is keyed by the
// item's NUMBER on the tape, not by its output row, so a chunk or an explicit list of items gives the bits of the whole call.
//
// One wavefront per item (a workgroup IS one wavefront), grid-stride over the items.  The walk itself is wave-uniform: the
// current node is pinned to a scalar with readfirstlane, so the draws run on the scalar unit and the two dependent loads of a
// step (rowptr, then col) are scalar loads.  The set is held across the lanes: entry j in register j / 64 of lane j % 64, four
// registers for SGNN_SEEDED_MAX_SIZE entries (0 = free: no node has id 0), so membership is four compares and a ballot and an
// append is one conditional move -- no LDS in the loop.  At the end the entries go to LDS once, every lane ranks its (up to
// four) entries by counting the smaller ones in a broadcast sweep, the entries are put at their ranks in LDS and the row is
// written coalesced; the key is the wave sum of sgnn_mix64 over the entries.  No float work, no atomics.
#include "common.h"

#define SGNN_SEEDED_MAX_SIZE 256       // entries of a set: 4 registers x 64 lanes
#define SGNN_SEEDED_GRID_CAP 8192      // workgroups of one launch: 8 wavefronts per SIMD on 256 compute units
#define SEEDED_REGS (SGNN_SEEDED_MAX_SIZE / SGNN_WAVE)

struct SeededArgs {
    int64_t max_id, n_seeds, per_seed; int width;
    uint64_t restart_thr; int max_steps; uint64_t h0; int64_t item_base, n_items;
};

// (the pointers are arguments of their own, marked __restrict__: behind a struct the compiler cannot tell that the outputs
// written in the loop leave the graph alone, and loads the walk's wave-uniform addresses through the vector unit)
__global__ __launch_bounds__(SGNN_WAVE) void seeded_walk_kernel(
    const SeededArgs a, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ seeds,
    const int32_t* __restrict__ sizes, const int64_t* __restrict__ item_ids, int32_t* __restrict__ out_nodes,
    int32_t* __restrict__ out_len, int32_t* __restrict__ out_steps, uint64_t* __restrict__ out_keys)
{
    __shared__ int32_t s_set[SGNN_SEEDED_MAX_SIZE];
    const int lane = threadIdx.x;

    for (int64_t i = blockIdx.x; i < a.n_items; i += gridDim.x) {
        const int64_t q = item_ids ? item_ids[i] : a.item_base + i;
        int32_t s = 0;
        int size = 1;
        if (q >= 0 && q / a.per_seed < a.n_seeds) {
            s = seeds[q / a.per_seed];
            size = min(max(sizes[q % a.per_seed], 1), a.width);
        }
        int32_t r[SEEDED_REGS];
#pragma unroll
        for (int k = 0; k < SEEDED_REGS; ++k) r[k] = 0;
        int n = 0, t = 0;
        if (s >= 1 && (int64_t)s <= a.max_id) {
            if (lane == 0) r[0] = s;
            n = 1;
            const uint64_t h1 = sgnn_tape_h1(a.h0, (uint64_t)q);
            int32_t cur = s;
            bool walk = rowptr[s + 1] > rowptr[s];
            while (walk && n < size && t < a.max_steps) {
                const uint32_t u = (uint32_t)(sgnn_tape_draw(h1, 2 * (uint64_t)t) >> 32);
                ++t;
                if ((uint64_t)u < a.restart_thr) { cur = s; continue; }
                const int64_t beg = rowptr[cur];
                const uint32_t d = (uint32_t)(rowptr[cur + 1] - beg);
                if (d == 0) { cur = s; continue; }                   // (a row without entries: only a one-way CSR has one here)
                cur = __builtin_amdgcn_readfirstlane(col[beg + sgnn_choice_index(h1, 2 * (uint64_t)t - 1, d)]);
                bool in = false;
#pragma unroll
                for (int k = 0; k < SEEDED_REGS; ++k) in |= r[k] == cur;
                if (__ballot(in) == 0) {
                    const int slot = n >> 6;                         // wave-uniform
#pragma unroll
                    for (int k = 0; k < SEEDED_REGS; ++k)
                        if (k == slot && lane == (n & 63)) r[k] = cur;
                    ++n;
                }
            }
        }

        // rank every entry among the n, place it, write the row
        __syncthreads();                                             // the item before this one is done with the LDS
#pragma unroll
        for (int k = 0; k < SEEDED_REGS; ++k) s_set[k * SGNN_WAVE + lane] = r[k];
        __syncthreads();
        int rank[SEEDED_REGS];
#pragma unroll
        for (int k = 0; k < SEEDED_REGS; ++k) rank[k] = 0;
        for (int j = 0; j < n; ++j) {
            const int32_t v = s_set[j];                              // one address for the wavefront: a broadcast
#pragma unroll
            for (int k = 0; k < SEEDED_REGS; ++k) rank[k] += v < r[k];
        }
        __syncthreads();
        uint64_t acc = 0;
#pragma unroll
        for (int k = 0; k < SEEDED_REGS; ++k)
            if (k * SGNN_WAVE + lane < n) {
                s_set[rank[k]] = r[k];
                acc += sgnn_mix64((uint64_t)(uint32_t)r[k]);
            }
        acc = sgnn_wave_sum_u64(acc);
        __syncthreads();
        int32_t* __restrict__ row = out_nodes + i * a.width;
        for (int j = lane; j < a.width; j += SGNN_WAVE) row[j] = j < n ? s_set[j] : 0;
        if (lane == 0) {
            out_len[i] = n;
            out_steps[i] = t;
            out_keys[i] = sgnn_set_key_finish(acc, (uint64_t)n);
        }
    }
}

extern "C" int64_t sgnn_seeded_walk_max_size(void) { return SGNN_SEEDED_MAX_SIZE; }

extern "C" int sgnn_seeded_walk_sets(const int64_t* rowptr, const int32_t* col, int64_t max_id, const int32_t* seeds,
                                     int64_t n_seeds, const int32_t* sizes, int64_t per_seed, int64_t width,
                                     uint64_t restart_thr, int64_t max_steps, uint64_t seed, uint64_t stream, int64_t item_base,
                                     const int64_t* item_ids, int64_t n_items, int32_t* out_nodes, int32_t* out_len,
                                     int32_t* out_steps, uint64_t* out_keys, void* stream_handle)
{
    if (max_id < 0 || n_seeds < 0 || n_items < 0 || item_base < 0 || max_steps < 0) return SGNN_ERR_BAD_ARG;
    if (width < 1 || width > SGNN_SEEDED_MAX_SIZE || per_seed < 1) return SGNN_ERR_BAD_ARG;
    if (restart_thr > (1ull << 32) || n_items > 0x7fffffff || max_steps > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    if (!item_ids && (unsigned __int128)item_base + (unsigned __int128)n_items > (unsigned __int128)n_seeds * (unsigned __int128)per_seed)
        return SGNN_ERR_BAD_ARG;
    if (n_items == 0) return SGNN_OK;
    if (!rowptr || !col || !sizes || (n_seeds > 0 && !seeds) || !out_nodes || !out_len || !out_steps || !out_keys)
        return SGNN_ERR_BAD_ARG;
    SeededArgs a = {};
    a.max_id = max_id; a.n_seeds = n_seeds; a.per_seed = per_seed; a.width = (int)width;
    a.restart_thr = restart_thr; a.max_steps = (int)max_steps; a.h0 = sgnn_tape_h0(seed, stream);
    a.item_base = item_base; a.n_items = n_items;
    hipLaunchKernelGGL(seeded_walk_kernel, dim3(sgnn_grid_for(n_items, 1, SGNN_SEEDED_GRID_CAP)), dim3(SGNN_WAVE), 0,
                       (hipStream_t)stream_handle, a, rowptr, col, seeds, sizes, item_ids, out_nodes, out_len, out_steps,
                       out_keys);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

SGNN_DEFINE_WARM(seeded_sets)

// Anchor-patch samplers driven by the counter-based draw tape (a1-a6).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// a4  neighbourhood anchors (reference SubGNN/anchor_patch_samplers.py:163-198) under the tape's
// neighbourhood-anchor law (common.h): per (row, slot) one index draw into the row's non-PAD
// entries in ascending order, one "all variates negative" draw for the PAD rule.  The rows are
// taken in canonical form -- ascending, PADs last (the host wrapper sorts; the fused border kernel
// answers the same rank query from its visited bitmap without ever sorting) -- so a slot is O(1).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_anchors_padded_kernel(
    const int64_t* __restrict__ ids, int64_t n_rows, int64_t L, int64_t n_slots,
    uint64_t h0, int64_t* __restrict__ out)
{
    const int64_t total = n_rows * n_slots;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / n_slots;
        const int64_t* row = ids + r * L;
        int64_t lo = 0, hi = L;                               // n = first PAD column of the canonical row
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (row[mid] != 0) lo = mid + 1; else hi = mid; }
        const int64_t n = lo;
        int64_t v = 0;
        if (n > 0) {
            const uint64_t h1 = sgnn_tape_h1(h0, (uint64_t)t);
            if (!(n < L && sgnn_nanchor_allneg(h1, (uint32_t)n))) v = row[sgnn_nanchor_index(h1, (uint32_t)n)];
        }
        out[t] = v;
    }
}

// Where a set's tape item comes from: its row number within the whole (possibly sharded) matrix, or a key the caller supplies
// per set (sgnn_set_keys: a function of the set's content, so the draw does not depend on where the set stands in the list).
struct ItemOfRow {
    int64_t base;
    __device__ uint64_t operator()(int64_t r) const { return (uint64_t)(base + r); }
};
struct ItemOfKey {
    const uint64_t* __restrict__ keys;
    __device__ uint64_t operator()(int64_t r) const { return keys[r]; }
};

// the law on one (set, slot): the index of the pick among the set's n ascending entries, -1 = PAD (n == 0 included)
__device__ static inline int64_t nanchor_pick(uint64_t h0, uint64_t item, int64_t n, bool has_pad) {
    if (n <= 0) return -1;
    const uint64_t h1 = sgnn_tape_h1(h0, item);
    if (has_pad && sgnn_nanchor_allneg(h1, (uint32_t)n)) return -1;
    return (int64_t)sgnn_nanchor_index(h1, (uint32_t)n);
}

template <class Item>
__global__ __launch_bounds__(256) void sample_anchors_ragged_kernel(
    const int64_t* __restrict__ set_ptr, const int32_t* __restrict__ set_nodes, int64_t n_sets,
    const uint8_t* __restrict__ row_has_pad, int64_t n_slots, uint64_t h0, Item item, int64_t* __restrict__ out)
{
    const int64_t total = n_sets * n_slots;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / n_slots;
        const int64_t beg = set_ptr[r];
        const bool has_pad = row_has_pad ? (row_has_pad[r] != 0) : true;
        const int64_t k = nanchor_pick(h0, item(r) * (uint64_t)n_slots + (uint64_t)(t - r * n_slots), set_ptr[r + 1] - beg, has_pad);
        out[t] = k < 0 ? 0 : set_nodes[beg + k];
    }
}

extern "C" int sgnn_sample_anchors_padded(const int64_t* ids, int64_t n_rows, int64_t L, int64_t n_slots,
                                          uint64_t seed, uint64_t stream_id, int64_t* out, void* stream)
{
    if (!ids || !out || n_rows < 0 || L < 0 || n_slots < 0) return SGNN_ERR_BAD_ARG;
    if (L >= (1ll << 32)) return SGNN_ERR_SET_TOO_LARGE;
    if (n_rows == 0 || n_slots == 0) return SGNN_OK;
    hipLaunchKernelGGL(sample_anchors_padded_kernel, dim3(sgnn_grid_for(n_rows * n_slots, 256)), dim3(256), 0,
                       (hipStream_t)stream, ids, n_rows, L, n_slots, sgnn_tape_h0(seed, stream_id), out);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

template <class Item>
static int launch_sample_anchors_ragged(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, const uint8_t* row_has_pad,
                                        int64_t n_slots, uint64_t seed, uint64_t stream_id, Item item, int64_t* out, void* stream)
{
    if (n_sets == 0 || n_slots == 0) return SGNN_OK;
    hipLaunchKernelGGL(sample_anchors_ragged_kernel<Item>, dim3(sgnn_grid_for(n_sets * n_slots, 256)), dim3(256), 0,
                       (hipStream_t)stream, set_ptr, set_nodes, n_sets, row_has_pad, n_slots,
                       sgnn_tape_h0(seed, stream_id), item, out);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_sample_anchors_ragged(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                          const uint8_t* row_has_pad, int64_t n_slots,
                                          uint64_t seed, uint64_t stream_id, int64_t item_base, int64_t* out, void* stream)
{
    if (!set_ptr || !set_nodes || !out || n_sets < 0 || n_slots < 0 || item_base < 0) return SGNN_ERR_BAD_ARG;
    return launch_sample_anchors_ragged(set_ptr, set_nodes, n_sets, row_has_pad, n_slots, seed, stream_id, ItemOfRow{item_base}, out,
                                        stream);
}

extern "C" int sgnn_sample_anchors_ragged_keyed(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                                const uint8_t* row_has_pad, const uint64_t* keys, int64_t n_slots,
                                                uint64_t seed, uint64_t stream_id, int64_t* out, void* stream)
{
    if (!set_ptr || !set_nodes || !row_has_pad || !keys || !out || n_sets < 0 || n_slots < 0) return SGNN_ERR_BAD_ARG;
    return launch_sample_anchors_ragged(set_ptr, set_nodes, n_sets, row_has_pad, n_slots, seed, stream_id, ItemOfKey{keys}, out,
                                        stream);
}

// Neighbourhood-border anchors drawn from KEPT sorted borders (sgnn_khop1_border_sorted): the law of
// sample_anchors_ragged_kernel with has_pad = counts[r] < width[0], and the slot's similarity (the hop level, 0 on PAD) in the
// same launch -- what khop1_sample_kernel + khop_sample_finish_kernel produce together, without rebuilding the border.
// Two border forms share the kernel: KEPT one-hop borders (counts beside ptr, the PAD rule from the matrix's width, one hop for
// all) and KEYED borders of any depth (the caller's row_has_pad, a hop per entry).
struct BorderOfWidth {
    const int64_t* __restrict__ counts;
    const int64_t* __restrict__ width;
    float hop;
    __device__ int64_t n(const int64_t*, int64_t r) const { return counts[r]; }
    __device__ bool has_pad(int64_t r, int64_t n) const { return n < width[0]; }
    __device__ float sim(int64_t) const { return hop; }
};
struct BorderOfFlags {
    const uint8_t* __restrict__ row_has_pad;
    const uint8_t* __restrict__ hops;
    __device__ int64_t n(const int64_t* ptr, int64_t r) const { return ptr[r + 1] - ptr[r]; }
    __device__ bool has_pad(int64_t r, int64_t) const { return row_has_pad[r] != 0; }
    __device__ float sim(int64_t e) const { return (float)hops[e]; }
};

template <class Item, class Border>
__global__ __launch_bounds__(256) void sample_anchors_border_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ ids, int64_t n_sets, Border border, int64_t n_slots, uint64_t h0,
    Item item, int64_t* __restrict__ out_anchor, float* __restrict__ out_sims)
{
    const int64_t total = n_sets * n_slots;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / n_slots;
        const int64_t n = border.n(ptr, r);
        const int64_t k = nanchor_pick(h0, item(r) * (uint64_t)n_slots + (uint64_t)(t - r * n_slots), n, border.has_pad(r, n));
        const int64_t v = k < 0 ? 0 : ids[ptr[r] + k];
        out_anchor[t] = v;
        out_sims[t] = v == 0 ? 0.f : border.sim(ptr[r] + k);
    }
}

extern "C" int sgnn_sample_border_anchors(const int64_t* ptr, const int32_t* ids, const int64_t* counts, int64_t n_sets,
                                          const int64_t* width, int64_t n_slots, uint64_t seed, uint64_t stream_id,
                                          int64_t item_base, int hop, int64_t* out_anchor, float* out_sims, void* stream)
{
    if (!ptr || !ids || !counts || !width || !out_anchor || !out_sims || n_sets < 0 || n_slots < 0 || item_base < 0 || hop < 0)
        return SGNN_ERR_BAD_ARG;
    if (n_sets == 0 || n_slots == 0) return SGNN_OK;
    hipLaunchKernelGGL((sample_anchors_border_kernel<ItemOfRow, BorderOfWidth>), dim3(sgnn_grid_for(n_sets * n_slots, 256)), dim3(256),
                       0, (hipStream_t)stream, ptr, ids, n_sets, BorderOfWidth{counts, width, (float)hop}, n_slots,
                       sgnn_tape_h0(seed, stream_id), ItemOfRow{item_base}, out_anchor, out_sims);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_sample_border_anchors_keyed(const int64_t* ptr, const int32_t* ids, const uint8_t* hops, int64_t n_sets,
                                                const uint8_t* row_has_pad, const uint64_t* keys, int64_t n_slots, uint64_t seed,
                                                uint64_t stream_id, int64_t* out_anchor, float* out_sims, void* stream)
{
    if (!ptr || !ids || !hops || !row_has_pad || !keys || !out_anchor || !out_sims || n_sets < 0 || n_slots < 0)
        return SGNN_ERR_BAD_ARG;
    if (n_sets == 0 || n_slots == 0) return SGNN_OK;
    hipLaunchKernelGGL((sample_anchors_border_kernel<ItemOfKey, BorderOfFlags>), dim3(sgnn_grid_for(n_sets * n_slots, 256)), dim3(256),
                       0, (hipStream_t)stream, ptr, ids, n_sets, BorderOfFlags{row_has_pad, hops}, n_slots,
                       sgnn_tape_h0(seed, stream_id), ItemOfKey{keys}, out_anchor, out_sims);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

// ---------------------------------------------------------------------------------------------
// a5/a6  np.random.choice(seq, n, replace=True) (reference anchor_patch_samplers.py:206,208,326)
// ---------------------------------------------------------------------------------------------
template <class Item>
__global__ void choice_ragged_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ seq,
                                     int64_t n_items, int64_t n_draws, uint64_t h0, Item item,
                                     int64_t* __restrict__ out)
{
    const int64_t total = n_items * n_draws;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / n_draws, j = t % n_draws;
        const int64_t beg = ptr[r];
        const int64_t n = ptr[r + 1] - beg;
        int64_t v = 0;
        if (n > 0) v = seq[beg + sgnn_choice_index(sgnn_tape_h1(h0, item(r)), (uint64_t)j, (uint32_t)n)];
        out[t] = v;
    }
}

template <class Item>
static int launch_choice_ragged(const int64_t* ptr, const int32_t* seq, int64_t n_items, int64_t n_draws, uint64_t seed,
                                uint64_t stream_id, Item item, int64_t* out, void* stream)
{
    if (n_items * n_draws == 0) return SGNN_OK;
    hipLaunchKernelGGL(choice_ragged_kernel<Item>, dim3(sgnn_grid_for(n_items * n_draws, 256)), dim3(256), 0,
                       (hipStream_t)stream, ptr, seq, n_items, n_draws, sgnn_tape_h0(seed, stream_id), item, out);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_choice_ragged(const int64_t* ptr, const int32_t* seq, int64_t n_items, int64_t n_draws,
                                  uint64_t seed, uint64_t stream_id, int64_t item_base, int64_t* out, void* stream)
{
    if (!ptr || !seq || !out || n_items < 0 || n_draws < 0 || item_base < 0) return SGNN_ERR_BAD_ARG;
    return launch_choice_ragged(ptr, seq, n_items, n_draws, seed, stream_id, ItemOfRow{item_base}, out, stream);
}

extern "C" int sgnn_choice_ragged_keyed(const int64_t* ptr, const int32_t* seq, int64_t n_items, const uint64_t* keys,
                                        int64_t n_draws, uint64_t seed, uint64_t stream_id, int64_t* out, void* stream)
{
    if (!ptr || !seq || !keys || !out || n_items < 0 || n_draws < 0) return SGNN_ERR_BAD_ARG;
    return launch_choice_ragged(ptr, seq, n_items, n_draws, seed, stream_id, ItemOfKey{keys}, out, stream);
}

// ---------------------------------------------------------------------------------------------
// Content key of a ragged set (subgnn_hip.h, sgnn_set_keys): one wavefront per set, lane l sums sgnn_mix64 of entries l, l + 64,
// ... (uint64 wrap-around: the sum commutes, so the order of the entries does not matter), a butterfly adds the 64 partial sums.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void set_keys_kernel(const int64_t* __restrict__ set_ptr, const int32_t* __restrict__ set_nodes,
                                                       int64_t n_sets, uint64_t* __restrict__ out_keys)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t s = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); s < n_sets; s += waves) {
        const int64_t beg = set_ptr[s], n = set_ptr[s + 1] - beg;
        uint64_t acc = 0;
        for (int64_t i = lane; i < n; i += 64) acc += sgnn_mix64((uint64_t)(uint32_t)set_nodes[beg + i]);
        acc = sgnn_wave_sum_u64(acc);
        if (lane == 0) out_keys[s] = sgnn_set_key_finish(acc, (uint64_t)(n > 0 ? n : 0));
    }
}

extern "C" int sgnn_set_keys(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, uint64_t* out_keys, void* stream)
{
    if (!set_ptr || !set_nodes || !out_keys || n_sets < 0) return SGNN_ERR_BAD_ARG;
    if (n_sets == 0) return SGNN_OK;
    hipLaunchKernelGGL(set_keys_kernel, dim3(sgnn_grid_for(n_sets, 4)), dim3(256), 0, (hipStream_t)stream, set_ptr, set_nodes, n_sets,
                       out_keys);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

// ---------------------------------------------------------------------------------------------
// a1-a3  triangular random walks (reference SubGNN/anchor_patch_samplers.py:20-158, 210-243)
// One WAVEFRONT per walk.  A walk is a serial dependent chain (each step needs the previous
// node), so walks run in parallel across wavefronts, and inside a step the 64 lanes share the
// work that dominates on hub nodes: the neighbour list of the current node is streamed in
// networkx order 64 entries at a time (coalesced), every lane classifies its entry (valid for
// the mode?  adjacent to the previous node? -- binary search in that node's sorted list), and
// wavefront ballots + popcounts give the triangle / non-triangle counts (pass 1) and the
// position of the drawn candidate (pass 2).  The walk state (tape counter, prev, curr) is
// wave-uniform.  Latency-bound integer work; the walks are few (patches x walks).
// No launch rule chooses this kernel: it is the device-side reference the tests compare the workgroup kernels below against
// (kernel = 1).  That is why it keeps its OWN copy of the walk (the body of triangular_walks_kernel, walk_count, walk_pick,
// walk_build_hash) and shares only WalkCtx and walk_valid with them: sharing a body would compare that body with itself.
// ---------------------------------------------------------------------------------------------
#define WK_HASH_BITS 8
#define WK_HASH (1 << WK_HASH_BITS)
#define WK_HASH_MAX 96          // patches / in-border sets up to this size use the LDS hash (else linear scan)
#define WK_CHUNKS 1024          // classification masks cached for neighbour lists up to 64 * WK_CHUNKS entries

struct WalkCtx {
    const int64_t* rowptr;
    const int32_t* col;
    const int32_t* col_sorted;
    const int32_t* patch;     // patch node view (mode 1/2), unique ids
    int32_t n_patch;
    const int32_t* inb;       // in-border nodes (mode 2)
    int32_t n_inb;
    int mode;
    const int32_t* hpatch;    // LDS hash of the patch (nullptr: linear scan)
    const int32_t* hinb;      // LDS hash of the in-border set
    int pp, pi;               // wave-uniform probe counts of the two hashes
};

__device__ static inline bool walk_in_list(const int32_t* a, int32_t n, int32_t v) {
    for (int32_t i = 0; i < n; ++i)
        if (a[i] == v) return true;
    return false;
}

__device__ static inline bool walk_in_hash(const int32_t* h, int P, int32_t v) {
    const uint32_t b = sgnn_hash32((uint32_t)v) >> (32 - WK_HASH_BITS);
    int hit = 0;
    for (int p = 0; p < P; ++p) hit |= (h[(b + p) & (WK_HASH - 1)] == v);
    return hit != 0;
}

// wave-cooperative build of a membership hash; returns the longest probe chain (wave-uniform)
__device__ static inline int walk_build_hash(int32_t* h, const int32_t* a, int32_t n, int lane) {
#pragma unroll
    for (int q = 0; q < WK_HASH / 64; ++q) h[lane + 64 * q] = 0;
    __syncthreads();
    int chain = 0;
    for (int i = lane; i < n; i += 64) {
        const int32_t v = a[i];
        uint32_t b = sgnn_hash32((uint32_t)v) >> (32 - WK_HASH_BITS);
        int c = 0;
        while (true) {
            ++c;
            const int32_t old = atomicCAS(&h[b], 0, v);
            if (old == 0 || old == v) break;
            b = (b + 1) & (WK_HASH - 1);
        }
        chain = c > chain ? c : chain;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(chain, d); chain = o > chain ? o : chain; }
    __syncthreads();
    return chain;
}

__device__ static inline bool walk_valid(const WalkCtx& c, int32_t v) {
    if (c.mode == 0) return true;
    const bool member = c.hpatch ? walk_in_hash(c.hpatch, c.pp, v) : walk_in_list(c.patch, c.n_patch, v);
    if (c.mode == 1) return member;
    if (!member) return true;                                                        // aps:143
    return c.hinb ? walk_in_hash(c.hinb, c.pi, v) : walk_in_list(c.inb, c.n_inb, v);
}

// pass 1: classify the valid neighbours of v (adjacent to prev or not; prev = 0: no test), count both
// classes and keep the per-chunk ballots in LDS for pass 2 (lists longer than the cache: not kept)
__device__ static inline void walk_count(const WalkCtx& c, int32_t v, int32_t prev, int lane, int32_t& nt, int32_t& nn,
                                         uint64_t* s_tri, uint64_t* s_non) {
    const int64_t r0 = c.rowptr[v], r1 = c.rowptr[v + 1];
    int64_t p0 = 0;
    int32_t pdeg = 0;
    if (prev) { p0 = c.rowptr[prev]; pdeg = (int32_t)(c.rowptr[prev + 1] - p0); }
    nt = 0; nn = 0;
    int chunk = 0;
    for (int64_t base = r0; base < r1; base += 64, ++chunk) {
        const int64_t e = base + lane;
        bool ok = false, tri = false;
        if (e < r1) {
            const int32_t w = c.col[e];
            ok = walk_valid(c, w);
            if (ok && prev) tri = sgnn_sorted_contains(c.col_sorted + p0, pdeg, w);
        }
        const uint64_t mt = __ballot(ok && tri), mn = __ballot(ok && !tri);
        if (chunk < WK_CHUNKS && lane == 0) { s_tri[chunk] = mt; s_non[chunk] = mn; }
        nt += __popcll(mt);
        nn += __popcll(mn);
    }
}

// pass 2: the pick-th (0-based, adjacency order) valid neighbour of v in the wanted class, from the
// cached ballots (one load of col[]), or by re-classifying when the list exceeded the cache
__device__ static inline int32_t walk_pick(const WalkCtx& c, int32_t v, int32_t prev, bool want_tri, int32_t pick, int lane,
                                           const uint64_t* s_tri, const uint64_t* s_non) {
    const int64_t r0 = c.rowptr[v], r1 = c.rowptr[v + 1];
    const int64_t n_chunks = (r1 - r0 + 63) / 64;
    int32_t seen = 0;
    if (n_chunks <= WK_CHUNKS) {
        const uint64_t* s = want_tri ? s_tri : s_non;
        for (int64_t ch = 0; ch < n_chunks; ++ch) {
            uint64_t m = s[ch];
            const int32_t cnt = __popcll(m);
            if (seen + cnt > pick) {
                int k = pick - seen;                          // k-th set bit of m
                while (k-- > 0) m &= m - 1;
                return c.col[r0 + ch * 64 + (__ffsll((unsigned long long)m) - 1)];
            }
            seen += cnt;
        }
        return 0;
    }
    int64_t p0 = 0;
    int32_t pdeg = 0;
    if (prev) { p0 = c.rowptr[prev]; pdeg = (int32_t)(c.rowptr[prev + 1] - p0); }
    for (int64_t base = r0; base < r1; base += 64) {
        const int64_t e = base + lane;
        bool hit = false;
        int32_t w = 0;
        if (e < r1) {
            w = c.col[e];
            if (walk_valid(c, w)) {
                const bool tri = prev ? sgnn_sorted_contains(c.col_sorted + p0, pdeg, w) : false;
                hit = (tri == want_tri);
            }
        }
        const uint64_t m = __ballot(hit);
        const int32_t cnt = __popcll(m);
        if (seen + cnt > pick) {
            const int32_t rank = __popcll(m & ((1ull << lane) - 1ull));
            const uint64_t sel = __ballot(hit && (seen + rank == pick));
            const int src = __ffsll((unsigned long long)sel) - 1;
            return __shfl(w, src);
        }
        seen += cnt;
    }
    return 0;
}

__global__ __launch_bounds__(64) void triangular_walks_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ col_sorted,
    const int32_t* __restrict__ node_order, int64_t n_nodes,
    const int64_t* __restrict__ patch_ptr, const int32_t* __restrict__ patch_nodes,
    const int64_t* __restrict__ inb_ptr, const int32_t* __restrict__ inb_nodes,
    int mode, int64_t n_items, int64_t walks_per_patch, int64_t walk_len, double beta,
    uint64_t h0, int64_t item_base, int64_t* __restrict__ out)
{
    __shared__ uint64_t s_tri[WK_CHUNKS], s_non[WK_CHUNKS];
    __shared__ int32_t s_hp[WK_HASH], s_hi[WK_HASH];
    const int lane = threadIdx.x;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        int64_t* o = out + item * walk_len;
        for (int64_t t = lane; t < walk_len; t += 64) o[t] = 0;
        WalkCtx c;
        c.rowptr = rowptr; c.col = col; c.col_sorted = col_sorted; c.mode = mode;
        c.patch = nullptr; c.n_patch = 0; c.inb = nullptr; c.n_inb = 0;
        c.hpatch = nullptr; c.hinb = nullptr; c.pp = 0; c.pi = 0;
        const uint64_t h1 = sgnn_tape_h1(h0, (uint64_t)(item_base + item));   // the walk's GLOBAL number: a dealt share draws what the whole launch would
        uint64_t j = 0;
        int32_t prev;
        __syncthreads();                            // previous item's LDS tables are no longer read
        if (mode == 0) {
            prev = node_order[sgnn_choice_index(h1, j++, (uint32_t)n_nodes)];          // aps:70
        } else {
            const int64_t p = item / walks_per_patch;
            c.patch = patch_nodes + patch_ptr[p];
            c.n_patch = (int32_t)(patch_ptr[p + 1] - patch_ptr[p]);
            if (c.n_patch == 0) continue;                                              // aps:134-135
            if (c.n_patch <= WK_HASH_MAX) { c.pp = walk_build_hash(s_hp, c.patch, c.n_patch, lane); c.hpatch = s_hp; }
            if (mode == 1) {
                prev = c.patch[sgnn_choice_index(h1, j++, (uint32_t)c.n_patch)];      // aps:70
            } else {
                c.inb = inb_nodes + inb_ptr[p];
                c.n_inb = (int32_t)(inb_ptr[p + 1] - inb_ptr[p]);
                if (c.n_inb == 0) continue;        // reference raises ValueError here (aps:78)
                if (c.n_inb <= WK_HASH_MAX) { c.pi = walk_build_hash(s_hi, c.inb, c.n_inb, lane); c.hinb = s_hi; }
                prev = c.inb[sgnn_choice_index(h1, j++, (uint32_t)c.n_inb)];          // aps:78
            }
        }
        if (walk_len < 1) continue;
        __syncthreads();                            // zero fill above precedes the lane-0 writes
        if (lane == 0) o[0] = prev;
        int32_t nt, nn;
        walk_count(c, prev, 0, lane, nt, nn, s_tri, s_non);                              // aps:72,79
        if (nn == 0 || walk_len < 2) continue;                                          // aps:83-84
        __syncthreads();
        int32_t curr = walk_pick(c, prev, 0, false, (int32_t)sgnn_choice_index(h1, j++, (uint32_t)nn), lane, s_tri, s_non);   // aps:74,80
        if (lane == 0) o[1] = curr;
        for (int64_t step = 2; step < walk_len; ++step) {
            __syncthreads();                        // pass 2 of the previous step has read the masks
            walk_count(c, curr, prev, lane, nt, nn, s_tri, s_non);                       // aps:35-45
            if (nt + nn == 0) break;                                                     // aps:94
            bool want_tri;
            if (nt == 0) want_tri = false;                                               // aps:97-98
            else if (nn == 0) want_tri = true;                                           // aps:99-100
            else want_tri = (sgnn_uniform01(h1, j++) <= beta);                           // aps:102
            const int32_t pick = (int32_t)sgnn_choice_index(h1, j++, (uint32_t)(want_tri ? nt : nn));
            __syncthreads();
            const int32_t nxt = walk_pick(c, curr, prev, want_tri, pick, lane, s_tri, s_non);
            prev = curr;
            curr = nxt;
            if (lane == 0) o[step] = nxt;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Workgroup-per-walk variant (graphs whose id range fits an LDS bitmap, ~1.1 M ids).
// The wavefront-per-walk kernel above spends a step on a hub in (a) streaming the hub's list 64
// entries at a time on ONE wavefront and (b) a binary search in the previous node's sorted list
// per entry -- ~13 dependent global loads per 64 entries.  Here the 16 wavefronts of a 1024-thread
// workgroup share the list (chunks of 64 dealt round-robin), and "adjacent to prev?" is one bit
// test in an LDS bitmap that holds N(prev): when the walk moves on, the bits of the old N(prev)
// are un-set and those of the new one set by two more cooperative, coalesced streams.  The walks
// are few (patches x walks per patch), so giving each a whole CU costs nothing.
// Same tape, same draws, same results as the wavefront kernel (tests compare both).
// ---------------------------------------------------------------------------------------------
#define WKB_THREADS 1024
#define WKB_LDS_BYTES (136 * 1024)

__device__ static inline void wkb_bits(uint32_t* bm, const int32_t* __restrict__ list, int32_t n, bool set, int tid) {
    for (int32_t i = tid; i < n; i += WKB_THREADS) {
        const int32_t w = list[i];
        if (set) atomicOr(&bm[w >> 5], 1u << (w & 31)); else atomicAnd(&bm[w >> 5], ~(1u << (w & 31)));
    }
}

// workgroup-cooperative build of a membership hash by T threads; returns the longest probe chain (uniform).  s_red: a word of
// the hash's OWN -- the result is read after the last barrier, so a second build must not reset the word of the first
template <int T>
__device__ static inline int wkb_build_hash(int32_t* h, const int32_t* a, int32_t n, int tid, int32_t* s_red) {
    for (int i = tid; i < WK_HASH; i += T) h[i] = 0;
    if (tid == 0) *s_red = 0;
    __syncthreads();
    int chain = 0;
    for (int i = tid; i < n; i += T) {
        const int32_t v = a[i];
        uint32_t b = sgnn_hash32((uint32_t)v) >> (32 - WK_HASH_BITS);
        int c = 0;
        while (true) {
            ++c;
            const int32_t old = atomicCAS(&h[b], 0, v);
            if (old == 0 || old == v) break;
            b = (b + 1) & (WK_HASH - 1);
        }
        chain = c > chain ? c : chain;
    }
    if (chain) atomicMax(s_red, chain);
    __syncthreads();
    return *s_red;
}

// pass 1 on the whole workgroup: classify the valid neighbours of v, keep the per-chunk ballots
__device__ static inline void wkb_count(const WalkCtx& c, int32_t v, bool has_prev, const uint32_t* bm, int tid,
                                        int32_t& nt, int32_t& nn, uint64_t* s_tri, uint64_t* s_non, int32_t* s_cnt) {
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = c.rowptr[v], r1 = c.rowptr[v + 1];
    const int64_t n_chunks = (r1 - r0 + 63) / 64;
    if (tid == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    int32_t lt = 0, ln = 0;
    for (int64_t ch = wave; ch < n_chunks; ch += WKB_THREADS / 64) {
        const int64_t e = r0 + ch * 64 + lane;
        bool ok = false, tri = false;
        if (e < r1) {
            const int32_t w = c.col[e];
            ok = walk_valid(c, w);
            if (ok && has_prev) tri = (bm[w >> 5] >> (w & 31)) & 1u;
        }
        const uint64_t mt = __ballot(ok && tri), mn = __ballot(ok && !tri);
        if (ch < WK_CHUNKS && lane == 0) { s_tri[ch] = mt; s_non[ch] = mn; }
        lt += __popcll(mt);
        ln += __popcll(mn);
    }
    if (lane == 0 && (lt | ln)) { atomicAdd(&s_cnt[0], lt); atomicAdd(&s_cnt[1], ln); }
    __syncthreads();
    nt = s_cnt[0];
    nn = s_cnt[1];
}

// pass 2 of both workgroup kernels: the pick-th valid neighbour (adjacency order) in the wanted class of the row [r0, r1)
// -> *s_next.  CH: chunks of cached ballots; adjacent(w): the kernel's test "is w adjacent to prev?" (false without a prev)
template <int CH, class Adjacent>
__device__ static inline int32_t wk_pick(const WalkCtx& c, int64_t r0, int64_t r1, const Adjacent& adjacent, bool want_tri, int32_t pick,
                                         int tid, const uint64_t* s_tri, const uint64_t* s_non, int32_t* s_next) {
    const int lane = tid & 63;
    const int64_t n_chunks = (r1 - r0 + 63) / 64;
    if (tid < 64) {
        if (n_chunks <= CH) {
            // lane l owns chunks [l*per, (l+1)*per): popcount them, scan over the wave, the owner of the crossing walks its chunks
            const uint64_t* s = want_tri ? s_tri : s_non;
            const int per = (int)((n_chunks + 63) / 64);
            const int c0 = lane * per, c1 = (c0 + per < n_chunks) ? c0 + per : (int)n_chunks;
            int32_t mine = 0;
            for (int ch = c0; ch < c1; ++ch) mine += __popcll(s[ch]);
            int32_t incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
            const int32_t excl = incl - mine;
            if (pick >= excl && pick < incl) {
                int32_t seen = excl;
                for (int ch = c0; ch < c1; ++ch) {
                    uint64_t m = s[ch];
                    const int32_t cnt = __popcll(m);
                    if (seen + cnt > pick) {
                        int k = pick - seen;
                        while (k-- > 0) m &= m - 1;
                        *s_next = c.col[r0 + (int64_t)ch * 64 + (__ffsll((unsigned long long)m) - 1)];
                        break;
                    }
                    seen += cnt;
                }
            }
        } else {
            // list longer than the ballot cache: wavefront 0 re-classifies it in order
            int32_t seen = 0, res = 0;
            bool done = false;
            for (int64_t base = r0; base < r1 && !done; base += 64) {
                const int64_t e = base + lane;
                bool hit = false;
                int32_t w = 0;
                if (e < r1) {
                    w = c.col[e];
                    if (walk_valid(c, w)) {
                        const bool tri = adjacent(w);
                        hit = (tri == want_tri);
                    }
                }
                const uint64_t m = __ballot(hit);
                const int32_t cnt = __popcll(m);
                if (seen + cnt > pick) {
                    const int32_t rank = __popcll(m & ((1ull << lane) - 1ull));
                    const uint64_t sel = __ballot(hit && (seen + rank == pick));
                    res = __shfl(w, __ffsll((unsigned long long)sel) - 1);
                    done = true;
                }
                seen += cnt;
            }
            if (lane == 0) *s_next = res;
        }
    }
    __syncthreads();
    return *s_next;
}

__global__ __launch_bounds__(WKB_THREADS) void triangular_walks_wg_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ col_sorted,
    const int32_t* __restrict__ node_order, int64_t n_nodes,
    const int64_t* __restrict__ patch_ptr, const int32_t* __restrict__ patch_nodes,
    const int64_t* __restrict__ inb_ptr, const int32_t* __restrict__ inb_nodes,
    int mode_all, int64_t n_items, int64_t walks_per_patch, int64_t walk_len, double beta,
    uint64_t h0_all, int64_t item_base, int64_t* __restrict__ out, int64_t words, uint64_t h0_border)
{
    extern __shared__ uint32_t s_adj[];                    // bitmap over node ids: N(prev)
    __shared__ uint64_t s_tri[WK_CHUNKS], s_non[WK_CHUNKS];
    __shared__ int32_t s_hp[WK_HASH], s_hi[WK_HASH];
    __shared__ int32_t s_cnt[2], s_next, s_red[2];
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < words; i += WKB_THREADS) s_adj[i] = 0;
    __syncthreads();
    for (int64_t item_all = blockIdx.x; item_all < n_items; item_all += gridDim.x) {
        int64_t* o = out + item_all * walk_len;
        for (int64_t t = tid; t < walk_len; t += WKB_THREADS) o[t] = 0;
        // mode 3: the internal walks (items [0, n / 2): mode 1) and the border walks (items [n / 2, n): mode 2) of the same
        // patches in ONE launch -- each side draws from its own tape stream under its own walk numbers, as two launches would
        int mode = mode_all;
        int64_t item = item_all;
        uint64_t h0 = h0_all;
        if (mode_all == 3) {
            const int64_t half = n_items >> 1;
            if (item_all >= half) { mode = 2; item = item_all - half; h0 = h0_border; } else mode = 1;
        }
        WalkCtx c;
        c.rowptr = rowptr; c.col = col; c.col_sorted = col_sorted; c.mode = mode;
        c.patch = nullptr; c.n_patch = 0; c.inb = nullptr; c.n_inb = 0;
        c.hpatch = nullptr; c.hinb = nullptr; c.pp = 0; c.pi = 0;
        const uint64_t h1 = sgnn_tape_h1(h0, (uint64_t)(item_base + item));   // the walk's GLOBAL number: a dealt share draws what the whole launch would
        uint64_t j = 0;
        int32_t prev;
        __syncthreads();                            // previous item's LDS tables are no longer read
        if (mode == 0) {
            prev = node_order[sgnn_choice_index(h1, j++, (uint32_t)n_nodes)];          // aps:70
        } else {
            const int64_t p = item / walks_per_patch;
            c.patch = patch_nodes + patch_ptr[p];
            c.n_patch = (int32_t)(patch_ptr[p + 1] - patch_ptr[p]);
            if (c.n_patch == 0) continue;                                              // aps:134-135
            if (c.n_patch <= WK_HASH_MAX) { c.pp = wkb_build_hash<WKB_THREADS>(s_hp, c.patch, c.n_patch, tid, &s_red[0]); c.hpatch = s_hp; }
            if (mode == 1) {
                prev = c.patch[sgnn_choice_index(h1, j++, (uint32_t)c.n_patch)];      // aps:70
            } else {
                c.inb = inb_nodes + inb_ptr[p];
                c.n_inb = (int32_t)(inb_ptr[p + 1] - inb_ptr[p]);
                if (c.n_inb == 0) continue;        // reference raises ValueError here (aps:78)
                if (c.n_inb <= WK_HASH_MAX) { c.pi = wkb_build_hash<WKB_THREADS>(s_hi, c.inb, c.n_inb, tid, &s_red[1]); c.hinb = s_hi; }
                prev = c.inb[sgnn_choice_index(h1, j++, (uint32_t)c.n_inb)];          // aps:78
            }
        }
        if (walk_len < 1) continue;
        __syncthreads();                            // zero fill above precedes the thread-0 writes
        if (tid == 0) o[0] = prev;
        int32_t nt, nn;
        wkb_count(c, prev, false, s_adj, tid, nt, nn, s_tri, s_non, s_cnt);             // aps:72,79
        if (nn == 0 || walk_len < 2) continue;                                          // aps:83-84
        int32_t curr = wk_pick<WK_CHUNKS>(c, rowptr[prev], rowptr[prev + 1], [](int32_t) { return false; }, false,
                                          (int32_t)sgnn_choice_index(h1, j++, (uint32_t)nn), tid, s_tri, s_non, &s_next);   // aps:74,80
        if (tid == 0) o[1] = curr;
        // the bitmap holds N(prev) from here on
        wkb_bits(s_adj, col + rowptr[prev], (int32_t)(rowptr[prev + 1] - rowptr[prev]), true, tid);
        __syncthreads();
        for (int64_t step = 2; step < walk_len; ++step) {
            wkb_count(c, curr, true, s_adj, tid, nt, nn, s_tri, s_non, s_cnt);          // aps:35-45
            if (nt + nn == 0) break;                                                     // aps:94
            bool want_tri;
            if (nt == 0) want_tri = false;                                               // aps:97-98
            else if (nn == 0) want_tri = true;                                           // aps:99-100
            else want_tri = (sgnn_uniform01(h1, j++) <= beta);                           // aps:102
            const int32_t pick = (int32_t)sgnn_choice_index(h1, j++, (uint32_t)(want_tri ? nt : nn));
            const int32_t nxt = wk_pick<WK_CHUNKS>(c, rowptr[curr], rowptr[curr + 1],
                                                   [&](int32_t w) { return ((s_adj[w >> 5] >> (w & 31)) & 1u) != 0; }, want_tri, pick, tid,
                                                   s_tri, s_non, &s_next);
            if (tid == 0) o[step] = nxt;
            // N(prev) out, N(curr) in: curr becomes prev
            wkb_bits(s_adj, col + rowptr[prev], (int32_t)(rowptr[prev + 1] - rowptr[prev]), false, tid);
            __syncthreads();
            if (step + 1 < walk_len) wkb_bits(s_adj, col + rowptr[curr], (int32_t)(rowptr[curr + 1] - rowptr[curr]), true, tid);
            __syncthreads();
            prev = (step + 1 < walk_len) ? curr : 0;
            curr = nxt;
        }
        // leave the bitmap clean for the next item of this workgroup
        if (prev) wkb_bits(s_adj, col + rowptr[prev], (int32_t)(rowptr[prev + 1] - rowptr[prev]), false, tid);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Workgroup-per-walk kernel WITHOUT a bitmap over node ids: a walk owns a few KB of LDS, so several walks share a CU
// (the bitmap kernel above: one walk per CU) and no pass over N(prev) sets or clears bits when the walk moves on.  "Is
// candidate w adjacent to prev?" takes one of three forms, chosen per step by the length of N(prev):
//   1  fewer than WKS_LIST_MAX entries: N(prev) lies in LDS as an open-addressing hash of WKS_SLOTS slots (at most half full;
//      an empty slot ends a probe) -- the count pass of the step BEFORE entered it when prev was its `curr`, from the very
//      entries it classified: no second fetch.  Three tables rotate: one is read, one is filled, one is emptied for the
//      step after (the barriers the step has anyway separate the three uses)
//   2  longer, and the graph has hub tables (DeviceGraph.hub_tables, the degree sequence's): bit hub_index[prev] of row w --
//      one load per candidate, all candidates independent
//   3  longer, no tables: binary search in the global col_sorted, as the wavefront kernel does
// Same tape, same draws, same order of candidates, same early exits as the two kernels above: same walks.
// T threads (T / 64 wavefronts share a neighbour list, chunks of 64 dealt round-robin, WKS_UNROLL chunks of a wavefront in
// flight at once); CH chunks of cached ballots.
// ---------------------------------------------------------------------------------------------
#define WKS_LIST_MAX 512        // == DS_SEARCH (degree_sequence.hip): the lists that have a row in the hub tables are at least this long
#define WKS_SLOTS 1024          // slots of a list's hash (2 * WKS_LIST_MAX: an empty slot always exists)
#define WKS_UNROLL 4

struct WksAdj {
    int form;                   // 0: no previous node; 1 / 2 / 3: see above
    int32_t n;                  // form 3: entries of N(prev)
    const int32_t* lds;         // form 1: the hash of N(prev) in LDS
    const int32_t* sorted;      // form 3: col_sorted + rowptr[prev]
    const uint32_t* bits;       // form 2: hub_bits + (hub number >> 5); row w is W words further
    int64_t W;
    uint32_t bit;               // form 2: hub number & 31
};

__device__ static inline uint32_t wks_slot(int32_t v) { return sgnn_hash32((uint32_t)v) >> 22; }      // 32 - log2(WKS_SLOTS)

__device__ static inline bool wks_in_list_hash(const int32_t* h, int32_t w) {
    uint32_t b = wks_slot(w);
    while (true) {
        const int32_t x = h[b];
        if (x == w) return true;
        if (x == 0) return false;                          // ids are >= 1: 0 = empty
        b = (b + 1) & (WKS_SLOTS - 1);
    }
}

__device__ static inline void wks_list_hash_insert(int32_t* h, int32_t v) {
    uint32_t b = wks_slot(v);
    while (true) {
        const int32_t old = atomicCAS(&h[b], 0, v);
        if (old == 0 || old == v) break;
        b = (b + 1) & (WKS_SLOTS - 1);
    }
}

__device__ static inline bool wks_adjacent(const WksAdj& a, int32_t w) {
    if (a.form == 2) return ((a.bits[(int64_t)w * a.W] >> a.bit) & 1u) != 0;
    if (a.form == 1) return wks_in_list_hash(a.lds, w);
    return sgnn_sorted_contains(a.sorted, a.n, w);
}

// how the NEXT step tests adjacency to v, whose row is [r0, r1), whose hub number is hub (-1: none) and whose list the
// count pass entered into the hash `staged` if it is short
__device__ static inline WksAdj wks_adj_of(const int32_t* col_sorted, int64_t r0, int64_t r1, int32_t hub, const uint32_t* hub_bits,
                                           int64_t W, const int32_t* staged) {
    WksAdj a;
    a.n = (int32_t)(r1 - r0); a.lds = staged; a.sorted = col_sorted + r0; a.bits = nullptr; a.W = W; a.bit = 0;
    if (r1 - r0 < WKS_LIST_MAX) a.form = 1;
    else if (hub >= 0) { a.form = 2; a.bits = hub_bits + (hub >> 5); a.bit = (uint32_t)hub & 31u; }
    else a.form = 3;
    return a;
}

// pass 1 on the whole workgroup: classify the valid neighbours of the node whose row is [r0, r1), keep the per-chunk
// ballots, enter the row into the hash `stage` when it is short (it is N(prev) of the next step) and empty `clear`, the
// hash the step after fills
template <int T, int CH>
__device__ static inline void wks_count(const WalkCtx& c, int64_t r0, int64_t r1, const WksAdj& a, int32_t* stage, int32_t* clear,
                                        int tid, int32_t& nt, int32_t& nn, uint64_t* s_tri, uint64_t* s_non, int32_t* s_cnt) {
    constexpr int NW = T / 64, U = WKS_UNROLL;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t n_chunks = (r1 - r0 + 63) / 64;
    const bool short_row = r1 - r0 < WKS_LIST_MAX;
    for (int i = tid; i < WKS_SLOTS; i += T) clear[i] = 0;
    int32_t lt = 0, ln = 0;
    for (int64_t ch0 = wave; ch0 < n_chunks; ch0 += U * NW) {
        // U independent loads of col[] in flight per wavefront: issued unconditionally (a lane past the row's end re-reads its
        // first entry) and fenced, so that none is moved down to its first use behind a branch -- a list of thousands of
        // entries costs U times fewer round trips
        int32_t w[U];
        bool ok[U], tri[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e = r0 + (ch0 + u * NW) * 64 + lane;
            ok[u] = e < r1;
            w[u] = c.col[ok[u] ? e : r0];
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (short_row && ok[u]) wks_list_hash_insert(stage, w[u]);
            ok[u] = ok[u] && walk_valid(c, w[u]);
        }
        if (a.form == 2) {                                  // and U independent loads of hub-table words (row 0 for a lane without a candidate)
            uint32_t word[U];
#pragma unroll
            for (int u = 0; u < U; ++u) word[u] = a.bits[(int64_t)(ok[u] ? w[u] : 0) * a.W];
            asm volatile("" ::: "memory");
#pragma unroll
            for (int u = 0; u < U; ++u) tri[u] = ((word[u] >> a.bit) & 1u) != 0;
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) tri[u] = ok[u] && a.form && wks_adjacent(a, w[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t ch = ch0 + u * NW;
            if (ch < n_chunks) {                            // wave-uniform
                const uint64_t mt = __ballot(ok[u] && tri[u]), mn = __ballot(ok[u] && !tri[u]);
                if (ch < CH && lane == 0) { s_tri[ch] = mt; s_non[ch] = mn; }
                lt += __popcll(mt);
                ln += __popcll(mn);
            }
        }
    }
    if (lane == 0) { s_cnt[2 * wave] = lt; s_cnt[2 * wave + 1] = ln; }
    __syncthreads();
    nt = 0; nn = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) { nt += s_cnt[2 * k]; nn += s_cnt[2 * k + 1]; }
}

template <int T, int CH>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(8, 8))) void triangular_walks_lists_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ col_sorted,
    const int32_t* __restrict__ hub_index, const uint32_t* __restrict__ hub_bits, int64_t hub_words,
    const int32_t* __restrict__ node_order, int64_t n_nodes,
    const int64_t* __restrict__ patch_ptr, const int32_t* __restrict__ patch_nodes,
    const int64_t* __restrict__ inb_ptr, const int32_t* __restrict__ inb_nodes,
    int mode_all, int64_t n_items, int64_t walks_per_patch, int64_t walk_len, double beta,
    uint64_t h0_all, int64_t item_base, int64_t* __restrict__ out, uint64_t h0_border)
{
    __shared__ uint64_t s_tri[CH], s_non[CH];
    __shared__ int32_t s_list[3][WKS_SLOTS];               // hashes of N(prev) (read), N(curr) (filled), and one being emptied
    __shared__ int32_t s_hp[WK_HASH], s_hi[WK_HASH];
    __shared__ int32_t s_cnt[2 * (T / 64)], s_next, s_red[2];
    const int tid = threadIdx.x;
    for (int64_t item_all = blockIdx.x; item_all < n_items; item_all += gridDim.x) {
        int64_t* o = out + item_all * walk_len;
        for (int64_t t = tid; t < walk_len; t += T) o[t] = 0;
        // mode 3: the internal walks (items [0, n / 2): mode 1) and the border walks (items [n / 2, n): mode 2) of the same
        // patches in ONE launch -- each side draws from its own tape stream under its own walk numbers, as two launches would
        int mode = mode_all;
        int64_t item = item_all;
        uint64_t h0 = h0_all;
        if (mode_all == 3) {
            const int64_t half = n_items >> 1;
            if (item_all >= half) { mode = 2; item = item_all - half; h0 = h0_border; } else mode = 1;
        }
        WalkCtx c;
        c.rowptr = rowptr; c.col = col; c.col_sorted = col_sorted; c.mode = mode;
        c.patch = nullptr; c.n_patch = 0; c.inb = nullptr; c.n_inb = 0;
        c.hpatch = nullptr; c.hinb = nullptr; c.pp = 0; c.pi = 0;
        const uint64_t h1 = sgnn_tape_h1(h0, (uint64_t)(item_base + item));   // the walk's GLOBAL number: a dealt share draws what the whole launch would
        uint64_t j = 0;
        int32_t prev;
        __syncthreads();                            // previous item's LDS tables are no longer read
        if (mode == 0) {
            prev = node_order[sgnn_choice_index(h1, j++, (uint32_t)n_nodes)];          // aps:70
        } else {
            const int64_t p = item / walks_per_patch;
            c.patch = patch_nodes + patch_ptr[p];
            c.n_patch = (int32_t)(patch_ptr[p + 1] - patch_ptr[p]);
            if (c.n_patch == 0) continue;                                              // aps:134-135
            if (c.n_patch <= WK_HASH_MAX) { c.pp = wkb_build_hash<T>(s_hp, c.patch, c.n_patch, tid, &s_red[0]); c.hpatch = s_hp; }
            if (mode == 1) {
                prev = c.patch[sgnn_choice_index(h1, j++, (uint32_t)c.n_patch)];      // aps:70
            } else {
                c.inb = inb_nodes + inb_ptr[p];
                c.n_inb = (int32_t)(inb_ptr[p + 1] - inb_ptr[p]);
                if (c.n_inb == 0) continue;        // reference raises ValueError here (aps:78)
                if (c.n_inb <= WK_HASH_MAX) { c.pi = wkb_build_hash<T>(s_hi, c.inb, c.n_inb, tid, &s_red[1]); c.hinb = s_hi; }
                prev = c.inb[sgnn_choice_index(h1, j++, (uint32_t)c.n_inb)];          // aps:78
            }
        }
        if (walk_len < 1) continue;
        prev = __builtin_amdgcn_readfirstlane(prev);
        for (int i = tid; i < WKS_SLOTS; i += T) s_list[0][i] = 0;      // the first hash to be filled
        __syncthreads();                            // zero fill above precedes the thread-0 writes
        if (tid == 0) o[0] = prev;
        int64_t r0 = rowptr[prev], r1 = rowptr[prev + 1];
        int32_t hub = hub_index ? hub_index[prev] : -1;
        int buf = 0;
        WksAdj a;
        a.form = 0; a.n = 0; a.lds = nullptr; a.sorted = nullptr; a.bits = nullptr; a.W = 0; a.bit = 0;
        int32_t nt, nn;
        wks_count<T, CH>(c, r0, r1, a, s_list[0], s_list[1], tid, nt, nn, s_tri, s_non, s_cnt);   // aps:72,79
        if (nn == 0 || walk_len < 2) continue;                                          // aps:83-84
        const auto adjacent = [&](int32_t w) { return a.form ? wks_adjacent(a, w) : false; };
        int32_t curr = wk_pick<CH>(c, r0, r1, adjacent, false, (int32_t)sgnn_choice_index(h1, j++, (uint32_t)nn), tid,
                                   s_tri, s_non, &s_next);                               // aps:74,80
        if (tid == 0) o[1] = curr;
        for (int64_t step = 2; step < walk_len; ++step) {
            // prev's list is in s_list[buf] if it is short; curr's goes into the next hash while it is counted, the third is emptied
            a = wks_adj_of(col_sorted, r0, r1, hub, hub_bits, hub_words, s_list[buf]);
            curr = __builtin_amdgcn_readfirstlane(curr);
            r0 = rowptr[curr]; r1 = rowptr[curr + 1];
            hub = hub_index ? hub_index[curr] : -1;
            buf = buf == 2 ? 0 : buf + 1;
            wks_count<T, CH>(c, r0, r1, a, s_list[buf], s_list[buf == 2 ? 0 : buf + 1], tid, nt, nn, s_tri, s_non, s_cnt);   // aps:35-45
            if (nt + nn == 0) break;                                                     // aps:94
            bool want_tri;
            if (nt == 0) want_tri = false;                                               // aps:97-98
            else if (nn == 0) want_tri = true;                                           // aps:99-100
            else want_tri = (sgnn_uniform01(h1, j++) <= beta);                           // aps:102
            const int32_t pick = (int32_t)sgnn_choice_index(h1, j++, (uint32_t)(want_tri ? nt : nn));
            curr = wk_pick<CH>(c, r0, r1, adjacent, want_tri, pick, tid, s_tri, s_non, &s_next);
            if (tid == 0) o[step] = curr;
        }
    }
}

// a launch as the entry points describe it to the launches.  mode 3: the internal walks (items [0, n / 2): mode 1, tape h0) and the
// border walks (items [n / 2, n): mode 2, tape h0_border) of the same patches in ONE launch
struct WkArgs {
    const int64_t* rowptr; const int32_t* col; const int32_t* col_sorted;
    const int32_t* node_order; int64_t n_nodes;
    const int64_t* patch_ptr; const int32_t* patch_nodes; const int64_t* inb_ptr; const int32_t* inb_nodes;
    int mode; int64_t n_items, walks_per_patch, walk_len; double beta;
    uint64_t h0; int64_t item_base; int64_t* out; uint64_t h0_border;
};

static int wkb_launch(const WkArgs& g, int64_t max_id, hipStream_t stream)
{
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)triangular_walks_wg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WKB_LDS_BYTES);
        attr_set = true;
    }
    const int64_t words = (max_id + 32) / 32;
    hipLaunchKernelGGL(triangular_walks_wg_kernel, dim3((int)(g.n_items < 2048 ? g.n_items : 2048)), dim3(WKB_THREADS),
                       (size_t)(words * 4), stream, g.rowptr, g.col, g.col_sorted, g.node_order, g.n_nodes, g.patch_ptr,
                       g.patch_nodes, g.inb_ptr, g.inb_nodes, g.mode, g.n_items, g.walks_per_patch, g.walk_len, g.beta, g.h0,
                       g.item_base, g.out, words, g.h0_border);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

#define WKS_VARIANTS 5
static int wks_launch(const WkArgs& g, const int32_t* hub_index, const uint32_t* hub_bits, int64_t hub_words, int variant,
                      hipStream_t stream)
{
    const dim3 grid((unsigned)(g.n_items < 0x7fffffff ? g.n_items : 0x7fffffff));   // one workgroup per walk
#define WKS_GO(T, CH)                                                                                                         \
    hipLaunchKernelGGL((triangular_walks_lists_kernel<T, CH>), grid, dim3(T), 0, stream, g.rowptr, g.col, g.col_sorted,       \
                       hub_index, hub_bits, hub_words, g.node_order, g.n_nodes, g.patch_ptr, g.patch_nodes, g.inb_ptr,        \
                       g.inb_nodes, g.mode, g.n_items, g.walks_per_patch, g.walk_len, g.beta, g.h0, g.item_base, g.out,       \
                       g.h0_border)
    switch (variant) {                              // 0 (the launch rule's choice) == 2
    case 1: WKS_GO(256, 256); break;
    case 3: WKS_GO(1024, 256); break;
    case 4: WKS_GO(512, 1024); break;
    default: WKS_GO(512, 256); break;
    }
#undef WKS_GO
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_triangular_walks_variants(void) { return WKS_VARIANTS; }

// The launch rule (variant 0).  A launch of at most WKS_FEW_WALKS walks on a graph whose id bitmap fits LDS stays with the
// bitmap kernel: every walk has a CU to itself there whatever the kernel, nothing waits for a free one, and the bitmap's
// bit test in LDS beats a gathered hub-table word where walks sit among the hubs (the benchmark's 210 graph walks of 50:
// 150 us against 234 - 346 us at 1024 - 256 threads, profiles/walks_probe.json).  More walks than that queue for CUs, and
// the list kernel runs several per CU (2 x 1050 patch walks of 10: 264 -> 164 us).  Tuned on that one hub-heavy graph:
// between 210 and 2100 walks, and on graphs without hubs: not measured.
#define WKS_FEW_WALKS 256
static bool wkb_fits(int64_t max_id) { return max_id > 0 && ((max_id + 32) / 32) * 4 <= WKB_LDS_BYTES; }
static bool wks_bitmap_kernel_wins(int variant, int64_t n_walks, int64_t max_id) {
    return variant == 0 && n_walks <= WKS_FEW_WALKS && wkb_fits(max_id);
}
// what variant 0 does with a launch of n_walks walks (both sides counted): 1 = the bitmap kernel (the hub tables are not read)
extern "C" int sgnn_triangular_walks_rule(int64_t n_walks, int64_t max_id) { return wks_bitmap_kernel_wins(0, n_walks, max_id) ? 1 : 0; }

// Both entry points end here: g.mode 0 / 1 / 2, or 3 with g.n_items counting both sides.  kernel 0: the workgroup kernels (the
// rule, or the list kernel at the shape `variant` names), 1: the wavefront kernel (no mode 3), 2: the bitmap kernel.
static int wk_run(const WkArgs& g, int64_t nnz, const int32_t* hub_index, const uint32_t* hub_bits, int64_t hub_words, int64_t max_id,
                  int kernel, int variant, hipStream_t stream)
{
    if (!g.rowptr || !g.col || !g.col_sorted || !g.out || g.n_items < 0 || g.walk_len < 0 || g.item_base < 0 || g.mode < 0
        || g.mode > 3 || kernel < 0 || kernel > 2 || (kernel == 1 && g.mode == 3))
        return SGNN_ERR_BAD_ARG;
    if (variant < 0 || variant >= WKS_VARIANTS || (hub_index != nullptr) != (hub_bits != nullptr) || (hub_index && hub_words < 1))
        return SGNN_ERR_BAD_ARG;
    if (g.mode == 0 && (!g.node_order || g.n_nodes <= 0)) return SGNN_ERR_BAD_ARG;
    if (g.mode >= 1 && (!g.patch_ptr || !g.patch_nodes || g.walks_per_patch <= 0)) return SGNN_ERR_BAD_ARG;
    if (g.mode >= 2 && (!g.inb_ptr || !g.inb_nodes)) return SGNN_ERR_BAD_ARG;
    if (nnz >= (1ll << 31)) return SGNN_ERR_NNZ_TOO_LARGE;
    if (g.n_items == 0 || g.walk_len == 0) return SGNN_OK;
    if (kernel == 2 && !wkb_fits(max_id)) return SGNN_ERR_SET_TOO_LARGE;
    if (kernel == 2 || (kernel == 0 && wks_bitmap_kernel_wins(variant, g.n_items, max_id))) return wkb_launch(g, max_id, stream);
    if (kernel == 0) return wks_launch(g, hub_index, hub_bits, hub_words, variant, stream);
    hipLaunchKernelGGL(triangular_walks_kernel, dim3((int)(g.n_items < 256 * 32 ? g.n_items : 256 * 32)), dim3(64), 0, stream,
                       g.rowptr, g.col, g.col_sorted, g.node_order, g.n_nodes, g.patch_ptr, g.patch_nodes, g.inb_ptr, g.inb_nodes,
                       g.mode, g.n_items, g.walks_per_patch, g.walk_len, g.beta, g.h0, g.item_base, g.out);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_triangular_walks(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted, int64_t nnz,
                                     const int32_t* hub_index, const uint32_t* hub_bits, int64_t hub_words,
                                     const int32_t* node_order, int64_t n_nodes,
                                     const int64_t* patch_ptr, const int32_t* patch_nodes,
                                     const int64_t* inb_ptr, const int32_t* inb_nodes,
                                     int mode, int64_t n_items, int64_t walks_per_patch, int64_t walk_len, double beta,
                                     uint64_t seed, uint64_t stream_id, int64_t item_base, int64_t max_id, int kernel,
                                     int variant, int64_t* out, void* stream)
{
    if (mode > 2) return SGNN_ERR_BAD_ARG;          // the combined launch has its own entry
    const WkArgs g = {rowptr, col, col_sorted, node_order, n_nodes, patch_ptr, patch_nodes, inb_ptr, inb_nodes, mode, n_items,
                      walks_per_patch, walk_len, beta, sgnn_tape_h0(seed, stream_id), item_base, out, 0};
    return wk_run(g, nnz, hub_index, hub_bits, hub_words, max_id, kernel, variant, (hipStream_t)stream);
}

// The internal AND the border walks over the same patches (aps:118-158 called twice by the reference: inside = True / False) in
// one launch: out (2, n_items, walk_len), [0] = internal (tape stream stream_id_int), [1] = border (stream_id_bor)
extern "C" int sgnn_triangular_walks_both(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted, int64_t nnz,
                                          const int32_t* hub_index, const uint32_t* hub_bits, int64_t hub_words,
                                          const int64_t* patch_ptr, const int32_t* patch_nodes, const int64_t* inb_ptr,
                                          const int32_t* inb_nodes, int64_t n_items, int64_t walks_per_patch, int64_t walk_len,
                                          double beta, uint64_t seed, uint64_t stream_id_int, uint64_t stream_id_bor,
                                          int64_t item_base, int64_t max_id, int kernel, int variant, int64_t* out, void* stream)
{
    const WkArgs g = {rowptr, col, col_sorted, nullptr, 0, patch_ptr, patch_nodes, inb_ptr, inb_nodes, 3, 2 * n_items,
                      walks_per_patch, walk_len, beta, sgnn_tape_h0(seed, stream_id_int), item_base, out,
                      sgnn_tape_h0(seed, stream_id_bor)};
    return wk_run(g, nnz, hub_index, hub_bits, hub_words, max_id, kernel, variant, (hipStream_t)stream);
}

SGNN_DEFINE_WARM(samplers)

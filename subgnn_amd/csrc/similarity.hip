// Similarity kernels: shortest-path similarities (a9, dense-parity and sparse forms); the structure
// similarity 1/(1+fastdtw) (a11) lives in dtw.hip.
#include "common.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// a9  dense-parity form (reference SubGNN/SubGNN.py:752-781): column-wise min over the APSP rows
// of a component.  HBM-bound streaming: 8*|cc|*N bytes in, 4*N out per component; lanes walk the
// columns (coalesced 512 B per wave-instruction), the member loop re-uses nothing.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_similarity_dense_kernel(
    const double* __restrict__ apsp, int64_t n_cols,
    const int64_t* __restrict__ set_ptr, const int32_t* __restrict__ set_nodes,
    float* __restrict__ out)
{
    const int64_t r = blockIdx.y;
    const int64_t beg = set_ptr[r];
    const int n = (int)(set_ptr[r + 1] - beg);
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n_cols; c += (int64_t)gridDim.x * blockDim.x) {
        float res = 0.f;
        if (n > 0) {
            double m = apsp[(int64_t)(set_nodes[beg] - 1) * n_cols + c];
            for (int i = 1; i < n; ++i) {
                const double v = apsp[(int64_t)(set_nodes[beg + i] - 1) * n_cols + c];
                m = v < m ? v : m;
            }
            res = (float)m;
        }
        out[r * n_cols + c] = res;
    }
}

extern "C" int sgnn_sp_similarity_dense(const double* apsp, int64_t n_cols,
                                        const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                        float* out, void* stream)
{
    if (!apsp || !set_ptr || !set_nodes || !out || n_cols <= 0 || n_sets < 0) return SGNN_ERR_BAD_ARG;
    if (n_sets == 0) return SGNN_OK;
    if (n_sets > 65535 * 32768ll) return SGNN_ERR_BAD_ARG;
    int gx = (int)((n_cols + 255) / 256);
    if (gx > 64) gx = 64;
    // grid.y is limited to 65535: fold larger set counts into several launches
    for (int64_t off = 0; off < n_sets; off += 65535) {
        const int64_t cnt = (n_sets - off) < 65535 ? (n_sets - off) : 65535;
        hipLaunchKernelGGL(sp_similarity_dense_kernel, dim3(gx, (int)cnt), dim3(256), 0, (hipStream_t)stream,
                           apsp, n_cols, set_ptr + off, set_nodes, out + off * n_cols);
        SGNN_CHECK_LAUNCH();
    }
    return SGNN_OK;
}

// ---------------------------------------------------------------------------------------------
// a9  sparse form: bit-parallel multi-source BFS (msbfs_*).  Every node carries a row of 64-bit words, one bit per source.
// The host enqueues all launches of a search without synchronising; what a launch does is decided on the device.
//
// Buffers (MsbfsLayout), zeroed by msbfs_init_kernel, the sources entered by msbfs_seed_kernel:
//   B[0..2]  three row arrays.  While the search pushes they are seen | next | frontier; once it pulls, three versions of seen.
//   flags    flags[L] = level L found a new bit.  Every launch of level L returns at once when flags[L - 1] is 0: the frontier
//            died, or the closing form closed the search.
//   fvol     fvol[L] = edge volume of level L's frontier: the sum over its new words of the node's degree (push levels only).
//   fbits    two bitmaps of one bit per node: "on the current frontier" | "has ever been on a frontier" (its seen row is not empty).
//   fdone    one byte per node: every source has reached it.
//   set_seen per (set, word): the sources whose hops to the set are recorded.
//
// A level is one launch of msbfs_level_kernel.  It pushes or pulls by MsbfsPlan::mode -- a function of the level, the host's
// plan and fvol[] of the levels before, so every launch that asks gets the same answer.
//   push  : every node of the frontier bitmap ORs its frontier words into next[] of its neighbours (atomics; 16-lane groups stream
//           a list, coalesced; 64 BFS's per edge visit).  msbfs_commit_kernel follows: new = next & ~seen; seen |= new;
//           frontier = new; next = 0; dist = the level for the new bits; it writes flags, fvol, fdone and both bitmaps.
//   pull  : once a frontier's edge volume has passed 1/alpha of all edges, or beyond the ``push_levels`` levels the host enqueued a
//           commit launch for (the caller's hint, from the status of an earlier search); from then on always.  Every node that
//           still misses a source ORs its neighbours' rows into its own: no atomics, complete nodes are skipped and a list is
//           abandoned as soon as nothing is missing (on a scale-free graph almost every node is complete after 3-4 levels).
//           What a pulling node v needs from a neighbour u is "has source s reached u before this level" -- seen[u] can stand in
//           for frontier[u]: for a v that s has not reached, a neighbour with dist(u, s) <= level - 2 cannot exist (v would have
//           been reached a level earlier).  So a pull level reads ONE version of the seen rows and writes the next one
//           (seen' = seen | new) into another buffer: no next[] accumulation, no zeroing, no commit pass over three 32 MB arrays
//           (30-34 us each on the benchmark); a commit launch enqueued behind it returns at once.
// Rotation: pull number k (k pull levels ran before it) reads B[k % 3] and writes B[(k + 1) % 3].  B[(k + 2) % 3], the version
//   before, is what the set reduction of the PREVIOUS level subtracts to get that level's new bits, and that reduction is the
//   prologue of this very launch (msbfs_new_bits): two buffers would race.
// Staleness: the row of a node that every source has reached is never rewritten (fdone skips it), so it goes stale in two of the
//   three buffers.  Nobody notices: all neighbours of a complete node are complete one level later and skipped too, the set
//   reduction masks with what a set has already recorded, and the finalisation takes a complete member as all ones.  Every
//   version is a subset of the truth and the newest write of a row is exact.
// Sets (sgnn_bfs_min_hops_to_sets): level L's set reduction (msbfs_set_reduce_item) records L for the sources that reached a set
//   for the first time.  It is the prologue of level L + 1's launch -- both only READ what level L left, and the reduction writes
//   set_seen / out, which no level touches -- and the last level's runs inside msbfs_set_finalize_kernel.
// The CLOSING form (sgnn_bfs_min_hops_to_sets_closing; in front of msbfs_closing_reduce_kernel) runs the same levels over the
//   same buffers but stops once every set has its hops: the reduction is a launch behind its level, nothing is finalised.
// ---------------------------------------------------------------------------------------------
// Row stride (in 64-bit words) of the row arrays: three words (129-192 sources, the benchmark's 183) are padded to four -- a
// pull level gathers one row per neighbour, and a 24-byte row straddles two 32-byte sectors every other time (1.5 sectors per
// gather on average), a 32-byte row is always one
static constexpr int64_t msbfs_row_stride(int64_t n_words) { return n_words == 3 ? 4 : n_words; }

#define MSBFS_DEFAULT_ALPHA 32     // pull when frontier word-edges * alpha > nnz * n_words; 0 = never pull
#define MSBFS_WCHUNK 4             // source words a pull pass keeps in registers
#define MSBFS_HUB_DEGREE 128       // push: lists this long go to the whole workgroup
#define MSBFS_HUB_SLOTS 128
#define MSBFS_PULL_HUB_DEGREE 512
#ifndef MSBFS_PULL_CHECK
#define MSBFS_PULL_CHECK 2         // pull: rounds of 16 neighbours between two tests of "is anything still missing"
#endif
#define MSBFS_CLOSING_LDS_SOURCES 1024

// Byte offsets into the workspace.  The totals are exactly what the three *_workspace_bytes queries have always returned:
// each of the two alignment points is budgeted MSBFS_ALIGN_SLACK bytes whatever it consumes, and a set search
// MSBFS_SETS_SLACK bytes that nothing uses.
#define MSBFS_ALIGN_SLACK 8
#define MSBFS_SETS_SLACK 16
struct MsbfsLayout {
    int64_t seen, frontier, next;      // n_ids rows of msbfs_row_stride words each
    int64_t fvol, flags;               // max_hops + 2 entries of 8 and of 4 bytes
    int64_t fbits, fdone;              // the bitmaps now | ever in 32-bit words; n_ids bytes rounded up to whole words
    int64_t set_seen;                  // a word per (set, source word)
    int64_t closing, wanted;           // open | ticket | closed: uint32 [max_hops + 2], [max_hops + 2], [2], zeroed with set_seen; as set_seen
    int64_t total;
};

static constexpr int64_t msbfs_closing_state_words(int max_hops) { return (2 * ((int64_t)max_hops + 2) + 2 + 1) / 2; }   // 64-bit words

// n_sets < 0: no set search (sgnn_bfs_hops)
static constexpr MsbfsLayout msbfs_layout(int64_t max_id, int64_t n_sources, int max_hops, int64_t n_sets, bool closing)
{
    const int64_t n_ids = max_id + 1, n_words = (n_sources + 63) / 64, levels = (int64_t)max_hops + 2;
    const int64_t rows = n_ids * msbfs_row_stride(n_words) * 8, items = n_sets < 0 ? 0 : n_sets * n_words * 8;
    MsbfsLayout L = {};
    int64_t at = 0, slack = 0;         // slack: budgeted and not consumed
    L.seen = at; at += rows;
    L.frontier = at; at += rows;
    L.next = at; at += rows;
    L.fvol = at; at += levels * 8;
    L.flags = at; at += levels * 4;
    slack += MSBFS_ALIGN_SLACK - (-at & 7); at += -at & 7;
    L.fbits = at; at += 2 * ((n_ids + 31) / 32) * 4;
    L.fdone = at; at += ((n_ids + 3) / 4) * 4;
    slack += MSBFS_ALIGN_SLACK - (-at & 7); at += -at & 7;
    L.set_seen = at; at += items;
    if (n_sets >= 0) slack += MSBFS_SETS_SLACK;
    L.closing = at; at += closing ? 8 * msbfs_closing_state_words(max_hops) : 0;
    L.wanted = at; at += closing ? items : 0;
    L.total = at + slack;
    return L;
}
// (1000 ids + 1, 70 sources: stride 2, the second alignment point consumes 4 bytes; 10^6 ids, 183 sources: stride 4, the first does)
static_assert(msbfs_layout(1000, 70, 16, -1, false).total == 49540 && msbfs_layout(999999, 183, 33, -1, false).total == 97250436, "sgnn_bfs_hops_workspace_bytes");
static_assert(msbfs_layout(1000, 70, 16, 10, false).total == 49716 && msbfs_layout(999999, 183, 33, 50000, false).total == 98450452, "sgnn_bfs_min_hops_workspace_bytes");
static_assert(msbfs_layout(1000, 70, 16, 10, true).total == 50028 && msbfs_layout(999999, 183, 33, 50000, true).total == 99650740, "sgnn_bfs_min_hops_closing_workspace_bytes");

struct MsbfsBufs { uint64_t* b[3]; };      // seen, next, frontier: in pull mode three versions of the seen rows (see above)

struct MsbfsSets {                 // the set reduction's operands (n_sets = 0: none)
    const int64_t* set_ptr;
    const int32_t* set_nodes;
    int64_t n_sets;
    uint64_t* set_seen;
    float* out;
};

// Which form a level takes: pull(l) for l >= 2 is sticky -- pull(l - 1), or the frontier volume level l - 1 left behind exceeds
// the threshold, or l lies beyond the levels the host enqueued a commit launch for.  pulls_before = the number of pull levels
// in front of the level (the version rotation's k).
struct MsbfsMode { bool pull, prev_pull; int pulls_before; };

struct MsbfsPlan {
    const unsigned long long* fvol;
    unsigned long long pull_above;     // ~0: never by volume
    int push_levels;

    __device__ __forceinline__ MsbfsMode mode(int level) const
    {
        bool p = false, pp = false;
        int k = 0;
        for (int l = 2; l <= level; ++l) {
            const bool pl = p || l > push_levels || (pull_above != ~0ull && fvol[l - 1] > pull_above);
            if (l < level) k += pl ? 1 : 0;
            pp = p;
            p = pl;
        }
        return {p, (level >= 2) ? pp : false, k};
    }
    // versions of the seen rows the pull levels among the first ``last_level`` levels wrote (a level runs while flags[] of the
    // one before is set): the newest version is B[versions_written % 3] (no pull: the commits kept B[0] current)
    __device__ __forceinline__ int versions_written(const int32_t* __restrict__ flags, int last_level) const
    {
        int n = 0;
        for (int l = 2; l <= last_level && flags[l - 1] != 0; ++l) n += mode(l).pull ? 1 : 0;
        return n;
    }
};

// Where a level left its new bits: the seeds and a push level (its commit) in the frontier rows B[2]; pull number k as the
// difference of the version it wrote, B[(k + 1) % 3], and the one it read, B[k % 3]
struct MsbfsNew { const uint64_t* cur; const uint64_t* old; };

__device__ __forceinline__ MsbfsNew msbfs_new_bits(const MsbfsBufs& B, bool pulled, int k)
{
    if (pulled) return {B.b[(k + 1) % 3], B.b[k % 3]};
    return {B.b[2], nullptr};
}

// the bits of word w that are sources
__device__ __forceinline__ uint64_t msbfs_valid(int64_t n_sources, int64_t w)
{
    const int64_t left = n_sources - w * 64;
    return left >= 64 ? ~0ull : ((1ull << left) - 1);
}

// f(s) for every source s whose bit of word w is set in ``bits``
template <class F>
__device__ __forceinline__ void msbfs_each_source(uint64_t bits, int64_t w, int64_t n_sources, F f)
{
    while (bits) {
        const int b = __ffsll((unsigned long long)bits) - 1;
        bits &= bits - 1;
        const int64_t s = w * 64 + b;
        if (s < n_sources) f(s);
    }
}

// CH words of a node's row from word w0 on; words at or beyond the stride read as 0 and are not stored.  A row of stride 4 is
// one 32-byte sector: two 16-byte accesses, no per-word tests.
template <int CH>
struct MsbfsRow {
    static_assert(CH == 4, "the stride-4 form is the whole chunk");
    uint64_t w[CH];

    __device__ __forceinline__ void load_words(const uint64_t* __restrict__ buf, int64_t v, int64_t rs, int64_t w0)
    {
#pragma unroll
        for (int q = 0; q < CH; ++q) w[q] = (w0 + q < rs) ? buf[v * rs + w0 + q] : 0;
    }
    __device__ __forceinline__ void load(const uint64_t* __restrict__ buf, int64_t v, int64_t rs, int64_t w0)
    {
        if (rs == 4) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(&buf[v * 4]);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(&buf[v * 4 + 2]);
            w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
        } else
            load_words(buf, v, rs, w0);
    }
    // |= the row of u; in the generic form only the words ``need`` still misses something of are read
    __device__ __forceinline__ void gather(const uint64_t* __restrict__ buf, int64_t u, int64_t rs, int64_t w0, const MsbfsRow& need)
    {
        if (rs == 4) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(&buf[u * 4]);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(&buf[u * 4 + 2]);
            w[0] |= a.x; w[1] |= a.y; w[2] |= b.x; w[3] |= b.y;
        } else {
#pragma unroll
            for (int q = 0; q < CH; ++q)
                if (need.w[q]) w[q] |= buf[u * rs + w0 + q];
        }
    }
    __device__ __forceinline__ void store(uint64_t* __restrict__ buf, int64_t v, int64_t rs, int64_t w0) const
    {
        if (rs == 4) {
            *reinterpret_cast<ulonglong2*>(&buf[v * 4]) = make_ulonglong2(w[0], w[1]);
            *reinterpret_cast<ulonglong2*>(&buf[v * 4 + 2]) = make_ulonglong2(w[2], w[3]);
        } else {
#pragma unroll
            for (int q = 0; q < CH; ++q)
                if (w0 + q < rs) buf[v * rs + w0 + q] = w[q];
        }
    }
};

__global__ void msbfs_init_kernel(const int32_t* __restrict__ sources, int64_t n_sources, int64_t n_words,
                                  int64_t n_ids, uint64_t* __restrict__ seen, uint64_t* __restrict__ frontier,
                                  uint64_t* __restrict__ next, uint8_t* __restrict__ dist, int32_t* __restrict__ flags,
                                  unsigned long long* __restrict__ fvol, uint32_t* __restrict__ fbits,
                                  int max_hops, int64_t rs,  // dist layout-agnostic: filled as a flat array
                                  uint64_t* __restrict__ set_seen, int64_t n_set_words, float* __restrict__ set_out, int64_t n_set_out)
{
    const int64_t gtid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = gtid; i < 2 * ((n_ids + 31) / 32) + (n_ids + 3) / 4; i += gsz) fbits[i] = 0;   // both bitmaps and fdone behind them
    for (int64_t i = gtid; i < n_ids * rs; i += gsz) { seen[i] = 0; frontier[i] = 0; next[i] = 0; }
    for (int64_t i = gtid; i < n_set_words; i += gsz) set_seen[i] = 0;             // (with the closing state behind it)
    for (int64_t i = gtid; i < n_set_out; i += gsz) set_out[i] = 0.f;              // unreachable pairs hold 0
    if (dist) for (int64_t i = gtid; i < n_sources * n_ids; i += gsz) dist[i] = 255;
    for (int64_t i = gtid; i <= max_hops; i += gsz) { flags[i] = (i == 0) ? 1 : 0; fvol[i] = 0; }
}

__global__ void msbfs_seed_kernel(const int32_t* __restrict__ sources, int64_t n_sources, int64_t n_words,
                                  int64_t n_ids, uint64_t* __restrict__ seen, uint64_t* __restrict__ frontier,
                                  uint8_t* __restrict__ dist, int64_t ss, int64_t sv, uint32_t* __restrict__ fbits, int64_t rs)
{
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= n_sources) return;
    const int32_t v = sources[s];
    atomicOr(&fbits[v >> 5], 1u << (v & 31));                 // level-0 frontier nodes
    atomicOr(&fbits[((n_ids + 31) / 32) + (v >> 5)], 1u << (v & 31));   // ... which have a non-empty seen row from now on
    const uint64_t bit = 1ull << (s & 63);
    atomicOr((unsigned long long*)&seen[(int64_t)v * rs + (s >> 6)], (unsigned long long)bit);
    atomicOr((unsigned long long*)&frontier[(int64_t)v * rs + (s >> 6)], (unsigned long long)bit);
    if (dist) dist[s * ss + v * sv] = 0;
}

__device__ __forceinline__ uint32_t msbfs_row_or32(uint32_t v)
{
    // OR over the 16 lanes of a DPP row by rotations: every lane ends with the full value (no LDS crossbar trips:
    // the xor-butterfly on __shfl_xor was 8 ds_bpermute per 64-bit word and call)
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);     // row_ror:8
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);     // row_ror:4
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);     // row_ror:2
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);     // row_ror:1
    return v;
}

__device__ __forceinline__ uint64_t msbfs_group_or(uint64_t x)
{
    // OR over the 16 lanes of a group (= one DPP row; all lanes of the wavefront must be executing)
    return ((uint64_t)msbfs_row_or32((uint32_t)(x >> 32)) << 32) | msbfs_row_or32((uint32_t)x);
}

// One thread per (set, word) item t: which sources reached a member of the set for the first time at ``level``?  The members'
// new bits are OR-ed, masked with ``want`` and with what the set has recorded, and the level is written for those sources:
// out[set, source] = min over members of the hop distance, without a (sources x nodes) hop table.
// -> the wanted sources the set still misses
__device__ __forceinline__ uint64_t msbfs_set_reduce_item(MsbfsNew nb, int64_t n_words, int64_t n_sources, const MsbfsSets& sets,
                                                          int level, int64_t rs, int64_t t, uint64_t want = ~0ull)
{
    const int64_t r = t / n_words, w = t % n_words;
    const uint64_t goal = want & msbfs_valid(n_sources, w);
    const uint64_t have = sets.set_seen[t];
    if ((goal & ~have) == 0) return 0;                       // nothing (left) to record
    uint64_t acc = 0;
    for (int64_t i = sets.set_ptr[r]; i < sets.set_ptr[r + 1]; ++i) {
        const int64_t o = (int64_t)sets.set_nodes[i] * rs + w;
        acc |= nb.old ? (nb.cur[o] & ~nb.old[o]) : nb.cur[o];
    }
    const uint64_t fresh = acc & want & ~have;
    if (fresh) {
        sets.set_seen[t] = have | fresh;
        msbfs_each_source(fresh, w, n_sources, [&](int64_t s) { sets.out[r * n_sources + s] = (float)level; });
    }
    return goal & ~(have | fresh);
}

// A group's list is long: hand node v to the whole workgroup.  -> false when the workgroup's slots are full: the group walks
// the list itself
__device__ __forceinline__ bool msbfs_park(int32_t* s_hub, int* s_nhub, int64_t v)
{
    const int sub = threadIdx.x & 15;
    int slot = 0;
    if (sub == 0) slot = atomicAdd(s_nhub, 1);
    slot = __shfl(slot, (threadIdx.x & 63) & ~15, 64);
    if (slot < MSBFS_HUB_SLOTS) {
        if (sub == 0) s_hub[slot] = (int32_t)v;
        return true;
    }
    return false;
}

// A frontier node's list is streamed by its 16-lane group -- except long lists (hubs: a BA graph of 1M nodes has lists of
// 10k+ entries, and hubs are on the frontier from level 1 on), which one group would walk for a millisecond while the rest
// of the chip is done: those are parked in LDS and streamed by the whole workgroup afterwards.  Frontier nodes are found in
// the frontier-node bitmap (125 KB), not by reading every node's row (32 MB): level 1 of the benchmark's search went from
// 55 us to the time of its 183 lists.
__device__ __forceinline__ void msbfs_push_level(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_ids, int64_t n_words, int64_t rs,
    const uint64_t* __restrict__ seen, uint64_t* __restrict__ next, const uint64_t* __restrict__ frontier,
    const uint32_t* __restrict__ fnode, int64_t group, int64_t n_groups, int32_t* s_hub, int* s_nhub)
{
    // one pass over the list for all source words: col[] is read once, and the n_words seen / next words of a neighbour
    // are contiguous
    auto stream = [&](int64_t v, int64_t e0, int64_t r1, int64_t stride) {
        for (int64_t e = e0; e < r1; e += stride) {
            const int64_t u = col[e];
            for (int64_t w = 0; w < n_words; ++w) {
                const uint64_t f = frontier[v * rs + w];
                const uint64_t m = f & ~seen[u * rs + w];
                if (m) atomicOr((unsigned long long*)&next[u * rs + w], (unsigned long long)m);
            }
        }
    };
    for (int64_t v = group; v < n_ids; v += n_groups) {
        if (!((fnode[v >> 5] >> (v & 31)) & 1u)) continue;
        const int64_t r0 = rowptr[v], r1 = rowptr[v + 1];
        if (r1 - r0 >= MSBFS_HUB_DEGREE && msbfs_park(s_hub, s_nhub, v)) continue;
        stream(v, r0 + (threadIdx.x & 15), r1, 16);
    }
    __syncthreads();
    const int n_hub = *s_nhub < MSBFS_HUB_SLOTS ? *s_nhub : MSBFS_HUB_SLOTS;
    for (int h = 0; h < n_hub; ++h) {
        const int64_t v = s_hub[h];
        stream(v, rowptr[v] + threadIdx.x, rowptr[v + 1], blockDim.x);
    }
}

// Version ``in`` -> version ``out`` of the seen rows.  -> this thread recorded a new bit.
// filter: the first pull level behind push levels -- the commits kept one bit per node "has ever been on a frontier" = its seen
// row is not empty (125 KB, L2-resident), consulted before the 32-byte gather: on the benchmark's level 3 about half of the
// neighbours still have an empty row.  Later pull levels do not maintain the bits (and hardly any row is empty by then).
// ROW4: the stride is 4.  Compiled apart from the generic form: as one function with a test of the stride at every row access
// the compiler merged the two forms of the gather -- 16 + 8 bytes, then the fourth word only where still needed, behind a
// wait of its own -- and the pull levels of the benchmark's search took 8 % longer (275 -> 301, 375 -> 397, 294 -> 315 us).
template <bool ROW4>
__device__ __forceinline__ bool msbfs_pull_level(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_ids, int64_t n_words, int64_t n_sources,
    int64_t stride, const uint64_t* __restrict__ in, uint64_t* __restrict__ out, bool filter, const uint32_t* __restrict__ fany,
    uint8_t* __restrict__ fdone, uint8_t* __restrict__ dist, int64_t ss, int64_t sv, int level, int64_t group, int64_t n_groups,
    int32_t* s_hub, int* s_nhub, unsigned long long* s_acc)
{
    typedef MsbfsRow<MSBFS_WCHUNK> Row;
    const int64_t rs = ROW4 ? 4 : stride;
    if (!ROW4) __builtin_assume(rs != 4);
    const int sub = threadIdx.x & 15;
    bool found = false;
    // row state of a chunk: need = the sources ``have`` misses.  -> their OR
    auto missing_of = [&](const Row& have, Row& need, int64_t w0) {
        uint64_t missing = 0;
#pragma unroll
        for (int q = 0; q < MSBFS_WCHUNK; ++q) {
            need.w[q] = (w0 + q < n_words ? msbfs_valid(n_sources, w0 + q) : 0) & ~have.w[q];
            missing |= need.w[q];
        }
        return missing;
    };
    auto gather = [&](Row& acc, const Row& need, int64_t u, int64_t w0) {
        if (!filter || ((fany[u >> 5] >> (u & 31)) & 1u)) acc.gather(in, u, rs, w0, need);
    };
    // ``got`` holds what the neighbours gave: write the next version of the row, every word of it (the target buffer holds an
    // older version) -- lane 0 the whole chunk, or lane q word q -- and lane q records word q's new bits.
    // -> nothing of the chunk is missing any more
    auto finish = [&](int64_t v, int64_t w0, const Row& have, const Row& need, const Row& got, int lane, bool lane0_writes_chunk) {
        Row fresh, row;
        bool complete = true;
#pragma unroll
        for (int q = 0; q < MSBFS_WCHUNK; ++q) {
            fresh.w[q] = got.w[q] & need.w[q];
            row.w[q] = have.w[q] | fresh.w[q];
            if (need.w[q] & ~fresh.w[q]) complete = false;
        }
        if (lane0_writes_chunk && lane == 0) row.store(out, v, rs, w0);
#pragma unroll
        for (int q = 0; q < MSBFS_WCHUNK; ++q) {             // (static register indices)
            if (lane != q) continue;
            if (!lane0_writes_chunk && w0 + q < rs) out[v * rs + w0 + q] = row.w[q];
            if (fresh.w[q]) {
                found = true;
                if (dist) msbfs_each_source(fresh.w[q], w0 + q, n_sources, [&](int64_t s) { dist[s * ss + v * sv] = (uint8_t)level; });
            }
        }
        return complete;
    };
    for (int64_t v = group; v < n_ids; v += n_groups) {
        // every source has reached it -- from level 3-4 on that is almost every node; such a row is not read, not rewritten
        // (it goes stale in the other versions: harmless, see the header)
        if (fdone[v]) continue;
        const int64_t r0 = rowptr[v], r1 = rowptr[v + 1];
        bool all_done = true, parked = false;
        for (int64_t w0 = 0; w0 < rs && !parked; w0 += MSBFS_WCHUNK) {
            Row have, need, acc = {};
            have.load(in, v, rs, w0);
            const uint64_t missing = missing_of(have, need, w0);
            if (missing != 0 && r1 - r0 >= MSBFS_PULL_HUB_DEGREE && msbfs_park(s_hub, s_nhub, v)) {
                parked = true;                               // all chunks of this node are done by the workgroup, below
                break;
            }
            if (missing != 0) {
                int since = 0;
                for (int64_t e = r0 + sub; e < r1 + sub; e += 16) {          // uniform trip count per group
                    if (e < r1) gather(acc, need, col[e], w0);
                    if (++since == MSBFS_PULL_CHECK) {       // every MSBFS_PULL_CHECK x 16 neighbours: anything still missing?
                        since = 0;
                        uint64_t left = 0;
#pragma unroll
                        for (int q = 0; q < MSBFS_WCHUNK; ++q) { acc.w[q] = msbfs_group_or(acc.w[q]); left |= need.w[q] & ~acc.w[q]; }
                        if (left == 0) break;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < MSBFS_WCHUNK; ++q) acc.w[q] = missing != 0 ? msbfs_group_or(acc.w[q]) : 0;
            if (!finish(v, w0, have, need, acc, sub, true)) all_done = false;
        }
        // (a byte per node, plain store: as bits in shared words this was an atomic OR per completing node -- 830k of them on the
        // level that completes most nodes, from workgroups on all XCDs into 1000 cache lines: 2.5x the level's time)
        if (!parked && all_done && sub == 0) fdone[v] = 1;
    }
    // parked long lists: 256 lanes per list, the words OR-ed through LDS
    __syncthreads();
    const int n_hub = *s_nhub < MSBFS_HUB_SLOTS ? *s_nhub : MSBFS_HUB_SLOTS;
    for (int h = 0; h < n_hub; ++h) {
        const int64_t v = s_hub[h];
        const int64_t r0 = rowptr[v], r1 = rowptr[v + 1];
        bool all_done = true;
        for (int64_t w0 = 0; w0 < rs; w0 += MSBFS_WCHUNK) {
            Row have, need, acc = {}, got;
            have.load_words(in, v, rs, w0);
            const uint64_t missing = missing_of(have, need, w0);
            if (threadIdx.x < MSBFS_WCHUNK) s_acc[threadIdx.x] = 0;
            __syncthreads();
            if (missing != 0) {                              // uniform over the workgroup
                for (int64_t e = r0 + threadIdx.x; e < r1; e += blockDim.x) gather(acc, need, col[e], w0);
#pragma unroll
                for (int q = 0; q < MSBFS_WCHUNK; ++q)
                    if (acc.w[q]) atomicOr(&s_acc[q], (unsigned long long)acc.w[q]);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < MSBFS_WCHUNK; ++q) got.w[q] = s_acc[q];      // (every thread reads the same words)
            if (!finish(v, w0, have, need, got, (int)threadIdx.x, false)) all_done = false;
            __syncthreads();
        }
        if (all_done && threadIdx.x == 0) fdone[v] = 1;
    }
    return found;
}

__global__ __launch_bounds__(256) void msbfs_level_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_ids, int64_t n_words,
    int64_t n_sources, MsbfsBufs B, int32_t* __restrict__ flags, MsbfsPlan plan, int level, const uint32_t* __restrict__ fnode,
    const uint32_t* __restrict__ fany, uint8_t* __restrict__ fdone, int64_t rs, MsbfsSets sets, uint8_t* __restrict__ dist,
    int64_t ss, int64_t sv)
{
    if (level > 1 && flags[level - 1] == 0) return;          // previous level found nothing (nothing to reduce either)
    const MsbfsMode m = plan.mode(level);
    const int k = m.pulls_before;
    if (sets.n_sets > 0) {                                   // the previous level's set reduction (level 0: the seeds)
        // what it reads is not written by this launch: a pull writes B[(k + 1) % 3], a push B[1] with k = 0
        const MsbfsNew nb = msbfs_new_bits(B, m.prev_pull, k - 1);
        const int64_t total = sets.n_sets * n_words;
        for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x)
            msbfs_set_reduce_item(nb, n_words, n_sources, sets, level - 1, rs, t);
    }
    // node ids are dealt out to the workgroups round-robin (group g of workgroup b takes b + G*(g + 16 i)):
    // consecutive ids -- the oldest, highest-degree nodes of a preferential-attachment graph sit next to
    // each other at the low ids -- land in different workgroups
    const int64_t group = blockIdx.x + (int64_t)gridDim.x * (threadIdx.x >> 4);
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x >> 4);
    __shared__ int32_t s_hub[MSBFS_HUB_SLOTS];
    __shared__ int s_nhub;
    __shared__ unsigned long long s_acc[MSBFS_WCHUNK];
    if (threadIdx.x == 0) s_nhub = 0;
    __syncthreads();
    if (!m.pull) {
        msbfs_push_level(rowptr, col, n_ids, n_words, rs, B.b[0], B.b[1], B.b[2], fnode, group, n_groups, s_hub, &s_nhub);
        return;
    }
    const uint64_t* in = B.b[k % 3];
    uint64_t* out = B.b[(k + 1) % 3];
    // (the generic instance assumes rs != 4: true only because this test sends every stride-4 search to the other one)
    const bool found = rs == 4 ? msbfs_pull_level<true>(rowptr, col, n_ids, n_words, n_sources, rs, in, out, k == 0, fany, fdone, dist, ss,
                                                        sv, level, group, n_groups, s_hub, &s_nhub, s_acc)
                               : msbfs_pull_level<false>(rowptr, col, n_ids, n_words, n_sources, rs, in, out, k == 0, fany, fdone, dist, ss,
                                                         sv, level, group, n_groups, s_hub, &s_nhub, s_acc);
    if (__syncthreads_or(found ? 1 : 0) && threadIdx.x == 0) atomicOr(&flags[level], 1);
}

// A push level's commit (a pull level commits itself: nothing to do).  ``fvol`` is plan.fvol, here to be written at [level].
__global__ __launch_bounds__(256) void msbfs_commit_kernel(
    const int64_t* __restrict__ rowptr, int64_t n_ids, int64_t n_words, int64_t n_sources, uint64_t* __restrict__ seen,
    uint64_t* __restrict__ frontier, uint64_t* __restrict__ next, uint8_t* __restrict__ dist, int32_t* __restrict__ flags,
    unsigned long long* __restrict__ fvol, int level, int64_t ss, int64_t sv, uint32_t* __restrict__ fcur,
    uint8_t* __restrict__ fdone, int64_t rs, MsbfsPlan plan)
{
    if (flags[level - 1] == 0) return;
    if (plan.mode(level).pull) return;
    // One lane per node, a wave per 64 consecutive nodes: the ballot of "some word of my node is new"
    // IS the two 32-bit words of the frontier-node bitmap for those nodes -- plain stores, every word of
    // fcur rewritten each level (nobody reads it while this kernel runs: expand of this level is done).
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t fwords = (n_ids + 31) / 32;
    bool any = false;
    unsigned long long vol = 0;
    for (int64_t base = wave * 64; base < n_ids; base += n_waves * 64) {
        const int64_t v = base + lane;
        int n_new = 0;
        bool done = v < n_ids;
        if (v < n_ids && rs == 4 && !dist) {
            // a padded row is one 32-byte sector: the three arrays are read and written with 16-byte accesses (one 8-byte
            // word per lane and array left the loads a quarter-filled: 50 us per level for 130 MB)
            MsbfsRow<4> nx, sn, nw;
            nx.load(next, v, 4, 0);
            sn.load(seen, v, 4, 0);
            uint64_t any_nx = 0, any_nw = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                nw.w[w] = w < n_words ? (nx.w[w] & ~sn.w[w]) : 0;
                any_nx |= nx.w[w];
                any_nw |= nw.w[w];
                sn.w[w] |= nw.w[w];
                if (w < n_words) {
                    done = done && (sn.w[w] == msbfs_valid(n_sources, w));
                    if (nw.w[w]) ++n_new;
                }
            }
            if (any_nx) MsbfsRow<4>{}.store(next, v, 4, 0);
            nw.store(frontier, v, 4, 0);
            if (any_nw) sn.store(seen, v, 4, 0);
        } else if (v < n_ids) {
            for (int64_t w = 0; w < n_words; ++w) {
                const int64_t i = v * rs + w;
                const uint64_t nx = next[i];
                const uint64_t sn = seen[i];
                const uint64_t nw = nx & ~sn;
                done = done && ((sn | nw) == msbfs_valid(n_sources, w));
                if (nx) next[i] = 0;
                frontier[i] = nw;
                if (nw) {
                    ++n_new;
                    seen[i] = sn | nw;
                    if (dist) msbfs_each_source(nw, w, n_sources, [&](int64_t s) { dist[s * ss + v * sv] = (uint8_t)level; });
                }
            }
        }
        if (n_new) {
            any = true;
            vol += (unsigned long long)n_new * (unsigned long long)(rowptr[v + 1] - rowptr[v]);
        }
        const unsigned long long mask = __ballot(n_new != 0);
        if (v < n_ids) fdone[v] = done ? 1 : 0;                 // (64 consecutive bytes per wavefront)
        if (lane == 0) {                                        // (this wavefront owns the two words: plain read-modify-write)
            uint32_t* __restrict__ fany = fcur + fwords;
            fcur[base >> 5] = (uint32_t)mask;
            if ((uint32_t)mask) fany[base >> 5] |= (uint32_t)mask;
            if ((base >> 5) + 1 < fwords) {
                fcur[(base >> 5) + 1] = (uint32_t)(mask >> 32);
                if ((uint32_t)(mask >> 32)) fany[(base >> 5) + 1] |= (uint32_t)(mask >> 32);
            }
        }
    }
    // one pair of atomics per workgroup: every wave adding to the same two words serialises at the
    // memory side (16k waves -> ~150 us of a 200 us launch)
    __shared__ unsigned long long s_vol[4];
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor((int)(uint32_t)vol, off, 64);
        const uint32_t hi = __shfl_xor((int)(uint32_t)(vol >> 32), off, 64);
        vol += ((unsigned long long)hi << 32) | lo;
    }
    const bool wave_any = __any(any);
    if (lane == 0) s_vol[threadIdx.x >> 6] = wave_any ? (vol | (1ull << 63)) : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0, flag = 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { t += s_vol[k] & ~(1ull << 63); flag |= s_vol[k] >> 63; }
        if (flag) { atomicOr(&flags[level], 1); atomicAdd(&fvol[level], t); }
    }
}

// status[0] = the last level that found anything, [1] = 1 if the LAST enqueued level still found something (too few levels
// enqueued), [2] = the first level that pulled among the levels that ran (0: none did) -- what a caller that repeats the
// search hands back as ``push_levels`` (+ a margin), [3] = 0.
// ``closed`` = the closing form's closed[0] (0: the full form, or the search did not close): [0] is then the closing level
// and [1] = 0 -- [1] = 1 says the enqueued levels ran out before the search closed and before the frontier died.
__device__ static inline void msbfs_write_status(const int32_t* __restrict__ flags, MsbfsPlan plan, int last_level, int closed,
                                                 int32_t* __restrict__ status)
{
    int last = closed ? closed - 1 : 0;
    if (!closed) for (int l = 1; l <= last_level; ++l) if (flags[l]) last = l;
    status[0] = last;
    status[1] = !closed && flags[last_level] != 0;
    int first_pull = 0;
    for (int l = 2; l <= (closed ? last : last + 1) && l <= last_level && first_pull == 0; ++l)
        if (plan.mode(l).pull) first_pull = l;
    status[2] = first_pull;
    status[3] = 0;
}

__global__ void msbfs_status_kernel(const int32_t* __restrict__ flags, int max_hops, int32_t* __restrict__ status, MsbfsPlan plan)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) msbfs_write_status(flags, plan, max_hops, 0, status);
}

__global__ void msbfs_closing_status_kernel(const int32_t* __restrict__ flags, MsbfsPlan plan, int max_hops,
                                            const uint32_t* __restrict__ closed, int32_t* __restrict__ status)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) msbfs_write_status(flags, plan, max_hops, (int)closed[0], status);
}

// The last level's set reduction, the status, and the finalisation.  The reference's matrix holds 0 for unreachable pairs, and
// its row-min runs over those zeros: a source that never reaches SOME member of a set gives 0 for the whole set
// (SubGNN.py:772).  So: AND the members' seen words, zero the sources missing from it.
__global__ __launch_bounds__(256) void msbfs_set_finalize_kernel(
    MsbfsBufs B, int64_t n_words, int64_t n_sources, int64_t rs, MsbfsSets sets, const int32_t* __restrict__ flags,
    int last_level, int32_t* __restrict__ status, MsbfsPlan plan, const uint8_t* __restrict__ fdone)
{
    if (status && blockIdx.x == 0 && threadIdx.x == 0) msbfs_write_status(flags, plan, last_level, 0, status);
    const int64_t total = sets.n_sets * n_words;
    const bool reduce_last = flags[last_level] != 0;         // the last enqueued level found something: its reduction is still due
    const MsbfsMode m = plan.mode(last_level);
    const MsbfsNew nb = msbfs_new_bits(B, m.pull, m.pulls_before);
    const uint64_t* newest = B.b[plan.versions_written(flags, last_level) % 3];
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        if (reduce_last) msbfs_set_reduce_item(nb, n_words, n_sources, sets, last_level, rs, t);
        const int64_t r = t / n_words, w = t % n_words;
        uint64_t all = ~0ull;
        // a member every source has reached (its "complete" byte: set by the commit or the pull level that saw it) restricts
        // nothing; any other member's row is exact in the version written last (complete rows are the only ones that go stale)
        for (int64_t i = sets.set_ptr[r]; i < sets.set_ptr[r + 1]; ++i) {
            const int64_t v = sets.set_nodes[i];
            if (!fdone[v]) all &= newest[v * rs + w];
        }
        msbfs_each_source(~all, w, n_sources, [&](int64_t s) { sets.out[r * n_sources + s] = 0.f; });
    }
}

// ---- the closing form of the set search ------------------------------------------------------------------------------------
// What is read from a set search is, per (set, source), the level at which the first member was reached -- final long before
// the last node of the graph has been.  On a symmetric CSR "source s never reaches member v" is a property of the graph (they
// lie in different connected components: sgnn_graph_component_labels), so the pairs that will ever hold a level are known
// before the first level runs: per (set, word) the WANTED sources are those whose label is the common label of the set's
// members (members of more than one component, or none: nothing is wanted, the row stays 0).  The search is CLOSED once every
// wanted pair is recorded, and nothing after that can change the result.  Protocol (msbfs_run with ``labels``):
//   * the set reduction is a launch of its own BEHIND its level (not the next launch's prologue: closure would be noticed a
//     level late): it records only wanted bits and says whether any item is still open.  Its last workgroup (a ticket) closes the search when
//     no item was open: closed[0] = level + 1 and flags[level] = 0 -- every later launch of the search, commits and push levels
//     included, then returns at the test of flags[level - 1] that ends a search whose frontier died (one exception: a search
//     closed by the SEEDS' reduction -- nothing wanted, or every wanted source a member -- still runs level 1's expand launch,
//     which does not test flags[0]; its commit returns and nothing reads what it pushed).
//   * a level is the level launch (without its prologue), its commit launch if it lies at or below push_levels, and the
//     reduction.
//   * no finalisation over the seen rows (stale after a closure): unwanted pairs were never written.
struct MsbfsClosing {
    const int32_t* labels;       // component label per node id
    const int32_t* sources;
    uint64_t* wanted;            // per (set, word)
    uint32_t* open;              // per level: some item still misses a wanted bit after the level's reduction
    uint32_t* ticket;            // per level: workgroups of the reduction that are through
    uint32_t* closed;            // [0] = closing level + 1 (0: open)
};

__global__ __launch_bounds__(256) void msbfs_closing_reduce_kernel(
    MsbfsBufs B, int64_t n_words, int64_t n_sources, int64_t rs, MsbfsSets sets, MsbfsClosing c, int32_t* __restrict__ flags,
    MsbfsPlan plan, int level)
{
    if (level > 0 && flags[level - 1] == 0) return;          // the level did not run (frontier dead, or closed)
    __shared__ int32_t s_lab[MSBFS_CLOSING_LDS_SOURCES];
    const bool lds = n_sources <= MSBFS_CLOSING_LDS_SOURCES;
    const MsbfsMode m = plan.mode(level);                    // (level 0, the seeds: as a push level)
    const MsbfsNew nb = msbfs_new_bits(B, m.pull, m.pulls_before);
    if (level == 0 && lds) {
        for (int64_t i = threadIdx.x; i < n_sources; i += blockDim.x) s_lab[i] = c.labels[c.sources[i]];
        __syncthreads();
    }
    bool open = false;
    const int64_t total = sets.n_sets * n_words;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        uint64_t want = 0;
        if (level == 0) {
            const int64_t r = t / n_words, w = t % n_words;
            const int64_t beg = sets.set_ptr[r], end = sets.set_ptr[r + 1];
            bool one = end > beg;
            int32_t common = -1;
            for (int64_t i = beg; i < end; ++i) {
                const int32_t lab = c.labels[sets.set_nodes[i]];
                if (i == beg) common = lab; else if (lab != common) one = false;
            }
            if (one)
                for (int b = 0; b < 64 && w * 64 + b < n_sources; ++b) {
                    const int64_t s = w * 64 + b;
                    if ((lds ? s_lab[s] : c.labels[c.sources[s]]) == common) want |= 1ull << b;
                }
            c.wanted[t] = want;
        } else
            want = c.wanted[t];
        if (msbfs_set_reduce_item(nb, n_words, n_sources, sets, level, rs, t, want)) open = true;
    }
    if (__syncthreads_or(open ? 1 : 0) && threadIdx.x == 0) atomicOr(&c.open[level], 1u);
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&c.ticket[level], 1u) == gridDim.x - 1) {      // the last workgroup: every other one's verdict is in
            __threadfence();
            if (__hip_atomic_load(&c.open[level], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                c.closed[0] = (uint32_t)level + 1;
                flags[level] = 0;
            }
        }
    }
}

// labels: the closing form (sets only).  push_levels: levels that may still push (a commit launch is enqueued for each); beyond
// them the search pulls.  < 0, or alpha = 0 (never pull: the caller's choice): every level
static int msbfs_run(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                     const int32_t* sources, int64_t n_sources, int max_hops, int node_major, uint8_t* dist,
                     const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, float* set_out,
                     void* workspace, hipStream_t st, int pull_alpha, int32_t* status = nullptr, int push_levels = -1,
                     const int32_t* labels = nullptr)
{
    if (push_levels < 0 || pull_alpha == 0 || push_levels > max_hops) push_levels = max_hops;
    if (push_levels < 1) push_levels = 1;                    // (level 1 always pushes: the seeds' lists)
    const int alpha = pull_alpha < 0 ? MSBFS_DEFAULT_ALPHA : pull_alpha;
    const int64_t n_ids = max_id + 1;
    const int64_t n_words = (n_sources + 63) / 64;
    const int64_t ss = node_major ? 1 : n_ids, sv = node_major ? n_sources : 1;
    const int64_t rs = msbfs_row_stride(n_words);
    const bool closing = labels != nullptr;
    const MsbfsLayout L = msbfs_layout(max_id, n_sources, max_hops, set_out ? n_sets : -1, closing);
    char* const ws = (char*)workspace;                       // (8-byte aligned: msbfs_check_args)
    uint64_t* seen = (uint64_t*)(ws + L.seen);
    uint64_t* frontier = (uint64_t*)(ws + L.frontier);
    uint64_t* next = (uint64_t*)(ws + L.next);
    unsigned long long* fvol = (unsigned long long*)(ws + L.fvol);
    int32_t* flags = (int32_t*)(ws + L.flags);
    uint32_t* fbits = (uint32_t*)(ws + L.fbits);
    uint8_t* fdone = (uint8_t*)(ws + L.fdone);
    const int64_t fwords = (n_ids + 31) / 32;
    const MsbfsBufs bufs = {{seen, next, frontier}};
    const MsbfsPlan plan = {fvol, alpha > 0 ? (unsigned long long)((nnz * n_words) / alpha) : ~0ull,
                            push_levels};
    const int64_t items = set_out ? n_sets * n_words : 0;
    const MsbfsSets sets = {set_ptr, set_nodes, set_out ? n_sets : 0, (uint64_t*)(ws + L.set_seen), set_out};
    MsbfsSets none = sets;
    none.n_sets = 0;
    MsbfsClosing cl = {};
    if (closing) {
        cl.labels = labels; cl.sources = sources;
        cl.open = (uint32_t*)(ws + L.closing);
        cl.ticket = cl.open + max_hops + 2;
        cl.closed = cl.ticket + max_hops + 2;
        cl.wanted = (uint64_t*)(ws + L.wanted);
    }
    const int big = sgnn_grid_for(n_ids * ((dist && n_sources > rs) ? n_sources : rs), 256);
    const int g_sets = set_out ? sgnn_grid_for(n_sets * n_words, 256) : 0;
    const int g_expand = sgnn_grid_for(n_ids * 16, 256);
    const int g_commit = sgnn_grid_for(n_ids, 256, 256 * 4);
    auto launch_level = [&](int level) {
        // (the closing form: no prologue reduction -- every level's own launch follows it)
        hipLaunchKernelGGL(msbfs_level_kernel, dim3(g_expand), dim3(256), 0, st, rowptr, col, n_ids, n_words, n_sources, bufs, flags,
                           plan, level, fbits, fbits + fwords, fdone, rs, closing ? none : sets, dist, ss, sv);
        SGNN_CHECK_LAUNCH();
        return SGNN_OK;
    };
    auto launch_commit = [&](int level) {
        hipLaunchKernelGGL(msbfs_commit_kernel, dim3(g_commit), dim3(256), 0, st, rowptr, n_ids, n_words, n_sources, seen, frontier,
                           next, dist, flags, fvol, level, ss, sv, fbits, fdone, rs, plan);
        SGNN_CHECK_LAUNCH();
        return SGNN_OK;
    };
    // (the closing state lies behind set_seen and is zeroed with it)
    hipLaunchKernelGGL(msbfs_init_kernel, dim3(big), dim3(256), 0, st, sources, n_sources, n_words, n_ids, seen,
                       frontier, next, dist, flags, fvol, fbits, max_hops, rs, sets.set_seen,
                       items + (closing ? msbfs_closing_state_words(max_hops) : 0), set_out, set_out ? n_sets * n_sources : 0);
    SGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(msbfs_seed_kernel, dim3((int)((n_sources + 255) / 256)), dim3(256), 0, st, sources, n_sources,
                       n_words, n_ids, seen, frontier, dist, ss, sv, fbits, rs);
    SGNN_CHECK_LAUNCH();
    for (int level = closing ? 0 : 1; level <= max_hops; ++level) {
        if (level >= 1) {
            if (int rc = launch_level(level)) return rc;
            if (level <= push_levels)                        // (a level beyond them pulls: it commits itself)
                if (int rc = launch_commit(level)) return rc;
        }
        if (closing) {                                       // the level's reduction (level 0: the seeds')
            hipLaunchKernelGGL(msbfs_closing_reduce_kernel, dim3(g_sets), dim3(256), 0, st, bufs, n_words, n_sources, rs, sets, cl,
                               flags, plan, level);
            SGNN_CHECK_LAUNCH();
        }
    }
    if (closing) {
        if (!status) return SGNN_OK;
        hipLaunchKernelGGL(msbfs_closing_status_kernel, dim3(1), dim3(64), 0, st, flags, plan, max_hops, cl.closed, status);
    } else if (set_out) {
        hipLaunchKernelGGL(msbfs_set_finalize_kernel, dim3(g_sets), dim3(256), 0, st, bufs, n_words, n_sources, rs, sets, flags,
                           max_hops, status, plan, fdone);
    } else {
        if (!status) return SGNN_OK;
        hipLaunchKernelGGL(msbfs_status_kernel, dim3(1), dim3(64), 0, st, flags, max_hops, status, plan);
    }
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

// the argument check of the three entry points; ``pointers``: all of them are there.  The workspace holds 64-bit words at
// offsets that are multiples of 8 (MsbfsLayout), so it has to start at one
static int msbfs_check_args(bool pointers, const void* workspace, int64_t nnz, int64_t n_sources, int64_t n_sets, int max_hops,
                            int64_t workspace_bytes, int64_t needed)
{
    if (!pointers || !workspace || ((uintptr_t)workspace & 7) || n_sources < 0 || n_sets < 0 || max_hops < 1 || max_hops > 254)
        return SGNN_ERR_BAD_ARG;
    if (nnz >= (1ll << 31)) return SGNN_ERR_NNZ_TOO_LARGE;
    return workspace_bytes < needed ? SGNN_ERR_BAD_ARG : SGNN_OK;
}

extern "C" int64_t sgnn_bfs_hops_workspace_bytes(int64_t max_id, int64_t n_sources, int max_hops) {
    return msbfs_layout(max_id, n_sources, max_hops, -1, false).total;
}

extern "C" int sgnn_bfs_hops(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                             const int32_t* sources, int64_t n_sources, int max_hops, int node_major, int pull_alpha,
                             uint8_t* dist, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (int rc = msbfs_check_args(rowptr && col && sources && dist, workspace, nnz, n_sources, 0, max_hops, workspace_bytes,
                                  sgnn_bfs_hops_workspace_bytes(max_id, n_sources, max_hops)))
        return rc;
    if (n_sources == 0) return SGNN_OK;
    return msbfs_run(rowptr, col, nnz, max_id, sources, n_sources, max_hops, node_major, dist, nullptr, nullptr, 0,
                     nullptr, workspace, (hipStream_t)stream, pull_alpha);
}

extern "C" int64_t sgnn_bfs_min_hops_workspace_bytes(int64_t max_id, int64_t n_sources, int max_hops, int64_t n_sets) {
    return msbfs_layout(max_id, n_sources, max_hops, n_sets, false).total;
}

extern "C" int sgnn_bfs_min_hops_to_sets(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                                         const int32_t* sources, int64_t n_sources, int max_hops, int pull_alpha, int push_levels,
                                         const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                         float* out, int32_t* out_status, void* workspace, int64_t workspace_bytes,
                                         void* stream)
{
    if (int rc = msbfs_check_args(rowptr && col && sources && set_ptr && set_nodes && out, workspace, nnz, n_sources, n_sets,
                                  max_hops, workspace_bytes, sgnn_bfs_min_hops_workspace_bytes(max_id, n_sources, max_hops, n_sets)))
        return rc;
    if (n_sources == 0 || n_sets == 0) return SGNN_OK;
    return msbfs_run(rowptr, col, nnz, max_id, sources, n_sources, max_hops, 0, nullptr, set_ptr, set_nodes, n_sets, out,
                     workspace, (hipStream_t)stream, pull_alpha, out_status, push_levels);
}

extern "C" int64_t sgnn_bfs_min_hops_closing_workspace_bytes(int64_t max_id, int64_t n_sources, int max_hops, int64_t n_sets) {
    return msbfs_layout(max_id, n_sources, max_hops, n_sets, true).total;
}

extern "C" int sgnn_bfs_min_hops_to_sets_closing(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                                                 const int32_t* sources, int64_t n_sources, int max_hops, int pull_alpha,
                                                 int push_levels, const int32_t* labels, const int64_t* set_ptr,
                                                 const int32_t* set_nodes, int64_t n_sets, float* out, int32_t* out_status,
                                                 void* workspace, int64_t workspace_bytes, void* stream)
{
    if (int rc = msbfs_check_args(rowptr && col && sources && labels && set_ptr && set_nodes && out, workspace, nnz, n_sources,
                                  n_sets, max_hops, workspace_bytes,
                                  sgnn_bfs_min_hops_closing_workspace_bytes(max_id, n_sources, max_hops, n_sets)))
        return rc;
    if (n_sources == 0 || n_sets == 0) return SGNN_OK;
    return msbfs_run(rowptr, col, nnz, max_id, sources, n_sources, max_hops, 0, nullptr, set_ptr, set_nodes, n_sets, out,
                     workspace, (hipStream_t)stream, pull_alpha, out_status, push_levels, labels);
}

// ---- connected components of the whole graph: labels[v] = the smallest id of v's component (ids without edges label
// themselves).  Hook the larger root under the smaller one (atomicMin: a parent is never above its child, so a tree's root
// is its smallest id), flatten, and repeat until no edge joins two trees -- once per graph, the host reads one word a round.
__device__ __forceinline__ int32_t cc_graph_root(const int32_t* lab, int32_t x)
{
    for (int32_t p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); p != x;
         p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        x = p;
    return x;
}

__global__ void cc_graph_init_kernel(int32_t* __restrict__ lab, int64_t n_ids)
{
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n_ids; v += (int64_t)gridDim.x * blockDim.x) lab[v] = (int32_t)v;
}

__global__ __launch_bounds__(256) void cc_graph_hook_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            int64_t n_ids, int32_t* lab, int32_t* __restrict__ changed)
{
    const int sub = threadIdx.x & 15;
    const int64_t group = blockIdx.x * (int64_t)(blockDim.x >> 4) + (threadIdx.x >> 4);
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x >> 4);
    bool any = false;
    for (int64_t v = group; v < n_ids; v += n_groups) {
        const int64_t r0 = rowptr[v], r1 = rowptr[v + 1];
        for (int64_t e = r0 + sub; e < r1; e += 16) {
            const int32_t u = col[e];
            if (u < 0 || u >= n_ids || u == v) continue;
            const int32_t a = cc_graph_root(lab, (int32_t)v), b = cc_graph_root(lab, u);
            if (a != b) {
                atomicMin(&lab[a > b ? a : b], a > b ? b : a);
                any = true;
            }
        }
    }
    if (any) *changed = 1;
}

__global__ void cc_graph_flatten_kernel(int32_t* lab, int64_t n_ids)
{
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n_ids; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = cc_graph_root(lab, (int32_t)v);
        if (r != (int32_t)v) __hip_atomic_store(&lab[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

extern "C" int64_t sgnn_graph_component_labels_workspace_bytes(int64_t max_id) { (void)max_id; return 16; }

extern "C" int sgnn_graph_component_labels(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                                           int32_t* labels, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (!rowptr || (!col && nnz > 0) || !labels || !workspace || max_id < 0 || nnz < 0 ||
        workspace_bytes < sgnn_graph_component_labels_workspace_bytes(max_id))
        return SGNN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_ids = max_id + 1;
    int32_t* changed = (int32_t*)workspace;
    hipLaunchKernelGGL(cc_graph_init_kernel, dim3(sgnn_grid_for(n_ids, 256)), dim3(256), 0, st, labels, n_ids);
    SGNN_CHECK_LAUNCH();
    for (int64_t round = 0; round <= n_ids; ++round) {       // (a round that joins nothing ends it; n_ids rounds always suffice)
        int32_t host = 0;
        if (hipMemsetAsync(changed, 0, 4, st) != hipSuccess) return SGNN_ERR_LAUNCH;
        hipLaunchKernelGGL(cc_graph_hook_kernel, dim3(sgnn_grid_for(n_ids * 16, 256)), dim3(256), 0, st, rowptr, col, n_ids, labels, changed);
        SGNN_CHECK_LAUNCH();
        hipLaunchKernelGGL(cc_graph_flatten_kernel, dim3(sgnn_grid_for(n_ids, 256)), dim3(256), 0, st, labels, n_ids);
        SGNN_CHECK_LAUNCH();
        if (hipMemcpyAsync(&host, changed, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return SGNN_ERR_LAUNCH;
        if (!host) break;
    }
    return SGNN_OK;
}

__global__ void min_hops_to_sets_kernel(const uint8_t* __restrict__ dist, int64_t n_sources, int64_t n_ids,
                                        const int64_t* __restrict__ set_ptr, const int32_t* __restrict__ set_nodes,
                                        int64_t n_sets, float* __restrict__ out, int64_t ss, int64_t sv)
{
    const int64_t total = n_sets * n_sources;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / n_sources, a = t % n_sources;
        const int64_t beg = set_ptr[r];
        const int n = (int)(set_ptr[r + 1] - beg);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            int d = dist[a * ss + (int64_t)set_nodes[beg + i] * sv];
            if (d == 255) d = 0;                               // unreachable pairs hold 0 in the matrix
            m = (i == 0 || d < m) ? d : m;
        }
        out[t] = (float)m;
    }
}

extern "C" int sgnn_min_hops_to_sets(const uint8_t* dist, int64_t n_sources, int64_t max_id, int node_major,
                                     const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                     float* out, void* stream)
{
    if (!dist || !set_ptr || !set_nodes || !out || n_sources < 0 || n_sets < 0) return SGNN_ERR_BAD_ARG;
    if (n_sets * n_sources == 0) return SGNN_OK;
    hipLaunchKernelGGL(min_hops_to_sets_kernel, dim3(sgnn_grid_for(n_sets * n_sources, 256)), dim3(256), 0,
                       (hipStream_t)stream, dist, n_sources, max_id + 1, set_ptr, set_nodes, n_sets, out,
                       node_major ? 1 : max_id + 1, node_major ? n_sources : 1);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

SGNN_DEFINE_WARM(similarity)

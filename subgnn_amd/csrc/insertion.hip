// Insertion sets (subgnn_hip.h, sgnn_insertion_count / sgnn_insertion_write): every add-one-candidate variant s U {v} of every
// ragged set, v running over the set's candidate row (or over ONE row shared by all sets) without the set's members.  The
// mirror of occlusion.hip.
//
// One workgroup per set, in the three tiers of id_table.h / occlusion.hip by the set's length: up to SGNN_SET_WAVE_MAX a
// workgroup of ONE wavefront with the set in LDS, up to SGNN_INS_LDS_MAX four wavefronts with the set in LDS, beyond it four
// wavefronts that read the set from global memory.  All three are one body.
//
// Per set:  (1) the set is copied to LDS and (write) the wavefronts add their parts of its mix sum, once;  (2) the candidate
// row is walked in chunks of one candidate per thread: a binary search gives the candidate's rank p in the set (the number of
// smaller entries) and whether it is a member; a ballot per wavefront and the wavefronts' totals in LDS give every kept
// candidate its place among the set's variants;  (3) count: the places add up to out_variants[s];  write: the chunk's kept
// (v, p) pairs go to LDS, the variant headers (offset, parent, candidate, key from the parent's sum plus sgnn_mix64(v)) are
// written one per thread, then the entries: every variant has n + 1 of them, so from LDS the chunk's kept x (n + 1) block is
// one coalesced sweep (entry j of a variant is entry j of the set before p, v at p, entry j - 1 behind); a streamed set is
// written one wavefront per variant, front to back.  No float work, no atomics.
#include "id_table.h"

#define SGNN_INS_LDS_MAX 1024          // entries of a set that is expanded from LDS (the occlusion tiers)

struct InsArgs {
    const int64_t* set_ptr; const int32_t* set_nodes; int64_t n_sets;
    const int64_t* cand_ptr; const int32_t* cand_ids; int shared;
    int64_t lo, hi;                                                                   // the lengths this launch takes
    int64_t* out_variants;                                                            // count
    const int64_t* var_ptr; const int64_t* entry_ptr; int64_t n_variants;             // write
    int64_t* out_ptr; int32_t* out_nodes; int32_t* out_parent; int32_t* out_cand; uint64_t* out_keys;
};

template <int THREADS, int CAP, bool WRITE>
__global__ __launch_bounds__(THREADS) void ins_kernel(const InsArgs a)
{
    constexpr bool LDS = CAP > 0;
    constexpr int N = LDS ? CAP : 1, W = THREADS / 64, NK = WRITE ? THREADS : 1;
    __shared__ int32_t s_nd[N];
    __shared__ int32_t s_v[NK];                                      // the chunk's kept candidates, in order
    __shared__ int32_t s_p[NK];                                      // ... and their ranks in the set
    __shared__ int s_cnt[2][W];                                      // kept candidates per wavefront, by the chunk's parity
    __shared__ unsigned long long s_part[W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1;

    for (int64_t s = blockIdx.x; s < a.n_sets; s += gridDim.x) {
        const int64_t beg = a.set_ptr[s], n64 = a.set_ptr[s + 1] - beg;
        if (n64 < a.lo || n64 > a.hi) continue;                      // the same for the whole workgroup
        const int n = (int)n64;
        const int32_t* __restrict__ nodes = a.set_nodes + beg;
        const int32_t* nd = LDS ? s_nd : nodes;
        const int64_t row = a.shared ? 0 : s;
        const int64_t cbeg = a.cand_ptr[row], m = a.cand_ptr[row + 1] - cbeg;
        const int32_t* __restrict__ cand = a.cand_ids + cbeg;

        __syncthreads();                                             // the set before this one is done with the LDS
        if (LDS) for (int i = tid; i < n; i += THREADS) s_nd[i] = nodes[i];
        if (WRITE) {
            uint64_t acc = 0;
            for (int i = tid; i < n; i += THREADS) acc += sgnn_mix64((uint64_t)(uint32_t)nodes[i]);
            acc = sgnn_wave_sum_u64(acc);
            if (lane == 0) s_part[wave] = (unsigned long long)acc;
        }
        __syncthreads();
        uint64_t tot = 0;
        if (WRITE) for (int w = 0; w < W; ++w) tot += s_part[w];
        const int64_t v0 = WRITE ? a.var_ptr[s] : 0, e0 = WRITE ? a.entry_ptr[s] : 0;
        const int64_t len = (int64_t)n + 1;

        int64_t run = 0;                                             // variants of this set before the chunk
        int par = 0;
        for (int64_t base = 0; base < m; base += THREADS, par ^= 1) {
            const int64_t i = base + tid;
            int32_t v = 0;
            int p = 0;
            bool keep = false;
            if (i < m) {
                v = cand[i];
                int hi = n;                                          // lower bound: the number of entries < v
                while (p < hi) {
                    const int mid = (int)(((unsigned)p + (unsigned)hi) >> 1);
                    if (nd[mid] < v) p = mid + 1; else hi = mid;
                }
                keep = !(p < n && nd[p] == v);
            }
            const uint64_t bal = __ballot(keep);
            if (lane == 0) s_cnt[par][wave] = __popcll(bal);
            __syncthreads();
            int before = 0, kept = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const int c = s_cnt[par][w];
                if (w < wave) before += c;
                kept += c;
            }
            if (!WRITE) { run += kept; continue; }                   // (the other parity's counts are written next: no barrier)

            if (keep) {
                const int k = before + __popcll(bal & below);
                s_v[k] = v; s_p[k] = p;
            }
            __syncthreads();
            if (tid < kept) {
                const int64_t vi = v0 + run + tid, o = e0 + (run + tid) * len;
                const int32_t x = s_v[tid];
                a.out_ptr[vi] = o;
                if (vi == a.n_variants - 1) a.out_ptr[vi + 1] = o + len;
                a.out_parent[vi] = (int32_t)s;
                a.out_cand[vi] = x;
                a.out_keys[vi] = sgnn_set_key_finish(tot + sgnn_mix64((uint64_t)(uint32_t)x), (uint64_t)len);
            }
            int32_t* __restrict__ dst = a.out_nodes + e0 + run * len;
            if (LDS) {
                const uint32_t l = (uint32_t)len, total = (uint32_t)kept * l;      // <= 256 * 1025
                for (uint32_t idx = tid; idx < total; idx += THREADS) {
                    const uint32_t k = idx / l, j = idx - k * l, q = (uint32_t)s_p[k];
                    dst[idx] = j == q ? s_v[k] : s_nd[j - (j > q)];
                }
            } else {
                for (int k = wave; k < kept; k += W) {
                    int32_t* __restrict__ out = dst + (int64_t)k * len;
                    const int64_t q = s_p[k];
                    const int32_t x = s_v[k];
                    for (int64_t j = lane; j < len; j += 64) out[j] = j == q ? x : nodes[j - (j > q)];
                }
            }
            run += kept;
            __syncthreads();                                         // the chunk's pairs are read
        }
        if (!WRITE && tid == 0) a.out_variants[s] = run;
    }
}

template <int THREADS, int CAP, bool WRITE>
static void ins_launch_tier(InsArgs a, int64_t lo, int64_t hi, hipStream_t st)
{
    a.lo = lo; a.hi = hi;
    hipLaunchKernelGGL((ins_kernel<THREADS, CAP, WRITE>), dim3(sgnn_grid_for(a.n_sets, 1, 256 * (THREADS == 64 ? 32 : 16))),
                       dim3(THREADS), 0, st, a);
}

template <bool WRITE> static void ins_launch(const InsArgs& a, int64_t max_len, hipStream_t st)
{
    ins_launch_tier<64, SGNN_SET_WAVE_MAX, WRITE>(a, 0, SGNN_SET_WAVE_MAX, st);
    if (max_len == 0 || max_len > SGNN_SET_WAVE_MAX)
        ins_launch_tier<256, SGNN_INS_LDS_MAX, WRITE>(a, SGNN_SET_WAVE_MAX + 1, SGNN_INS_LDS_MAX, st);
    if (max_len == 0 || max_len > SGNN_INS_LDS_MAX)
        ins_launch_tier<256, 0, WRITE>(a, SGNN_INS_LDS_MAX + 1, 0x7fffffff, st);
}

static bool ins_refused(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len,
                        const int64_t* cand_ptr, const int32_t* cand_ids, int shared)
{
    if (n_sets < 0 || n_sets > 0x7fffffff || max_set_len < 0) return true;
    if (shared != 0 && shared != 1) return true;
    if (n_sets > 0 && (!set_ptr || !set_nodes || !cand_ptr || !cand_ids)) return true;
    return false;
}

extern "C" int sgnn_insertion_count(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len,
                                    const int64_t* cand_ptr, const int32_t* cand_ids, int shared, int64_t* out_variants,
                                    void* stream)
{
    if (ins_refused(set_ptr, set_nodes, n_sets, max_set_len, cand_ptr, cand_ids, shared)) return SGNN_ERR_BAD_ARG;
    if (n_sets > 0 && !out_variants) return SGNN_ERR_BAD_ARG;
    if (n_sets == 0) return SGNN_OK;
    InsArgs a = {};
    a.set_ptr = set_ptr; a.set_nodes = set_nodes; a.n_sets = n_sets;
    a.cand_ptr = cand_ptr; a.cand_ids = cand_ids; a.shared = shared;
    a.out_variants = out_variants;
    ins_launch<false>(a, max_set_len, (hipStream_t)stream);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_insertion_write(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len,
                                    const int64_t* cand_ptr, const int32_t* cand_ids, int shared, const int64_t* var_ptr,
                                    const int64_t* entry_ptr, int64_t n_variants, int64_t* out_ptr, int32_t* out_nodes,
                                    int32_t* out_parent, int32_t* out_cand, uint64_t* out_keys, void* stream)
{
    if (ins_refused(set_ptr, set_nodes, n_sets, max_set_len, cand_ptr, cand_ids, shared) || n_variants < 0 || n_variants > 0x7fffffff)
        return SGNN_ERR_BAD_ARG;
    if (n_variants > 0 && (n_sets == 0 || !var_ptr || !entry_ptr || !out_ptr || !out_nodes || !out_parent || !out_cand || !out_keys))
        return SGNN_ERR_BAD_ARG;
    if (n_sets == 0 || n_variants == 0) return SGNN_OK;
    InsArgs a = {};
    a.set_ptr = set_ptr; a.set_nodes = set_nodes; a.n_sets = n_sets;
    a.cand_ptr = cand_ptr; a.cand_ids = cand_ids; a.shared = shared;
    a.var_ptr = var_ptr; a.entry_ptr = entry_ptr; a.n_variants = n_variants;
    a.out_ptr = out_ptr; a.out_nodes = out_nodes; a.out_parent = out_parent; a.out_cand = out_cand; a.out_keys = out_keys;
    ins_launch<true>(a, max_set_len, (hipStream_t)stream);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

SGNN_DEFINE_WARM(insertion)

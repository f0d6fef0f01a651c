// Occlusion sets (subgnn_hip.h, sgnn_occlusion_count / sgnn_occlusion_write): every leave-one-unit-out variant of every ragged
// set, a unit being an entry (node mode) or a component (component mode, from the labels of sgnn_cc_labels).
//
// One workgroup per set, in three tiers by the set's length (id_table.h): up to SGNN_SET_WAVE_MAX a workgroup of ONE
// wavefront with the set in LDS, up to SGNN_OCC_LDS_MAX four wavefronts with the set in LDS, beyond it four wavefronts that
// stream the set from global memory and keep the unit tables (component mode) in the caller's workspace.  All three are one
// body; the home of the tables is a template argument because it decides how they may be read (id_table.h: idt_ld, idt_sync).
//
// Per set:  (1) the set is copied to LDS, once;  (2) component mode: wavefront 0 ranks the roots (entries that label
// themselves) by position with ballots -- a root's rank is the unit's rank -- then every entry takes its root's rank and adds
// itself to its unit's size and, for the keys, sgnn_mix64 of itself to its unit's sum;  (3) the wavefronts add their parts of
// the parent's sum;  (4) count: the lengths n - size[u];  write: the variant headers (offset, parent, unit, key from the
// parent's sum minus the unit's), then the entries.  Node mode from LDS: the variants of a set are n rows of n - 1 entries
// back to back, so the whole block is one coalesced sweep (entry j of variant u is entry j + (j >= u) of the set).  Otherwise
// one wavefront per variant walks the set 64 entries at a time: a ballot of the kept entries gives every kept lane its
// place, so a variant is written front to back in runs of consecutive addresses, with no workgroup barrier in the loop.
#include "id_table.h"

#define SGNN_OCC_LDS_MAX 1024          // entries of a set that is expanded from LDS (4 x 4 KB of tables + 8 KB of sums per workgroup)

struct OccArgs {
    const int64_t* set_ptr; const int32_t* set_nodes; const int32_t* labels; int64_t n_sets;
    int64_t lo, hi;                                                                   // the lengths this launch takes
    int64_t* out_units; int64_t* out_variants; int64_t* out_len;                      // count
    const int64_t* var_ptr; const int64_t* len_scan; int64_t n_variants;              // write
    int64_t* out_ptr; int32_t* out_nodes; int32_t* out_parent; int32_t* out_unit; uint64_t* out_keys;
    unsigned long long* ws_sum; int32_t* ws_rank; int32_t* ws_size;                   // the streamed tier's unit tables
};

template <bool LDS> __device__ __forceinline__ uint64_t occ_ld64(const unsigned long long* p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the label of entry i as the kernel takes it: a position before i that labels itself, else i (a unit of its own)
__device__ __forceinline__ int occ_label(const int32_t* __restrict__ lab, int i) {
    const int l = lab[i];
    return (l >= 0 && l < i && lab[l] == l) ? l : i;
}

template <int THREADS, int CAP, bool COMP, bool WRITE>
__global__ __launch_bounds__(THREADS) void occ_kernel(const OccArgs a)
{
    constexpr bool LDS = CAP > 0;
    constexpr int N = LDS ? CAP : 1, NC = (LDS && COMP) ? CAP : 1, NS = (LDS && COMP && WRITE) ? CAP : 1;
    __shared__ int32_t s_nd[N];
    __shared__ int32_t s_rk[NC];
    __shared__ int32_t s_sz[NC];
    __shared__ unsigned long long s_sm[NS];
    __shared__ unsigned long long s_tot;
    __shared__ int s_units;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1;

    for (int64_t s = blockIdx.x; s < a.n_sets; s += gridDim.x) {
        const int64_t beg = a.set_ptr[s], n64 = a.set_ptr[s + 1] - beg;
        if (n64 < a.lo || n64 > a.hi) continue;                      // the same for the whole workgroup
        const int n = (int)n64;
        const int32_t* __restrict__ nodes = a.set_nodes + beg;
        int32_t* rk = LDS ? s_rk : a.ws_rank + beg;
        int32_t* sz = LDS ? s_sz : a.ws_size + beg;
        unsigned long long* sm = LDS ? s_sm : a.ws_sum + beg;
        const int32_t* nd = LDS ? s_nd : nodes;

        __syncthreads();                                             // the set before this one is done with the LDS
        if (tid == 0) s_tot = 0;
        if (LDS) for (int i = tid; i < n; i += THREADS) s_nd[i] = nodes[i];
        __syncthreads();

        int U = n;
        if (COMP) {
            const int32_t* __restrict__ lab = a.labels + beg;
            if (wave == 0) {
                int run = 0;
                for (int base = 0; base < n; base += 64) {
                    const int i = base + lane;
                    const bool root = i < n && occ_label(lab, i) == i;
                    const uint64_t m = __ballot(root);
                    if (root) {
                        const int r = run + __popcll(m & below);
                        rk[i] = r; sz[r] = 0;
                        if (WRITE) sm[r] = 0;
                    }
                    run += __popcll(m);
                }
                if (lane == 0) s_units = run;
            }
            idt_sync<LDS>();
            U = s_units;
            for (int i = tid; i < n; i += THREADS) {
                const int l = occ_label(lab, i);
                const int r = idt_ld<LDS>(rk + l);                   // a root's entry: nobody writes it in this loop
                if (l != i) rk[i] = r;
                atomicAdd(&sz[r], 1);
                if (WRITE) atomicAdd(&sm[r], (unsigned long long)sgnn_mix64((uint64_t)(uint32_t)nd[i]));
            }
        }
        if (WRITE) {
            uint64_t acc = 0;
            for (int i = tid; i < n; i += THREADS) acc += sgnn_mix64((uint64_t)(uint32_t)nd[i]);
            acc = sgnn_wave_sum_u64(acc);
            if (lane == 0) atomicAdd(&s_tot, (unsigned long long)acc);
        }
        idt_sync<LDS>();

        const bool any = U >= 2;                                     // fewer units: removing one leaves nothing
        if (!WRITE) {
            if (tid == 0) { a.out_units[s] = U; a.out_variants[s] = any ? U : 0; }
            for (int u = tid; u < n; u += THREADS)
                a.out_len[beg + u] = (any && u < U) ? (int64_t)(n - (COMP ? idt_ld<LDS>(sz + u) : 1)) : 0;
            continue;
        }
        if (!any) continue;

        const int64_t v0 = a.var_ptr[s];
        const int64_t* __restrict__ off = a.len_scan + beg;
        const uint64_t tot = s_tot;
        for (int u = tid; u < U; u += THREADS) {
            const int64_t v = v0 + u, o = off[u];
            const int len = n - (COMP ? idt_ld<LDS>(sz + u) : 1);
            const uint64_t gone = COMP ? occ_ld64<LDS>(sm + u) : sgnn_mix64((uint64_t)(uint32_t)nd[u]);
            a.out_ptr[v] = o;
            if (v == a.n_variants - 1) a.out_ptr[v + 1] = o + len;
            a.out_parent[v] = (int32_t)s;
            a.out_unit[v] = u;
            a.out_keys[v] = sgnn_set_key_finish(tot - gone, (uint64_t)len);
        }
        if (!COMP && LDS) {
            const uint32_t m = (uint32_t)n - 1, total = (uint32_t)n * m;
            int32_t* __restrict__ dst = a.out_nodes + off[0];
            for (uint32_t idx = tid; idx < total; idx += THREADS) {
                const uint32_t u = idx / m, j = idx - u * m;
                dst[idx] = nd[j + (j >= u)];
            }
        } else {
            for (int u = wave; u < U; u += THREADS / 64) {
                int32_t* __restrict__ dst = a.out_nodes + off[u];
                int64_t run = 0;
                for (int base = 0; base < n; base += 64) {
                    const int i = base + lane;
                    const bool keep = i < n && (COMP ? idt_ld<LDS>(rk + i) != u : i != u);
                    const uint64_t m = __ballot(keep);
                    if (keep) dst[run + __popcll(m & below)] = nd[i];
                    run += __popcll(m);
                }
            }
        }
    }
}

template <int THREADS, int CAP, bool COMP, bool WRITE>
static void occ_launch_tier(OccArgs a, int64_t lo, int64_t hi, hipStream_t st)
{
    a.lo = lo; a.hi = hi;
    hipLaunchKernelGGL((occ_kernel<THREADS, CAP, COMP, WRITE>), dim3(sgnn_grid_for(a.n_sets, 1, 256 * (THREADS == 64 ? 32 : 16))),
                       dim3(THREADS), 0, st, a);
}

template <bool COMP, bool WRITE> static void occ_launch(const OccArgs& a, int64_t max_len, hipStream_t st)
{
    occ_launch_tier<64, SGNN_SET_WAVE_MAX, COMP, WRITE>(a, 0, SGNN_SET_WAVE_MAX, st);
    if (max_len == 0 || max_len > SGNN_SET_WAVE_MAX)
        occ_launch_tier<256, SGNN_OCC_LDS_MAX, COMP, WRITE>(a, SGNN_SET_WAVE_MAX + 1, SGNN_OCC_LDS_MAX, st);
    if (max_len == 0 || max_len > SGNN_OCC_LDS_MAX)
        occ_launch_tier<256, 0, COMP, WRITE>(a, SGNN_OCC_LDS_MAX + 1, 0x7fffffff, st);
}

extern "C" int64_t sgnn_occlusion_lds_max(void) { return SGNN_OCC_LDS_MAX; }

// per entry of the input: the unit's sum (8 bytes), the entry's unit rank and the unit's size (4 bytes each), each table at
// the set's offset
extern "C" int64_t sgnn_occlusion_workspace_bytes(int64_t total_entries) { return total_entries < 0 ? 0 : 16 * total_entries; }

static bool occ_refused(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len, int mode,
                        const int32_t* labels, int64_t total_entries, void* workspace, int64_t workspace_bytes)
{
    if (n_sets < 0 || n_sets > 0x7fffffff || max_set_len < 0 || total_entries < 0 || workspace_bytes < 0) return true;
    if (mode != SGNN_OCC_NODE && mode != SGNN_OCC_COMPONENT) return true;
    if (n_sets > 0 && (!set_ptr || !set_nodes || (mode == SGNN_OCC_COMPONENT && !labels))) return true;
    const bool streamed = mode == SGNN_OCC_COMPONENT && n_sets > 0 && (max_set_len == 0 || max_set_len > SGNN_OCC_LDS_MAX);
    if (streamed && (!workspace || workspace_bytes < sgnn_occlusion_workspace_bytes(total_entries))) return true;
    return false;
}

static void occ_workspace(OccArgs& a, void* workspace, int64_t total_entries)
{
    a.ws_sum = (unsigned long long*)workspace;
    a.ws_rank = workspace ? (int32_t*)(a.ws_sum + total_entries) : nullptr;
    a.ws_size = workspace ? a.ws_rank + total_entries : nullptr;
}

extern "C" int sgnn_occlusion_count(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len, int mode,
                                    const int32_t* labels, int64_t* out_units, int64_t* out_variants, int64_t* out_len,
                                    int64_t total_entries, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (occ_refused(set_ptr, set_nodes, n_sets, max_set_len, mode, labels, total_entries, workspace, workspace_bytes))
        return SGNN_ERR_BAD_ARG;
    if (n_sets > 0 && (!out_units || !out_variants || !out_len)) return SGNN_ERR_BAD_ARG;
    if (n_sets == 0) return SGNN_OK;
    OccArgs a = {};
    a.set_ptr = set_ptr; a.set_nodes = set_nodes; a.labels = labels; a.n_sets = n_sets;
    a.out_units = out_units; a.out_variants = out_variants; a.out_len = out_len;
    occ_workspace(a, workspace, total_entries);
    if (mode == SGNN_OCC_COMPONENT) occ_launch<true, false>(a, max_set_len, (hipStream_t)stream);
    else occ_launch<false, false>(a, max_set_len, (hipStream_t)stream);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_occlusion_write(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len, int mode,
                                    const int32_t* labels, const int64_t* var_ptr, const int64_t* len_scan, int64_t n_variants,
                                    int64_t* out_ptr, int32_t* out_nodes, int32_t* out_parent, int32_t* out_unit, uint64_t* out_keys,
                                    int64_t total_entries, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (occ_refused(set_ptr, set_nodes, n_sets, max_set_len, mode, labels, total_entries, workspace, workspace_bytes) || n_variants < 0)
        return SGNN_ERR_BAD_ARG;
    if (n_variants > 0 && (n_sets == 0 || !var_ptr || !len_scan || !out_ptr || !out_nodes || !out_parent || !out_unit || !out_keys))
        return SGNN_ERR_BAD_ARG;
    if (n_sets == 0 || n_variants == 0) return SGNN_OK;
    OccArgs a = {};
    a.set_ptr = set_ptr; a.set_nodes = set_nodes; a.labels = labels; a.n_sets = n_sets;
    a.var_ptr = var_ptr; a.len_scan = len_scan; a.n_variants = n_variants;
    a.out_ptr = out_ptr; a.out_nodes = out_nodes; a.out_parent = out_parent; a.out_unit = out_unit; a.out_keys = out_keys;
    occ_workspace(a, workspace, total_entries);
    if (mode == SGNN_OCC_COMPONENT) occ_launch<true, true>(a, max_set_len, (hipStream_t)stream);
    else occ_launch<false, true>(a, max_set_len, (hipStream_t)stream);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

SGNN_DEFINE_WARM(occlusion)

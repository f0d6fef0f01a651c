// Node overlap of ragged node sets (subgnn_hip.h, sgnn_overlap_topk / sgnn_overlap_diverse): which rows of a bank share nodes
// with a set, and how many.  No float work; every result is an integer, every order a comparison of integers.
//
// A bank carries its postings: for node id v, post_rows[post_ptr[v] .. post_ptr[v + 1]) are the bank rows that hold v,
// ascending.  The counting body (ovl_count) is the whole workgroup over ONE set: sixteen lanes per member walk the member's
// posting list and add 1 to the entry of every row met, in an open-addressing table of id_table.h's slot rule keyed by
// row + 1 (0 = empty), the counter an integer atomicAdd beside the key -- so the table's content, as a set of (row, count)
// pairs, does not depend on the order.  The table has the smallest power of two >= max(64, 2 P) slots for the P postings the
// set walks (at most P rows are met: load <= 1/2).  Its home follows id_table.h: P <= SGNN_SET_LDS_MAX in LDS, beyond it in the
// caller's workspace, every set in the region at its own offset, read there by agent-scope loads behind a device-wide fence.
//
// sgnn_overlap_topk: one workgroup per query: count, then one sweep that gives every met row its denominator, counts the rows
// met and strikes the excluded row, then k rounds of a workgroup arg-best under the exact order; the round's winner is struck.
// sgnn_overlap_diverse: ONE workgroup walks the ranked sets: the cursor skips suppressed rows, the accepted set is counted
// against the sets' own postings, and every later row that is too similar is marked -- nothing is read back by the host.
//
// Every loop is bounded by what it walks: the queries or rows, a set's members, a member's postings, the table's slots, k.
#include "id_table.h"

#define OVL_THREADS 256
#define OVL_WAVES   (OVL_THREADS / 64)
#define OVL_GROUP   16                                      // lanes that share one member's posting list
#define OVL_MAX_K   64
#define OVL_MIN_HALF 32                                     // a table has at least 2 * this many slots
#define OVL_MAX_ENTRIES (1ll << 28)                         // postings of the workspace regions of one call (id_table.h)

template <bool LDS> __device__ __forceinline__ void ovl_st(int32_t* p, int32_t v) {          // a store idt_ld<LDS> reads back
    if (LDS) *p = v; else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the table of a set that walks P postings: `pos` holds the counters
__device__ __forceinline__ IdTable ovl_table(int32_t* key, int32_t* cnt, int64_t P) {
    const int n = P < OVL_MIN_HALF ? OVL_MIN_HALF : (int)P;
    return IdTable{key, cnt, __clz(2 * n - 1)};
}

// one more shared node with row r: id_table.h's insert (CAS on the empty key, linear probing) with the counter beside it
__device__ __forceinline__ void ovl_add(const IdTable& t, int32_t r) {
    const uint32_t slots = idt_slots(t), mask = slots - 1;
    const int32_t v = r + 1;
    uint32_t h = idt_slot(t, v);
    for (uint32_t tries = 0; tries < slots; ++tries) {
        const int32_t old = atomicCAS(&t.key[h], 0, v);
        if (old == 0 || old == v) { atomicAdd(&t.pos[h], 1); return; }
        h = (h + 1) & mask;
    }
}

// the whole workgroup: the table of the rows that share a node with nodes[0, n), readable when it returns
template <bool LDS>
__device__ __forceinline__ void ovl_count(const IdTable& t, const int32_t* __restrict__ nodes, int n,
                                          const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post_rows,
                                          int64_t max_id, int64_t n_rows, int tid)
{
    const uint32_t slots = idt_slots(t);
    for (uint32_t i = tid; i < slots; i += OVL_THREADS) { t.key[i] = 0; t.pos[i] = 0; }
    idt_sync<LDS>();
    const int group = tid / OVL_GROUP, lane = tid % OVL_GROUP;
    for (int i = group; i < n; i += OVL_THREADS / OVL_GROUP) {
        const int64_t v = nodes[i];
        if (v < 0 || v > max_id) continue;                           // no bank row holds it
        const int64_t beg = post_ptr[v], end = post_ptr[v + 1];
        for (int64_t j = beg + lane; j < end; j += OVL_GROUP) {
            const int32_t r = post_rows[j];
            if ((uint64_t)r < (uint64_t)n_rows) ovl_add(t, r);
        }
    }
    idt_sync<LDS>();
}

// ---- the order: the larger fraction n / d (d > 0) first, equal fractions by the smaller row; n = 0 is no candidate
struct OvlBest { int32_t n, d, row, slot; };

__device__ __forceinline__ bool ovl_better(const OvlBest& a, const OvlBest& b) {
    const int64_t l = (int64_t)a.n * b.d, r = (int64_t)b.n * a.d;
    return l > r || (l == r && a.row < b.row);
}

__device__ __forceinline__ int32_t ovl_den(int measure, int32_t i, int32_t q, int32_t b) {
    return measure == SGNN_OVL_JACCARD ? q + b - i : measure == SGNN_OVL_CONTAINMENT ? q : measure == SGNN_OVL_COVERAGE ? b : 1;
}

struct OvlTopkArgs {
    const int64_t* q_ptr; const int32_t* q_nodes; int64_t n_q;
    const int64_t* q_postings; const int64_t* q_ws_off;
    const int64_t* bank_ptr; int64_t n_rows;
    const int64_t* post_ptr; const int32_t* post_rows; int64_t max_id;
    const int64_t* exclude; int k, measure;
    int32_t* ws; int64_t ws_entries;
    int64_t* out_rows; int32_t* out_inter; int32_t* out_touched;
};

template <bool LDS>
__global__ __launch_bounds__(OVL_THREADS) void ovl_topk_kernel(const OvlTopkArgs a)
{
    constexpr int NL = LDS ? SGNN_SET_LDS_HASH : 1;
    __shared__ int32_t s_key[NL], s_cnt[NL], s_den[NL];
    __shared__ OvlBest s_best[OVL_WAVES];
    __shared__ int s_touched;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int64_t s = blockIdx.x; s < a.n_q; s += gridDim.x) {
        const int64_t P = a.q_postings[s];
        if (P < 0 || (P <= SGNN_SET_LDS_MAX) != LDS) continue;       // the other launch's (the same for the whole workgroup)
        const int64_t qbeg = a.q_ptr[s];
        const int nq = (int)(a.q_ptr[s + 1] - qbeg);
        int64_t* __restrict__ o_rows = a.out_rows + s * a.k;
        int32_t* __restrict__ o_inter = a.out_inter + s * a.k;
        int32_t *key = s_key, *cnt = s_cnt, *den = s_den;
        bool fits = true;
        if (!LDS) {
            const int64_t off = a.q_ws_off ? a.q_ws_off[s] : -1;
            fits = off >= 0 && P <= a.ws_entries && off <= a.ws_entries - P;
            if (fits) { key = a.ws + 4 * off; cnt = key + 4 * a.ws_entries; den = cnt + 4 * a.ws_entries; }
        }
        if (!fits) {                                                 // a region the workspace does not hold: fillers
            for (int j = tid; j < a.k; j += OVL_THREADS) { o_rows[j] = -1; o_inter[j] = 0; }
            if (tid == 0) a.out_touched[s] = 0;
            continue;
        }
        const IdTable t = ovl_table(key, cnt, P);
        const uint32_t slots = idt_slots(t);
        if (tid == 0) s_touched = 0;                                 // (ovl_count's barriers stand between this and its use)
        ovl_count<LDS>(t, a.q_nodes + qbeg, nq, a.post_ptr, a.post_rows, a.max_id, a.n_rows, tid);

        // denominators, the number of rows met, the excluded row
        const int64_t skip = a.exclude ? a.exclude[s] : -1;
        int met = 0;
        for (uint32_t i = tid; i < slots; i += OVL_THREADS) {
            const int32_t kk = idt_ld<LDS>(key + i);
            if (kk == 0) continue;
            const int32_t row = kk - 1, c = idt_ld<LDS>(cnt + i);
            ovl_st<LDS>(den + i, ovl_den(a.measure, c, nq, (int32_t)(a.bank_ptr[row + 1] - a.bank_ptr[row])));
            if (row == skip) ovl_st<LDS>(cnt + i, 0);
            ++met;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) met += __shfl_xor(met, d);
        if (lane == 0 && met) atomicAdd(&s_touched, met);
        idt_sync<LDS>();
        if (tid == 0) a.out_touched[s] = s_touched;

        for (int j = 0; j < a.k; ++j) {
            OvlBest b = {0, 1, 0x7fffffff, -1};
            for (uint32_t i = tid; i < slots; i += OVL_THREADS) {
                const int32_t c = idt_ld<LDS>(cnt + i);
                if (c <= 0) continue;
                const OvlBest x = {c, idt_ld<LDS>(den + i), idt_ld<LDS>(key + i) - 1, (int32_t)i};
                if (ovl_better(x, b)) b = x;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const OvlBest x = {__shfl_xor(b.n, d), __shfl_xor(b.d, d), __shfl_xor(b.row, d), __shfl_xor(b.slot, d)};
                if (ovl_better(x, b)) b = x;
            }
            if (lane == 0) s_best[wave] = b;
            __syncthreads();
            b = s_best[0];
#pragma unroll
            for (int w = 1; w < OVL_WAVES; ++w) { const OvlBest x = s_best[w]; if (ovl_better(x, b)) b = x; }
            if (tid == 0) {
                o_rows[j] = b.n > 0 ? (int64_t)b.row : -1;
                o_inter[j] = b.n;
                if (b.n > 0) ovl_st<LDS>(cnt + b.slot, 0);           // struck: the next round does not see it
            }
            idt_sync<LDS>();                                         // (also: s_best is read before the next round writes it)
        }
    }
}

struct OvlDiverseArgs {
    const int64_t* set_ptr; const int32_t* set_nodes; int64_t n_sets;
    const int64_t* set_postings;
    const int64_t* post_ptr; const int32_t* post_rows; int64_t max_id;
    int64_t tau_num, tau_den, top;
    int32_t* ws; int64_t ws_entries;
    int64_t* out_accepted; int32_t* out_n; int32_t* out_by;
};

// rows c > r that share too much with the accepted row r are marked: i * tau_den > tau_num * (|r| + |c| - i)
template <bool LDS>
__device__ __forceinline__ void ovl_suppress(const OvlDiverseArgs& a, int32_t* key, int32_t* cnt, int64_t P, int64_t r, int tid)
{
    const int64_t beg = a.set_ptr[r];
    const int nr = (int)(a.set_ptr[r + 1] - beg);
    const IdTable t = ovl_table(key, cnt, P);
    ovl_count<LDS>(t, a.set_nodes + beg, nr, a.post_ptr, a.post_rows, a.max_id, a.n_sets, tid);
    const uint32_t slots = idt_slots(t);
    for (uint32_t i = tid; i < slots; i += OVL_THREADS) {
        const int32_t kk = idt_ld<LDS>(key + i);
        if (kk == 0) continue;
        const int64_t c = kk - 1;
        if (c <= r || idt_ld<false>(a.out_by + c) >= 0) continue;
        const int64_t shared = idt_ld<LDS>(cnt + i), nc = a.set_ptr[c + 1] - a.set_ptr[c];
        if (shared * a.tau_den > a.tau_num * (nr + nc - shared)) ovl_st<false>(a.out_by + c, (int32_t)r);
    }
    idt_sync<false>();                                               // the marks, before the cursor reads them
}

__global__ __launch_bounds__(OVL_THREADS) void ovl_diverse_kernel(const OvlDiverseArgs a)
{
    __shared__ int32_t s_key[SGNN_SET_LDS_HASH], s_cnt[SGNN_SET_LDS_HASH];
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < a.n_sets; i += OVL_THREADS) ovl_st<false>(a.out_by + i, -1);
    for (int64_t i = tid; i < a.top; i += OVL_THREADS) a.out_accepted[i] = -1;
    idt_sync<false>();
    int64_t n_acc = 0;
    for (int64_t r = 0; r < a.n_sets && n_acc < a.top; ++r) {
        if (idt_ld<false>(a.out_by + r) >= 0) continue;              // one word, the same for every thread
        if (tid == 0) a.out_accepted[n_acc] = r;
        ++n_acc;
        if (n_acc == a.top) break;
        const int64_t P = a.set_postings[r];
        if (P <= SGNN_SET_LDS_MAX) ovl_suppress<true>(a, s_key, s_cnt, P < 0 ? 0 : P, r, tid);
        else if (P <= a.ws_entries) ovl_suppress<false>(a, a.ws, a.ws + 4 * a.ws_entries, P, r, tid);
    }
    if (tid == 0) a.out_n[0] = (int32_t)n_acc;
}

extern "C" int64_t sgnn_overlap_max_k(void) { return OVL_MAX_K; }
extern "C" int64_t sgnn_overlap_lds_max(void) { return SGNN_SET_LDS_MAX; }

// three tables (keys, counters, denominators) of 4 slots per posting
extern "C" int64_t sgnn_overlap_workspace_bytes(int64_t entries)
{
    if (entries < 0 || entries > OVL_MAX_ENTRIES) return -1;
    return entries * 48;
}

extern "C" int sgnn_overlap_topk(const int64_t* q_ptr, const int32_t* q_nodes, int64_t n_queries, const int64_t* q_postings,
                                 const int64_t* q_ws_off, const int64_t* bank_ptr, int64_t n_rows, const int64_t* post_ptr,
                                 const int32_t* post_rows, int64_t max_id, const int64_t* exclude, int64_t k, int measure,
                                 void* workspace, int64_t ws_entries, int64_t workspace_bytes, int64_t* out_rows,
                                 int32_t* out_inter, int32_t* out_touched, void* stream)
{
    if (n_queries < 0 || n_queries > 0x7fffffff || n_rows < 0 || n_rows > 0x7fffffff || max_id < 0 || max_id > 0x7fffffff)
        return SGNN_ERR_BAD_ARG;
    if (k < 1 || k > OVL_MAX_K || measure < SGNN_OVL_JACCARD || measure > SGNN_OVL_COUNT) return SGNN_ERR_BAD_ARG;
    if (ws_entries < 0 || ws_entries > OVL_MAX_ENTRIES || workspace_bytes < ws_entries * 48 || (ws_entries > 0 && !workspace))
        return SGNN_ERR_BAD_ARG;
    if (n_queries == 0) return SGNN_OK;
    if (!q_ptr || !q_nodes || !q_postings || !bank_ptr || !post_ptr || !post_rows || !out_rows || !out_inter || !out_touched)
        return SGNN_ERR_BAD_ARG;
    if (ws_entries > 0 && !q_ws_off) return SGNN_ERR_BAD_ARG;
    OvlTopkArgs a = {};
    a.q_ptr = q_ptr; a.q_nodes = q_nodes; a.n_q = n_queries; a.q_postings = q_postings; a.q_ws_off = q_ws_off;
    a.bank_ptr = bank_ptr; a.n_rows = n_rows; a.post_ptr = post_ptr; a.post_rows = post_rows; a.max_id = max_id;
    a.exclude = exclude; a.k = (int)k; a.measure = measure;
    a.ws = (int32_t*)workspace; a.ws_entries = ws_entries;
    a.out_rows = out_rows; a.out_inter = out_inter; a.out_touched = out_touched;
    const dim3 grid(sgnn_grid_for(n_queries, 1));
    hipLaunchKernelGGL(ovl_topk_kernel<true>, grid, dim3(OVL_THREADS), 0, (hipStream_t)stream, a);
    // (without a workspace a query beyond the LDS tier has no region: the second launch writes its fillers)
    hipLaunchKernelGGL(ovl_topk_kernel<false>, grid, dim3(OVL_THREADS), 0, (hipStream_t)stream, a);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_overlap_diverse(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, const int64_t* set_postings,
                                    const int64_t* post_ptr, const int32_t* post_rows, int64_t max_id, int64_t tau_num,
                                    int64_t tau_den, int64_t top, void* workspace, int64_t ws_entries, int64_t workspace_bytes,
                                    int64_t* out_accepted, int32_t* out_n, int32_t* out_suppressed_by, void* stream)
{
    if (n_sets < 0 || n_sets > 0x7fffffff || max_id < 0 || max_id > 0x7fffffff || top < 1 || top > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    if (tau_den < 1 || tau_den > (1ll << 20) || tau_num < 0 || tau_num > tau_den) return SGNN_ERR_BAD_ARG;
    if (ws_entries < 0 || ws_entries > OVL_MAX_ENTRIES || workspace_bytes < ws_entries * 48 || (ws_entries > 0 && !workspace))
        return SGNN_ERR_BAD_ARG;
    if (!out_accepted || !out_n || (n_sets > 0 && (!set_ptr || !set_nodes || !set_postings || !post_ptr || !post_rows || !out_suppressed_by)))
        return SGNN_ERR_BAD_ARG;
    OvlDiverseArgs a = {};
    a.set_ptr = set_ptr; a.set_nodes = set_nodes; a.n_sets = n_sets; a.set_postings = set_postings;
    a.post_ptr = post_ptr; a.post_rows = post_rows; a.max_id = max_id;
    a.tau_num = tau_num; a.tau_den = tau_den; a.top = top;
    a.ws = (int32_t*)workspace; a.ws_entries = ws_entries;
    a.out_accepted = out_accepted; a.out_n = out_n; a.out_by = out_suppressed_by;
    hipLaunchKernelGGL(ovl_diverse_kernel, dim3(1), dim3(OVL_THREADS), 0, (hipStream_t)stream, a);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

SGNN_DEFINE_WARM(overlap)

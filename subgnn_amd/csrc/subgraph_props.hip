// Structural properties of induced subgraphs: the quantities behind the DENSITY, CUT RATIO, CORENESS and COMPONENT labels of
// the synthetic benchmarks (reference prepare_dataset/prepare_dataset.py:519-550: nx.density, nx.edge_boundary,
// nx.core_number and nx.number_connected_components of G.subgraph(nodes)), for every ragged set at once.  Integer only.
//
// A MEMBER of a set is an entry v with 1 <= v <= max_id whose CSR row is not empty; every other entry (PAD = 0 included) is
// dropped, as G.subgraph drops ids that are not nodes, and a repeated id counts once (its first position stands for it).
// Per set, int64[6]: {members, edges among them (no self loops, an undirected edge once, an id repeated inside a CSR row once),
// members with a self loop, boundary edges = distinct (member, non-member neighbour) pairs, connected components, sum of the
// members' core numbers (self loops ignored)}.  Per position (optional), int32: the member's core number, -1 for a dropped entry.
//
// Tiers, by the number of ENTRIES of the set (id_table.h):
//   <= SGNN_SET_WAVE_MAX  one wavefront per set, lane i owns entry i.  The n (n - 1) / 2 pairs are tested 64 per round by a
//                         binary search of the shorter of the two sorted rows (a hub's list is never streamed for a 20-node
//                         set); the hits become the 64-bit rows of the induced adjacency matrix, one row per lane, in a register.
//                         From there nothing leaves the registers: edges = sum of popcounts / 2, components = Warshall closure
//                         of the bit rows (row k is broadcast at step k), cores = peeling under a wave-uniform alive mask
//                         (__ballot): lanes with popcount(row & alive) <= k leave with core k; k rises when none is left.
//   <= SGNN_SET_LDS_MAX   one 256-thread workgroup per set, its tables in LDS (56 KiB: two workgroups per CU).  Bit rows of 2048
//                         members would be 512 KiB, so this form keeps counters instead: an id -> first position hash table,
//                         union-find parents, the current induced degree per member and a removal queue.  One wavefront streams
//                         a member's row against the table (degree, boundary, self loop, unions); the peel is level-synchronous:
//                         members of degree <= k are queued and marked with their core, their rows are streamed again to
//                         decrement the neighbours, and k jumps to the smallest remaining degree when the queue stays empty.
//   >  SGNN_SET_LDS_MAX   the same workgroup code with the tables in the caller's workspace (11 int32 per entry, each set at its
//                         own offset; sgnn_subgraph_properties_workspace_bytes).  No set size is refused.
// Every table is initialised by the set that uses it: neither LDS nor the workspace carries anything from one set or call to
// the next.
#include "id_table.h"

SGNN_DEFINE_WARM(subgraph_props)

#define SP_THREADS 256
#define SP_WAVES 4                      // wave tier: wavefronts (= sets) per workgroup
#define SP_DROPPED INT32_MIN            // deg[] marks of the workgroup form: entry is no member ...
#define SP_REPEAT (INT32_MIN + 1)       // ... entry repeats an earlier member; >= 0: alive with that degree; -1 - k: left with core k

__device__ __forceinline__ int32_t sp_wave_sum(int32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__device__ __forceinline__ uint64_t sp_bcast64(uint64_t x, int l) {      // l is wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// ---- sets of at most 64 entries ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * SP_WAVES) void subgraph_props_wave_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t max_id, int rows_simple,
    const int64_t* __restrict__ sub_ptr, const int32_t* __restrict__ sub_nodes, int64_t n_sets, int poison_larger,
    int64_t* __restrict__ out_counts, int32_t* __restrict__ out_core)
{
    const int lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6); s < n_sets; s += (int64_t)gridDim.x * SP_WAVES) {
        const int64_t beg = sub_ptr[s];
        const int64_t len = sub_ptr[s + 1] - beg;
        if (len > SGNN_SET_WAVE_MAX) {                            // (wave-uniform) the workgroup form owns it ...
            if (poison_larger) {                            // ... unless the caller promised there was no such set: marked, never stale
                if (lane < 6) out_counts[s * 6 + lane] = -1;
                if (out_core) for (int64_t i = lane; i < len; i += 64) out_core[beg + i] = -1;
            }
            continue;
        }
        const int n = __builtin_amdgcn_readfirstlane(len < 0 ? 0 : (int)len);      // (the same in every lane: the loops below are scalar)
        int32_t v = 0, deg = 0;
        uint32_t r0 = 0;
        if (lane < n) {
            v = sub_nodes[beg + lane];
            if (v >= 1 && (int64_t)v <= max_id) {           // (the bound comes first: rowptr has max_id + 2 entries)
                const int64_t a = rowptr[v];
                r0 = (uint32_t)a;
                deg = (int32_t)(rowptr[v + 1] - a);
            }
        }
        const bool member = deg > 0;
        int first = lane;                                   // the first position that holds my id
        for (int j = 0; j < n; ++j) {
            const int32_t vj = __builtin_amdgcn_readlane(v, j);
            if (member && vj == v && j < first) first = j;
        }
        const bool own = member && first == lane;           // one lane per distinct member
        const uint64_t members = __ballot(own);
        // ---- the bit rows: pair p = j (j - 1) / 2 + i (i < j), 64 pairs per round
        uint64_t row = 0;
        const int npairs = n * (n - 1) / 2;
        for (int p0 = 0; p0 < npairs; p0 += 64) {
            const int p = p0 + lane;
            int i = 0, j = 0;
            if (p < npairs) {
                j = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
                while (j * (j - 1) / 2 > p) --j;
                while ((j + 1) * j / 2 <= p) ++j;
                i = p - j * (j - 1) / 2;
            }
            const int32_t vi = __shfl(v, i), vj = __shfl(v, j);
            const int32_t di = __shfl(deg, i), dj = __shfl(deg, j);
            const uint32_t ri = __shfl(r0, i), rj = __shfl(r0, j);
            bool linked = false;
            if (p < npairs && ((members >> i) & 1) && ((members >> j) & 1)) {
                if (di <= dj) linked = sgnn_sorted_contains(col + ri, di, vj);
                else linked = sgnn_sorted_contains(col + rj, dj, vi);
            }
            uint64_t hits = __ballot(linked);
            while (hits) {                                  // (wave-uniform) one step per edge found
                const int l = __ffsll((unsigned long long)hits) - 1;
                hits &= hits - 1;
                const int a = __builtin_amdgcn_readlane(i, l), b = __builtin_amdgcn_readlane(j, l);
                if (lane == a) row |= 1ull << b;
                if (lane == b) row |= 1ull << a;
            }
        }
        const bool self_loop = own && sgnn_sorted_contains(col + r0, deg, v);
        // neighbours that are not the member itself, an id once
        int32_t distinct = deg - (self_loop ? 1 : 0);
        if (!rows_simple) {                                 // rows may repeat an id: count each row's runs, one row per step
            uint64_t m = members;
            while (m) {
                const int j = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const int32_t vj = __builtin_amdgcn_readlane(v, j), dj = __builtin_amdgcn_readlane(deg, j);
                const uint32_t rj = (uint32_t)__builtin_amdgcn_readlane((int)r0, j);
                int32_t c = 0;
                for (int32_t e = lane; e < dj; e += 64) {
                    const int32_t u = col[rj + (uint32_t)e];
                    c += (u != vj && (e == 0 || col[rj + (uint32_t)e - 1u] != u)) ? 1 : 0;
                }
                c = sp_wave_sum(c);
                if (lane == j) distinct = c;
            }
        }
        const int32_t internal = __popcll(row);
        // ---- components: transitive closure of the rows (Warshall: at step k every row that reaches k takes row k)
        uint64_t reach = own ? (row | (1ull << lane)) : 0ull;
        for (int k = 0; k < n; ++k) {
            const uint64_t rk = sp_bcast64(reach, k);
            if ((reach >> k) & 1) reach |= rk;
        }
        const bool root = own && (__ffsll((unsigned long long)reach) - 1 == lane);
        // ---- cores: peel
        uint64_t alive = members;
        int32_t core = 0;
        int k = 0;
        while (alive) {                                     // (wave-uniform: alive comes out of __ballot)
            const bool in = (alive >> lane) & 1;
            const bool leave = in && __popcll(row & alive) <= k;
            const uint64_t gone = __ballot(leave);
            if (gone) { if (leave) core = k; alive &= ~gone; }
            else ++k;
        }
        // ---- results (a set has at most 64 x 63 / 2 edges and its core sum at most 64 x 63: both halves of one word)
        const int32_t packed = sp_wave_sum(own ? (internal | (core << 16)) : 0);
        const int32_t boundary = sp_wave_sum(own ? distinct - internal : 0);
        const int n_self = __popcll(__ballot(self_loop)), n_comp = __popcll(__ballot(root));
        if (lane == 0) {
            int64_t* o = out_counts + s * 6;
            o[0] = __popcll(members);
            o[1] = (packed & 0xffff) >> 1;
            o[2] = n_self;
            o[3] = boundary;
            o[4] = n_comp;
            o[5] = packed >> 16;
        }
        if (out_core) {
            const int32_t c = __shfl(core, first);
            if (lane < n) out_core[beg + lane] = member ? c : -1;
        }
    }
}

// ---- sets of more than 64 entries: one workgroup per set, tables in LDS or in the workspace ---------------------------------
// (the id table gives the first position of a member's id; how the tables are read and fenced per home: id_table.h)
struct SpTables { IdTable t; int32_t* par; int32_t* deg; int32_t* queue; };

template <bool LDS>
__global__ __launch_bounds__(SP_THREADS) void subgraph_props_block_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t max_id,
    const int64_t* __restrict__ sub_ptr, const int32_t* __restrict__ sub_nodes, int64_t n_sets, int poison_larger,
    int64_t* __restrict__ out_counts, int32_t* __restrict__ out_core, int32_t* __restrict__ ws)
{
    __shared__ int32_t s_hk[LDS ? SGNN_SET_LDS_HASH : 1], s_hv[LDS ? SGNN_SET_LDS_HASH : 1];
    __shared__ int32_t s_par[LDS ? SGNN_SET_LDS_MAX : 1], s_deg[LDS ? SGNN_SET_LDS_MAX : 1], s_queue[LDS ? SGNN_SET_LDS_MAX : 1];
    __shared__ int32_t s_members, s_self, s_boundary, s_comp, s_qn[2], s_min[2];
    __shared__ unsigned long long s_deg_sum, s_core_sum;
    const int tid = threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t total = sub_ptr[n_sets];
    for (int64_t s = blockIdx.x; s < n_sets; s += gridDim.x) {
        const int64_t beg = sub_ptr[s];
        const int64_t len = sub_ptr[s + 1] - beg;
        if (len <= SGNN_SET_WAVE_MAX) continue;                   // (block-uniform) the wave form owns it
        if (LDS && len > SGNN_SET_LDS_MAX) {
            if (poison_larger) {                            // no workspace was given: marked, never left as it was
                if (tid < 6) out_counts[s * 6 + tid] = -1;
                if (out_core) for (int64_t i = tid; i < len; i += SP_THREADS) out_core[beg + i] = -1;
            }
            continue;
        }
        if (!LDS && len <= SGNN_SET_LDS_MAX) continue;
        const int n = (int)len;
        const int32_t* nodes = sub_nodes + beg;
        SpTables t;
        if (LDS) {
            t.t = idt_in_lds(s_hk, s_hv); t.par = s_par; t.deg = s_deg; t.queue = s_queue;
        } else {                                            // keys[4 total] | positions[4 total] | par[total] | deg[total] | queue[total]
            t.t = idt_in_workspace(ws, beg, n, ws + 4 * total);
            t.par = ws + 8 * total + beg; t.deg = ws + 9 * total + beg; t.queue = ws + 10 * total + beg;
        }
        idt_clear<true>(t.t, tid, SP_THREADS);
        if (tid == 0) { s_members = 0; s_self = 0; s_boundary = 0; s_comp = 0; s_deg_sum = 0ull; s_core_sum = 0ull; s_qn[0] = 0; s_min[0] = 0x7fffffff; }
        idt_sync<LDS>();
        for (int i = tid; i < n; i += SP_THREADS) {
            const int32_t v = nodes[i];
            const bool member = v >= 1 && (int64_t)v <= max_id && rowptr[v + 1] > rowptr[v];
            t.par[i] = i;
            t.deg[i] = member ? SP_REPEAT : SP_DROPPED;     // (the first position of an id is set to its degree below)
            if (member) idt_insert<true>(t.t, v, i);
        }
        idt_sync<LDS>();
        // ---- a member's row by one wavefront: induced degree, boundary, self loop, unions
        for (int i = wave; i < n; i += SP_THREADS / 64) {
            if (idt_ld<LDS>(t.deg + i) == SP_DROPPED) continue;   // (wave-uniform)
            const int32_t v = nodes[i];
            if (idt_first<LDS>(t.t, v) != i) continue;             // a repeat: its first position stands for it
            const int64_t a = rowptr[v], b = rowptr[v + 1];
            int32_t cnt = 0, bnd = 0, self = 0;
            for (int64_t e = a + lane; e < b; e += 64) {
                const int32_t u = col[e];
                if (e > a && col[e - 1] == u) continue;     // an id repeated inside the row counts once
                if (u == v) { self = 1; continue; }
                const int j = idt_first<LDS>(t.t, u);
                if (j >= 0) { ++cnt; uf_union<LDS>(t.par, i, j); }
                else ++bnd;
            }
            cnt = sp_wave_sum(cnt);
            bnd = sp_wave_sum(bnd);
            self = sp_wave_sum(self);
            if (lane == 0) {
                t.deg[i] = cnt;
                atomicAdd(&s_members, 1);
                atomicAdd(&s_self, self);
                atomicAdd(&s_boundary, bnd);
                atomicAdd(&s_deg_sum, (unsigned long long)cnt);
            }
        }
        idt_sync<LDS>();
        {
            int roots = 0;
            for (int i = tid; i < n; i += SP_THREADS) roots += (idt_ld<LDS>(t.deg + i) >= 0 && uf_find<LDS>(t.par, i) == i) ? 1 : 0;
            if (roots) atomicAdd(&s_comp, roots);
        }
        // ---- level-synchronous peel.  Two barriers per round; the queue length and the smallest remaining degree alternate
        // between two slots, so that the slot of the next round is reset while this round's is still being read
        int alive = s_members;                              // (block-uniform: read behind the barrier above)
        int k = 0, round = 0;
        unsigned long long core_sum = 0ull;
        while (alive > 0) {
            const int cur = round & 1;
            ++round;
            for (int i = tid; i < n; i += SP_THREADS) {
                const int32_t d = idt_ld<LDS>(t.deg + i);
                if (d < 0) continue;
                if (d <= k) {
                    t.deg[i] = -1 - k;
                    t.queue[atomicAdd(&s_qn[cur], 1)] = i;
                    core_sum += (unsigned long long)k;
                } else atomicMin(&s_min[cur], d);
            }
            idt_sync<LDS>();
            const int qn = s_qn[cur], next_k = s_min[cur];
            if (tid == 0) { s_qn[cur ^ 1] = 0; s_min[cur ^ 1] = 0x7fffffff; }
            alive -= qn;
            if (alive == 0) break;                          // (block-uniform)
            if (qn == 0) k = next_k;                        // nothing left at this level: on to the smallest degree there is
            if (qn == 0 && next_k == 0x7fffffff) break;     // (cannot happen on a symmetric CSR; an asymmetric one must not spin)
            for (int q = wave; q < qn; q += SP_THREADS / 64) {
                const int i = idt_ld<LDS>(t.queue + q);
                const int32_t v = nodes[i];
                const int64_t a = rowptr[v], b = rowptr[v + 1];
                for (int64_t e = a + lane; e < b; e += 64) {
                    const int32_t u = col[e];
                    if (u == v || (e > a && col[e - 1] == u)) continue;
                    const int j = idt_first<LDS>(t.t, u);
                    // (members that have left hold a negative mark, and none leaves during this phase)
                    if (j >= 0 && idt_ld<LDS>(t.deg + j) >= 0) atomicSub(&t.deg[j], 1);
                }
            }
            idt_sync<LDS>();
        }
        if (core_sum) atomicAdd(&s_core_sum, core_sum);
        idt_sync<LDS>();
        if (tid == 0) {
            int64_t* o = out_counts + s * 6;
            o[0] = s_members;
            o[1] = (int64_t)(s_deg_sum >> 1);
            o[2] = s_self;
            o[3] = s_boundary;
            o[4] = s_comp;
            o[5] = (int64_t)s_core_sum;
        }
        if (out_core) {
            for (int i = tid; i < n; i += SP_THREADS) {
                int32_t d = idt_ld<LDS>(t.deg + i);
                if (d == SP_REPEAT) d = idt_ld<LDS>(t.deg + idt_first<LDS>(t.t, nodes[i]));
                out_core[beg + i] = d == SP_DROPPED ? -1 : -1 - d;
            }
        }
        idt_sync<LDS>();                                          // the next set re-initialises the tables
    }
}

extern "C" int64_t sgnn_subgraph_properties_workspace_bytes(int64_t total_nodes)
{
    return (total_nodes < 0 ? 0 : total_nodes) * 11 * 4 + 64;
}

extern "C" int sgnn_subgraph_properties(const int64_t* rowptr, const int32_t* col_sorted, int64_t nnz, int64_t max_id,
                                        int rows_simple, const int64_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sets,
                                        int64_t max_len, int64_t total_nodes, int64_t* out_counts, int32_t* out_core,
                                        void* workspace, int64_t workspace_bytes, void* stream)
{
    if (!rowptr || !col_sorted || !sub_ptr || !sub_nodes || !out_counts || n_sets < 0 || max_id < 0 || nnz < 0 || total_nodes < 0)
        return SGNN_ERR_BAD_ARG;
    if (nnz >= (1ll << 31)) return SGNN_ERR_NNZ_TOO_LARGE;
    if (max_id >= (1ll << 31) - 1) return SGNN_ERR_BAD_ARG;
    const bool huge = max_len > SGNN_SET_LDS_MAX;                 // the caller says so: such sets need the workspace
    if (huge) {
        if (!workspace || workspace_bytes < sgnn_subgraph_properties_workspace_bytes(total_nodes)) return SGNN_ERR_BAD_ARG;
        if (total_nodes >= (1ll << 28)) return SGNN_ERR_SET_TOO_LARGE;       // 4 x total must index with 32 bits
    }
    if (n_sets == 0) return SGNN_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(subgraph_props_wave_kernel, dim3(sgnn_grid_for(n_sets, SP_WAVES, 1 << 20)), dim3(64 * SP_WAVES), 0, st,
                       rowptr, col_sorted, max_id, rows_simple, sub_ptr, sub_nodes, n_sets,
                       (max_len > 0 && max_len <= SGNN_SET_WAVE_MAX) ? 1 : 0, out_counts, out_core);
    if (max_len <= 0 || max_len > SGNN_SET_WAVE_MAX)
        hipLaunchKernelGGL(subgraph_props_block_kernel<true>, dim3((int)(n_sets < 2048 ? n_sets : 2048)), dim3(SP_THREADS), 0, st,
                           rowptr, col_sorted, max_id, sub_ptr, sub_nodes, n_sets, huge ? 0 : 1, out_counts, out_core, (int32_t*)nullptr);
    if (huge)
        hipLaunchKernelGGL(subgraph_props_block_kernel<false>, dim3((int)(n_sets < 1024 ? n_sets : 1024)), dim3(SP_THREADS), 0, st,
                           rowptr, col_sorted, max_id, sub_ptr, sub_nodes, n_sets, 0, out_counts, out_core, (int32_t*)workspace);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

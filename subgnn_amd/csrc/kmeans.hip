// libsubgnn_hip.so: one Lloyd iteration over a bank of embeddings (sgnn_kmeans_step + sgnn_kmeans_finish) -- every row
// assigned to its best centre under the score and the order of sgnn_topk_rows, and the per-cluster sums formed in the same
// launch, with no (N, K) matrix and no atomics on floats.
//
//   kmeans_step_kernel    one workgroup per SLOT: a contiguous range of 32-row tiles.
//                         Assignment, tile by tile: the rows take the place of topk_rows' queries and the centres that of its
//                         bank -- the same staged chunks of 32 columns, zero-padded, the same v_mfma_f32_32x32x2_f32 chain from 0
//                         over ascending d, the same epilogue -- so a pair's score has topk_rows' bits.  Of a tile of 128 centres
//                         each wave reduces eight rows' 128 keys ((order key of the score << 32) | centre) to their minimum and
//                         keeps the running minimum: the winner of the strict total order, whatever the tiling.  Wave 0 then
//                         writes the tile's 32 (assign, score), counts the rows that differ from prev_assign and adds the scores
//                         in double: a fixed butterfly over the tile's 32 rows (rows past N count 0), tiles in ascending order.
//                         Accumulation, after the slot's last tile: for every chunk of W columns (W = 32, 16 or 8: K * W floats
//                         are 32 KiB of LDS at most) K x W accumulators are zeroed in LDS and the slot's rows pass through in
//                         blocks of 64, staged coalesced.  Thread (column c, group g) of the 256 = W x G adds, in ascending row
//                         order, the rows whose cluster is g modulo G: every accumulator has ONE owner, so there is no conflict
//                         and a cluster's partial sum is the float32 chain acc = acc + x over its rows of the slot, ascending,
//                         from +0.  The chunk's accumulators go to the slot's K x D partial in the workspace; the groups'
//                         owners of column 0 count the rows (integers) on the first chunk.
//   kmeans_finish_kernel  one workgroup per cluster: counts[k] = sum of the slots' counts; sums[k][d] = the chain acc = acc + p
//                         over the slots' partials in slot order from +0; the next centre sums / (float)count (one correctly
//                         rounded division) or the previous centre of a cluster without rows; c_aux_next from the chain
//                         q = fmaf(v, v, q) of each thread over its columns d = t, t + 256, ... followed by the halving tree
//                         q[t] += q[t + 128], q[t + 64], ... , q[t + 1] over the 256 threads.  Workgroup 0 also adds the slots'
//                         inertia (double, slot order) and changed counts and counts the clusters without rows.
#include "common.h"
#include "topk_order.h"
#include <math.h>

#define KM_MAX_K     1024
#define KM_TR        32            // rows per tile (topk_rows' query tile)
#define KM_TC        128           // centres per tile (topk_rows' bank tile): one 32-centre sub-tile per wave
#define KM_THREADS   256
#define KM_RPW       (KM_TR / (KM_THREADS / 64))   // rows per wave in the selection
#define KM_MAX_SLOTS 1024          // partial slots (= workgroups of the step): four per CU
#define KM_PART_CAP  (64ll << 20)  // bytes of the slots' K x D partial sums: fewer slots for wide K * D
#define KM_RB        64            // rows per staged block of the accumulation
#define KM_ACC_BYTES (32 << 10)    // LDS of the K x W accumulators
// LDS, one array used twice: [assignment] row chunk, centre chunk, score tile, row aux, winners;
//                            [accumulation] K x W accumulators, row block, its clusters, counts
#define KM_LDS_ASSIGN ((KM_TR * TK_LD + KM_TC * TK_LD + KM_TR * KM_TC + KM_TR) * 4 + KM_TR * 8)
#define KM_LDS_ACCUM  (KM_ACC_BYTES + KM_RB * 32 * 4 + KM_RB * 4 + KM_MAX_K * 4)
#define KM_LDS_BYTES  (KM_LDS_ACCUM > KM_LDS_ASSIGN ? KM_LDS_ACCUM : KM_LDS_ASSIGN)

__device__ __forceinline__ uint64_t km_min_xor(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    return o < v ? o : v;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_step_kernel(
    const float* __restrict__ x, uint32_t x_stride, int N, const float* __restrict__ cen, uint32_t c_stride, int K, int D,
    int metric, const float* __restrict__ x_aux, const float* __restrict__ c_aux, const int32_t* __restrict__ prev,
    int n_row_tiles, int tiles_per_slot, int log_w, int32_t* assign, float* __restrict__ score, double* __restrict__ ws_inertia,
    float* __restrict__ ws_sums, int32_t* __restrict__ ws_counts, int32_t* __restrict__ ws_changed)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[KM_LDS_BYTES];
    float* const qs = (float*)lds;
    float* const bs = qs + KM_TR * TK_LD;
    float* const sc = bs + KM_TC * TK_LD;
    float* const qaux_s = sc + KM_TR * KM_TC;
    uint64_t* const best_s = (uint64_t*)(qaux_s + KM_TR);          // byte offset 37632: a multiple of 8

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = blockIdx.x;
    const bool lower_better = metric == SGNN_TOPK_L2;
    const int tile_lo = slot * tiles_per_slot, tile_hi = min(tile_lo + tiles_per_slot, n_row_tiles);   // never empty
    const int row_lo = tile_lo * KM_TR, row_hi = min(tile_hi * KM_TR, N);

    const int sr = tid >> 5, scol = tid & 31;          // staging: 8 rows x 32 columns per pass
    const int fr = lane & 31, fk = lane >> 5;          // MFMA operands: row (of x or of the centres) and k of the pair
    const int n_chunks = (D + TK_KC - 1) / TK_KC;
    const int n_ctiles = (K + KM_TC - 1) / KM_TC;
    const int n_steps = n_ctiles * n_chunks;

    double inertia = 0.0;                              // wave 0 only
    int changed = 0;

    // ------------------------------------------------------------------ assignment ---------
    for (int rt = tile_lo; rt < tile_hi; ++rt) {
        const int q0 = rt * KM_TR;                     // < N
        if (tid < KM_TR) qaux_s[tid] = q0 + tid < N ? x_aux[q0 + tid] : 0.0f;   // (read after the chunks' barriers)
        uint64_t best[KM_RPW];
#pragma unroll
        for (int u = 0; u < KM_RPW; ++u) best[u] = TK_FILLER;

        // as topk_rows_kernel: the next step's elements are loaded ahead of this step's MFMAs, every load from an address
        // clamped into its matrix (a wave-uniform 64-bit tile base plus a 32-bit offset per lane: strides are below 2^23),
        // and what lies past D or past the last row is replaced by zero afterwards
        float qv[KM_TR / 8], bv[KM_TC / 8];
        const float* const qt = x + (int64_t)q0 * x_stride;
        const int q_last = N - 1 - q0;                 // >= 0
        auto load_step = [&](int step) {
            const int ct = step / n_chunks, chunk = step - ct * n_chunks;
            const int d = chunk * TK_KC + scol, b0 = ct * KM_TC;
            const bool d_in = d < D;
            const uint32_t dc = d_in ? (uint32_t)d : 0u;
            const float* const bt = cen + (int64_t)b0 * c_stride;
            const int b_last = K - 1 - b0;             // >= 0: the tile exists
#pragma unroll
            for (int p = 0; p < KM_TR / 8; ++p) {
                const int r = sr + 8 * p;
                const float v = qt[(uint32_t)min(r, q_last) * x_stride + dc];
                qv[p] = (d_in && r <= q_last) ? v : 0.0f;
            }
#pragma unroll
            for (int p = 0; p < KM_TC / 8; ++p) {
                const int r = sr + 8 * p;
                const float v = bt[(uint32_t)min(r, b_last) * c_stride + dc];
                bv[p] = (d_in && r <= b_last) ? v : 0.0f;
            }
        };
        tk_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        load_step(0);
        int step = 0;
        for (int ct = 0; ct < n_ctiles; ++ct) {
            const int b0 = ct * KM_TC;
            for (int chunk = 0; chunk < n_chunks; ++chunk, ++step) {
                __syncthreads();                       // the chunk before this one has been read
#pragma unroll
                for (int p = 0; p < KM_TR / 8; ++p) qs[(sr + 8 * p) * TK_LD + scol] = qv[p];
#pragma unroll
                for (int p = 0; p < KM_TC / 8; ++p) bs[(sr + 8 * p) * TK_LD + scol] = bv[p];
                __syncthreads();
                if (step + 1 < n_steps) load_step(step + 1);
                const float* qa = qs + fr * TK_LD + fk;
                const float* ba = bs + (wave * 32 + fr) * TK_LD + fk;
#pragma unroll
                for (int kk = 0; kk < TK_KC; kk += 2)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[kk], ba[kk], acc, 0, 0, 0);
            }
            // the metric's epilogue; C/D layout: column (centre) = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
            {
                const int c = wave * 32 + fr;
                const int bi = b0 + c;
                const float baux = bi < K ? c_aux[bi] : 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
                    float s = acc[r];
                    if (metric == SGNN_TOPK_COSINE) s = __fmul_rn(__fmul_rn(s, qaux_s[row]), baux);
                    else s = __fsub_rn(__fadd_rn(qaux_s[row], baux), __fmul_rn(2.0f, s));
                    sc[row * KM_TC + c] = s;
                    acc[r] = 0.0f;
                }
            }
            __syncthreads();
            // selection: the minimum key of this wave's eight rows over the tile's 128 centres (the next tile's barriers order
            // these reads before the next scores are written: D >= 1, so at least two lie between)
#pragma unroll
            for (int u = 0; u < KM_RPW; ++u) {
                const int qq = wave * KM_RPW + u;
                uint64_t m = TK_FILLER;
#pragma unroll
                for (int h = 0; h < KM_TC / 64; ++h) {
                    const int c = h * 64 + lane;
                    const int bi = b0 + c;
                    const uint64_t key = ((uint64_t)tk_order_key(sc[qq * KM_TC + c], lower_better) << 32) | (uint32_t)bi;
                    if (bi < K && key < m) m = key;
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) m = km_min_xor(m, off);
                if (m < best[u]) best[u] = m;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < KM_RPW; ++u) best_s[wave * KM_RPW + u] = best[u];
        }
        __syncthreads();
        if (wave == 0) {
            const int r = lane & 31;
            const int qi = q0 + r;
            const bool valid = lane < KM_TR && qi < N;
            const uint64_t key = best_s[r];            // K >= 1: a centre, never the filler
            const int a = (int)(uint32_t)key;
            const float s = tk_key_score((uint32_t)(key >> 32), lower_better);
            bool ch = false;
            if (valid) {
                ch = prev == nullptr || prev[qi] != a;
                assign[qi] = a;
                score[qi] = s;
            }
            changed += __popcll(__ballot(ch));
            double v = valid ? (double)s : 0.0;
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off, 32);
            inertia += v;
        }
        // (best_s and qaux_s are written again only after the next tile's chunk barriers / this barrier's successors)
        __syncthreads();
    }
    if (tid == 0) {
        ws_inertia[slot] = inertia;
        ws_changed[slot] = changed;
    }

    // ------------------------------------------------------------------ accumulation -------
    __threadfence_block();                             // this workgroup's assign[] is read back below
    __syncthreads();
    float* const accs = (float*)lds;
    float* const xs = (float*)(lds + KM_ACC_BYTES);
    int* const as_s = (int*)(xs + KM_RB * 32);
    int* const cnt_s = as_s + KM_RB;
    const int W = 1 << log_w, G = KM_THREADS >> log_w;
    const int col = tid & (W - 1), g = tid >> log_w;
    const int KW = K << log_w;
    for (int k = tid; k < K; k += KM_THREADS) cnt_s[k] = 0;
    for (int c0 = 0; c0 < D; c0 += W) {
        for (int e = tid; e < KW; e += KM_THREADS) accs[e] = 0.0f;
        __syncthreads();
        for (int rb = row_lo; rb < row_hi; rb += KM_RB) {
            const int nb = min(KM_RB, row_hi - rb);
            if (tid < KM_RB) as_s[tid] = tid < nb ? assign[rb + tid] : 0;
            for (int e = tid; e < (KM_RB << log_w); e += KM_THREADS) {
                const int r = e >> log_w, d = c0 + (e & (W - 1));
                xs[e] = (r < nb && d < D) ? x[(int64_t)(rb + r) * x_stride + d] : 0.0f;
            }
            __syncthreads();
            for (int r = 0; r < nb; ++r) {
                const int a = as_s[r];
                if ((a & (G - 1)) == g) {
                    const int e = (a << log_w) + col;
                    accs[e] = __fadd_rn(accs[e], xs[(r << log_w) + col]);
                    if (c0 == 0 && col == 0) cnt_s[a] += 1;
                }
            }
            __syncthreads();
        }
        for (int e = tid; e < KW; e += KM_THREADS) {
            const int k = e >> log_w, d = c0 + (e & (W - 1));
            if (d < D) ws_sums[((int64_t)slot * K + k) * D + d] = accs[e];
        }
        __syncthreads();
    }
    for (int k = tid; k < K; k += KM_THREADS) ws_counts[(int64_t)slot * K + k] = cnt_s[k];
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_finish_kernel(
    const double* __restrict__ ws_inertia, const float* __restrict__ ws_sums, const int32_t* __restrict__ ws_counts,
    const int32_t* __restrict__ ws_changed, int S, int K, int D, int metric, const float* cen, int64_t c_stride,
    float* __restrict__ sums, int32_t* __restrict__ counts, double* __restrict__ inertia, int32_t* __restrict__ empty,
    float* c_next, float* __restrict__ c_aux_next, int32_t* __restrict__ changed_out, int64_t it)
{
    __shared__ float red[KM_THREADS];
    __shared__ int n_s, e_s;
    const int tid = threadIdx.x, k = blockIdx.x;
    if (tid == 0) { n_s = 0; e_s = 0; }
    __syncthreads();
    int n = 0;
    for (int s = tid; s < S; s += KM_THREADS) n += ws_counts[(int64_t)s * K + k];
    if (n != 0) atomicAdd(&n_s, n);                    // integers in LDS: order-free
    __syncthreads();
    n = n_s;
    const float fn = (float)n;
    float q = 0.0f;
    for (int d = tid; d < D; d += KM_THREADS) {
        float acc = 0.0f;
        for (int s = 0; s < S; ++s) acc = __fadd_rn(acc, ws_sums[((int64_t)s * K + k) * D + d]);
        sums[(int64_t)k * D + d] = acc;
        const float v = n > 0 ? __fdiv_rn(acc, fn) : cen[(int64_t)k * c_stride + d];
        c_next[(int64_t)k * D + d] = v;
        q = fmaf(v, v, q);
    }
    red[tid] = q;
    __syncthreads();
    for (int off = KM_THREADS / 2; off >= 1; off >>= 1) {
        if (tid < off) red[tid] = __fadd_rn(red[tid], red[tid + off]);
        __syncthreads();
    }
    if (tid == 0) {
        counts[k] = n;
        const float sq = red[0];
        c_aux_next[k] = metric == SGNN_TOPK_COSINE ? __fdiv_rn(1.0f, __fsqrt_rn(fmaxf(sq, 1e-30f))) : sq;
    }
    if (k != 0) return;                                // whole workgroups leave
    int e = 0;
    for (int kk = tid; kk < K; kk += KM_THREADS) {
        int m = 0;
        for (int s = 0; s < S; ++s) m += ws_counts[(int64_t)s * K + kk];
        e += m == 0;
    }
    if (e != 0) atomicAdd(&e_s, e);
    __syncthreads();
    if (tid == 0) {
        double in = 0.0;
        int ch = 0;
        for (int s = 0; s < S; ++s) { in += ws_inertia[s]; ch += ws_changed[s]; }
        *inertia = in;
        *empty = e_s;
        changed_out[it] = ch;
    }
}

// slots: as many as there are 32-row tiles, up to KM_MAX_SLOTS and up to KM_PART_CAP bytes of K x D partials; none empty
static bool km_geometry(int64_t N, int64_t K, int64_t D, int64_t* n_tiles, int64_t* per, int64_t* S, int* log_w) {
    if (N < 1 || N > TK_MAX_ROWS || K < 1 || K > KM_MAX_K || D < 1 || D >= TK_MAX_STRIDE) return false;
    const int64_t nt = (N + KM_TR - 1) / KM_TR;
    int64_t s = KM_PART_CAP / (K * D * (int64_t)sizeof(float));
    if (s > KM_MAX_SLOTS) s = KM_MAX_SLOTS;
    if (s > nt) s = nt;
    if (s < 1) s = 1;
    const int64_t p = (nt + s - 1) / s;
    *n_tiles = nt; *per = p; *S = (nt + p - 1) / p;
    *log_w = K * 32 * (int64_t)sizeof(float) <= KM_ACC_BYTES ? 5 : (K * 16 * (int64_t)sizeof(float) <= KM_ACC_BYTES ? 4 : 3);
    return true;
}

// workspace: [S] double inertia | [S][K][D] float sums | [S][K] int32 counts | [S] int32 changed
static int64_t km_ws_bytes(int64_t S, int64_t K, int64_t D) { return S * 8 + S * K * D * 4 + S * K * 4 + S * 4; }

extern "C" int64_t sgnn_kmeans_max_k(void) { return KM_MAX_K; }

extern "C" int64_t sgnn_kmeans_slots(int64_t N, int64_t K, int64_t D)
{
    int64_t nt, per, S; int lw;
    return km_geometry(N, K, D, &nt, &per, &S, &lw) ? S : (int64_t)SGNN_ERR_BAD_ARG;
}

extern "C" int64_t sgnn_kmeans_workspace_bytes(int64_t N, int64_t K, int64_t D)
{
    int64_t nt, per, S; int lw;
    return km_geometry(N, K, D, &nt, &per, &S, &lw) ? km_ws_bytes(S, K, D) : (int64_t)SGNN_ERR_BAD_ARG;
}

extern "C" int sgnn_kmeans_step(const float* x, int64_t x_stride, int64_t N, const float* c, int64_t c_stride, int64_t K,
                                int64_t D, int metric, const float* x_aux, const float* c_aux, const int32_t* prev_assign,
                                int32_t* assign, float* score, void* workspace, int64_t workspace_bytes, void* stream)
{
    int64_t nt, per, S; int lw;
    if (!km_geometry(N, K, D, &nt, &per, &S, &lw)) return SGNN_ERR_BAD_ARG;
    if (x == nullptr || c == nullptr || x_aux == nullptr || c_aux == nullptr || assign == nullptr || score == nullptr ||
        workspace == nullptr) return SGNN_ERR_BAD_ARG;
    if (metric != SGNN_TOPK_COSINE && metric != SGNN_TOPK_L2) return SGNN_ERR_BAD_ARG;
    if (x_stride < D || c_stride < D || x_stride >= TK_MAX_STRIDE || c_stride >= TK_MAX_STRIDE) return SGNN_ERR_BAD_ARG;
    if (workspace_bytes < km_ws_bytes(S, K, D)) return SGNN_ERR_BAD_ARG;
    char* w = (char*)workspace;
    double* ws_inertia = (double*)w;
    float* ws_sums = (float*)(w + S * 8);
    int32_t* ws_counts = (int32_t*)(w + S * 8 + S * K * D * 4);
    int32_t* ws_changed = ws_counts + S * K;
    hipLaunchKernelGGL(kmeans_step_kernel, dim3((unsigned)S), dim3(KM_THREADS), 0, (hipStream_t)stream, x, (uint32_t)x_stride,
                       (int)N, c, (uint32_t)c_stride, (int)K, (int)D, metric, x_aux, c_aux, prev_assign, (int)nt, (int)per, lw,
                       assign, score, ws_inertia, ws_sums, ws_counts, ws_changed);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_kmeans_finish(const void* workspace, int64_t workspace_bytes, int64_t N, int64_t K, int64_t D, int metric,
                                  const float* c, int64_t c_stride, float* sums, int32_t* counts, double* inertia,
                                  int32_t* empty, float* c_next, float* c_aux_next, int32_t* changed, int64_t it,
                                  void* stream)
{
    int64_t nt, per, S; int lw;
    if (!km_geometry(N, K, D, &nt, &per, &S, &lw)) return SGNN_ERR_BAD_ARG;
    if (workspace == nullptr || c == nullptr || sums == nullptr || counts == nullptr || inertia == nullptr ||
        empty == nullptr || c_next == nullptr || c_aux_next == nullptr || changed == nullptr || it < 0) return SGNN_ERR_BAD_ARG;
    if (metric != SGNN_TOPK_COSINE && metric != SGNN_TOPK_L2) return SGNN_ERR_BAD_ARG;
    if (c_stride < D || c_stride >= TK_MAX_STRIDE || workspace_bytes < km_ws_bytes(S, K, D)) return SGNN_ERR_BAD_ARG;
    const char* w = (const char*)workspace;
    const int32_t* ws_counts = (const int32_t*)(w + S * 8 + S * K * D * 4);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)K), dim3(KM_THREADS), 0, (hipStream_t)stream, (const double*)w,
                       (const float*)(w + S * 8), ws_counts, ws_counts + S * K, (int)S, (int)K, (int)D, metric, c, c_stride,
                       sums, counts, inertia, empty, c_next, c_aux_next, changed, it);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

SGNN_DEFINE_WARM(kmeans)

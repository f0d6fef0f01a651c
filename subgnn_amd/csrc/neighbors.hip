// libsubgnn_hip.so: nearest rows of a bank of embeddings (sgnn_topk_rows) -- scores on the fp32 MFMA, each query's running
// best k held on chip, nothing but the winners written.
//
//   topk_rows_kernel    one workgroup per (tile of 32 queries, slice of the bank).  Per tile of 128 bank rows it stages the
//                       query and bank tiles through LDS in chunks of 32 columns, zero-padded past D and past the last row, and
//                       each of the four waves forms one 32 x 32 score tile with v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain
//                       from 0, so a pair's score is defined bit for bit.  The scores go through the metric's epilogue into an
//                       LDS tile; then each wave serves eight queries.  A query's list is ONE 64-bit key per lane, ascending
//                       over the lanes (sixteen registers for the eight lists, every index static); a candidate is compared
//                       with the list's k-th key first, so most tiles cost one compare per score, and a survivor enters with
//                       one compare per lane and a one-lane shift.
//   topk_merge_kernel   one wave per query merges the slices' lists (each ascending) under the same order.
//
// The key is (order key of the score << 32) | bank row: smaller = better.  The order key is the usual monotone map of the float's
// bits (complemented where a higher score is better), NaN = 0xFFFFFFFE behind every number, filler = all ones behind everything.
// Keys are distinct (the row is in them), so the order is strict and total and the result cannot depend on tiles, slices or the
// order of insertions.  The score is read back out of the key: a zero comes back as +0, a NaN as the quiet NaN 0x7FC00000.
#include "common.h"
#include "topk_order.h"
#include <math.h>

#define TK_MAX_K      64
#define TK_TQ         32          // queries per workgroup
#define TK_TB         128         // bank rows per tile: one 32-row sub-tile per wave
#define TK_THREADS    256
#define TK_QPW        (TK_TQ / (TK_THREADS / 64))   // queries per wave in the selection
#define TK_MAX_SPLITS 1024
#define TK_WANT_BLOCKS 1024       // four workgroups per CU
// (the staged-chunk geometry, the limits, the order key and its inverse: topk_order.h, shared with kmeans.hip)

__device__ __forceinline__ uint64_t tk_readlane(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// the list (ascending over the lanes) with c entered at its rank; the last lane's key drops out
__device__ __forceinline__ uint64_t tk_insert(uint64_t mine, uint64_t c, int lane) {
    const uint32_t plo = (uint32_t)__shfl_up((int)(uint32_t)mine, 1);
    const uint32_t phi = (uint32_t)__shfl_up((int)(uint32_t)(mine >> 32), 1);
    const uint64_t prev = ((uint64_t)phi << 32) | plo;
    if (mine < c) return mine;
    return (lane == 0 || prev < c) ? c : prev;
}

__device__ __forceinline__ void tk_write_row(uint64_t key, int lane, int k, bool lower_better, float* out_score, int64_t* out_index) {
    if (lane < k) {
        const uint32_t idx = (uint32_t)key;
        out_score[lane] = tk_key_score((uint32_t)(key >> 32), lower_better);
        out_index[lane] = key == TK_FILLER ? (int64_t)-1 : (int64_t)idx;
    }
}

__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(
    const float* __restrict__ q, uint32_t q_stride, int Q, const float* __restrict__ bank, uint32_t b_stride, int N, int D,
    int k, int metric, const float* __restrict__ q_aux, const float* __restrict__ b_aux, const int64_t* __restrict__ exclude,
    int n_tiles, int tiles_per_split, int splits, uint64_t* __restrict__ ws, float* __restrict__ out_score,
    int64_t* __restrict__ out_index)
{
    __shared__ float qs[TK_TQ * TK_LD];
    __shared__ float bs[TK_TB * TK_LD];
    __shared__ float sc[TK_TQ * TK_TB];
    __shared__ float qaux_s[TK_TQ];
    __shared__ uint32_t ex_s[TK_TQ];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = (int)blockIdx.x * TK_TQ;            // < Q
    const int split = blockIdx.y;
    const bool lower_better = metric == SGNN_TOPK_L2;
    const int tile_lo = min(split * tiles_per_split, n_tiles), tile_hi = min(tile_lo + tiles_per_split, n_tiles);

    if (tid < TK_TQ) {
        const int qi = q0 + tid;
        qaux_s[tid] = (q_aux != nullptr && qi < Q) ? q_aux[qi] : 0.0f;
        const int64_t e = (exclude != nullptr && qi < Q) ? exclude[qi] : (int64_t)-1;
        ex_s[tid] = (e >= 0 && e < N) ? (uint32_t)e : 0xFFFFFFFFu;
    }

    uint64_t list[TK_QPW];
#pragma unroll
    for (int u = 0; u < TK_QPW; ++u) list[u] = TK_FILLER;

    const int sr = tid >> 5, scol = tid & 31;          // staging: 8 rows x 32 columns per pass
    const int fr = lane & 31, fk = lane >> 5;          // MFMA operands: row (query or bank) and k of the pair

    // One step = one chunk of 32 columns of one tile.  The next step's elements are loaded into registers ahead of this step's
    // MFMAs, so their latency is spent under the matrix work.  Every load is issued, from an address clamped into the matrix
    // (a wave-uniform 64-bit tile base plus a 32-bit offset per lane: the host refuses row strides of 2^23 elements and more),
    // and what lies past D or past the last row is replaced by zero afterwards: no branch around any load.
    const int n_chunks = (D + TK_KC - 1) / TK_KC;
    float qv[TK_TQ / 8], bv[TK_TB / 8];
    const float* const qt = q + (int64_t)q0 * q_stride;
    const int q_last = Q - 1 - q0;                     // >= 0
    auto load_step = [&](int tile, int chunk) {
        const int d = chunk * TK_KC + scol, b0 = tile * TK_TB;
        const bool d_in = d < D;
        const uint32_t dc = d_in ? (uint32_t)d : 0u;
        const float* const bt = bank + (int64_t)b0 * b_stride;
        const int b_last = N - 1 - b0;                 // >= 0: the tile exists
#pragma unroll
        for (int p = 0; p < TK_TQ / 8; ++p) {
            const int r = sr + 8 * p;
            const float v = qt[(uint32_t)min(r, q_last) * q_stride + dc];
            qv[p] = (d_in && r <= q_last) ? v : 0.0f;
        }
#pragma unroll
        for (int p = 0; p < TK_TB / 8; ++p) {
            const int r = sr + 8 * p;
            const float v = bt[(uint32_t)min(r, b_last) * b_stride + dc];
            bv[p] = (d_in && r <= b_last) ? v : 0.0f;
        }
    };
    tk_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    if (tile_lo < tile_hi) load_step(tile_lo, 0);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        const int b0 = tile * TK_TB;
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            __syncthreads();                           // the chunk before this one has been read
#pragma unroll
            for (int p = 0; p < TK_TQ / 8; ++p) qs[(sr + 8 * p) * TK_LD + scol] = qv[p];
#pragma unroll
            for (int p = 0; p < TK_TB / 8; ++p) bs[(sr + 8 * p) * TK_LD + scol] = bv[p];
            __syncthreads();
            if (chunk + 1 < n_chunks) load_step(tile, chunk + 1);
            else if (tile + 1 < tile_hi) load_step(tile + 1, 0);
            const float* qa = qs + fr * TK_LD + fk;
            const float* ba = bs + (wave * 32 + fr) * TK_LD + fk;
#pragma unroll
            for (int kk = 0; kk < TK_KC; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[kk], ba[kk], acc, 0, 0, 0);
        }
        // the metric's epilogue; C/D layout: column (bank row) = lane & 31, row (query) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        {
            const int c = wave * 32 + fr;
            const int bi = b0 + c;
            const float baux = (b_aux != nullptr && bi < N) ? b_aux[bi] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
                float s = acc[r];
                if (metric == SGNN_TOPK_COSINE) s = __fmul_rn(__fmul_rn(s, qaux_s[row]), baux);
                else if (metric == SGNN_TOPK_L2) s = __fsub_rn(__fadd_rn(qaux_s[row], baux), __fmul_rn(2.0f, s));
                sc[row * TK_TB + c] = s;
                acc[r] = 0.0f;
            }
        }
        __syncthreads();
        // selection: this wave's eight queries against the tile's 128 scores (the next tile's first barrier orders these
        // reads before the next scores are written: D >= 1, so at least two barriers lie between)
#pragma unroll
        for (int u = 0; u < TK_QPW; ++u) {
            const int qq = wave * TK_QPW + u;
            const uint32_t ex = ex_s[qq];
#pragma unroll
            for (int h = 0; h < TK_TB / 64; ++h) {
                const int c = h * 64 + lane;
                const int bi = b0 + c;
                const uint64_t key = ((uint64_t)tk_order_key(sc[qq * TK_TB + c], lower_better) << 32) | (uint32_t)bi;
                const uint64_t thr = tk_readlane(list[u], k - 1);
                unsigned long long mask = __ballot(bi < N && (uint32_t)bi != ex && key < thr);
                while (mask != 0ull) {                 // (a survivor of the old k-th key that the new one beats lands beyond k)
                    const int src = __ffsll((long long)mask) - 1;
                    mask &= mask - 1ull;
                    list[u] = tk_insert(list[u], tk_readlane(key, src), lane);
                }
            }
        }
    }

#pragma unroll
    for (int u = 0; u < TK_QPW; ++u) {
        const int64_t qi = q0 + wave * TK_QPW + u;
        if (qi >= Q) continue;
        if (splits == 1) tk_write_row(list[u], lane, k, lower_better, out_score + qi * k, out_index + qi * k);
        else if (lane < k) ws[(qi * splits + split) * k + lane] = list[u];
    }
}

__global__ __launch_bounds__(TK_THREADS) void topk_merge_kernel(const uint64_t* __restrict__ ws, int64_t Q, int k, int metric,
                                                               int splits, float* __restrict__ out_score,
                                                               int64_t* __restrict__ out_index)
{
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * (TK_THREADS / 64) + (threadIdx.x >> 6);
    if (qi >= Q) return;                               // whole waves leave; no barrier follows
    uint64_t list = TK_FILLER, thr = TK_FILLER;
    for (int s = 0; s < splits; ++s) {
        const uint64_t key = lane < k ? ws[(qi * splits + s) * k + lane] : TK_FILLER;
        for (int i = 0; i < k; ++i) {                  // the slice's list is ascending: the first key that fails ends it
            const uint64_t c = tk_readlane(key, i);
            if (c >= thr) break;
            list = tk_insert(list, c, lane);
            thr = tk_readlane(list, k - 1);
        }
    }
    tk_write_row(list, lane, k, metric == SGNN_TOPK_L2, out_score + qi * k, out_index + qi * k);
}

// slices of the bank: as many as fill the chip at four workgroups per CU, none of them empty; a caller's count is taken as given
static void tk_geometry(int64_t Q, int64_t N, int64_t splits, int64_t* n_tiles, int64_t* tiles_per_split, int64_t* S) {
    const int64_t nq = (Q + TK_TQ - 1) / TK_TQ;
    const int64_t nt = (N + TK_TB - 1) / TK_TB;
    int64_t s = splits, per;
    if (s <= 0) {
        s = (TK_WANT_BLOCKS + nq - 1) / nq;
        if (s > nt) s = nt;
        if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
        if (s < 1) s = 1;
        per = (nt + s - 1) / s;
        if (per < 1) per = 1;
        s = (nt + per - 1) / per;
        if (s < 1) s = 1;
    } else {
        per = (nt + s - 1) / s;
        if (per < 1) per = 1;
    }
    *n_tiles = nt; *tiles_per_split = per; *S = s;
}

extern "C" int64_t sgnn_topk_max_k(void) { return TK_MAX_K; }

extern "C" int64_t sgnn_topk_rows_workspace_bytes(int64_t Q, int64_t N, int64_t k, int64_t splits)
{
    if (Q < 1 || N < 0 || k < 1 || k > TK_MAX_K || splits < 0 || splits > TK_MAX_SPLITS) return SGNN_ERR_BAD_ARG;
    int64_t nt, per, S;
    tk_geometry(Q, N, splits, &nt, &per, &S);
    return S == 1 ? 0 : Q * S * k * (int64_t)sizeof(uint64_t);
}

extern "C" int sgnn_topk_rows(const float* q, int64_t q_stride, int64_t Q, const float* bank, int64_t b_stride, int64_t N,
                              int64_t D, int64_t k, int metric, const float* q_aux, const float* b_aux, const int64_t* exclude,
                              int64_t splits, float* out_score, int64_t* out_index, void* workspace, int64_t workspace_bytes,
                              void* stream)
{
    if (q == nullptr || out_score == nullptr || out_index == nullptr || Q < 1 || D < 1 || N < 0 || N > TK_MAX_ROWS ||
        Q > TK_MAX_ROWS) return SGNN_ERR_BAD_ARG;
    if ((N > 0 && bank == nullptr) || q_stride < D || (N > 0 && b_stride < D) ||
        q_stride >= TK_MAX_STRIDE || b_stride >= TK_MAX_STRIDE) return SGNN_ERR_BAD_ARG;
    if (k < 1 || k > TK_MAX_K || splits < 0 || splits > TK_MAX_SPLITS) return SGNN_ERR_BAD_ARG;
    if (metric != SGNN_TOPK_DOT && metric != SGNN_TOPK_COSINE && metric != SGNN_TOPK_L2) return SGNN_ERR_BAD_ARG;
    if (metric != SGNN_TOPK_DOT && (q_aux == nullptr || (N > 0 && b_aux == nullptr))) return SGNN_ERR_BAD_ARG;
    int64_t nt, per, S;
    tk_geometry(Q, N, splits, &nt, &per, &S);
    const int64_t need = S == 1 ? 0 : Q * S * k * (int64_t)sizeof(uint64_t);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return SGNN_ERR_BAD_ARG;
    const dim3 grid((unsigned)((Q + TK_TQ - 1) / TK_TQ), (unsigned)S);
    hipLaunchKernelGGL(topk_rows_kernel, grid, dim3(TK_THREADS), 0, (hipStream_t)stream, q, (uint32_t)q_stride, (int)Q, bank,
                       (uint32_t)b_stride, (int)N, (int)D, (int)k, metric, q_aux, b_aux, exclude, (int)nt, (int)per, (int)S,
                       (uint64_t*)workspace, out_score, out_index);
    SGNN_CHECK_LAUNCH();
    if (S > 1) {
        const int per_block = TK_THREADS / 64;
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((Q + per_block - 1) / per_block)), dim3(TK_THREADS), 0,
                           (hipStream_t)stream, (const uint64_t*)workspace, Q, (int)k, metric, (int)S, out_score, out_index);
        SGNN_CHECK_LAUNCH();
    }
    return SGNN_OK;
}

SGNN_DEFINE_WARM(neighbors)

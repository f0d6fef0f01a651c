// Node-embedding pre-training on the whole graph: the GPU counterpart of the reference's prepare_dataset/train_node_emb.py +
// model.py (TrainNet: two GINConv / GCNConv layers over one-hot features, link prediction on dot products, utils.py:22-56).
//
//   sgnn_ne_aggregate   out[v] = a_self[v] X[v] + sum_{e in row v} w[e] X[col[e]] (+ bias), optional relu -> dropout epilogue.
//                       One wavefront per destination row, 16-byte row loads; rows longer than NE_CHUNK entries are cut into
//                       chunks summed by separate wavefronts into partials, which a second launch adds in chunk order (the
//                       split of cdna_hip_programming.md Appendix B "Scatter / gather / embedding": the transpose of the
//                       reference-direction message graph has hub rows thousands of entries long).  No atomics: every output
//                       row has one owner, every sum a fixed order -- bit-reproducible.
//   sgnn_ne_negatives   uniform (u, v) id pairs from the draw tape, rejecting u == v and pairs that are edges (binary search in
//                       the sorted adjacency row of u).
//   sgnn_ne_link_loss   per scored pair: dot, s = sigmoid(dot), the reference's two-class nll(log_softmax(stack(1 - s, s))) term
//                       and its derivative w.r.t. the dot; the mean loss by per-block partials added in a fixed order.
//   sgnn_ne_relu_drop_bwd  the gradient through relu -> dropout from the layer's stored OUTPUT: an element passed both iff it is
//                       positive (the scale is > 1), so neither the mask nor the pre-activation is kept.
#include "common.h"

#define NE_CHUNK 512            // entries per wavefront before a row is split (the guide's measured chunk)
#define NE_WAVES 4              // wavefronts per workgroup

// lanes of one wavefront cover one row of F4 = F / 4 float4 columns with L lanes (L = 8 .. 64, a power of two) and C float4s
// per lane; the 64 / L lane groups of the wavefront take different entries of the row and are added at the end
template <int L, int C>
__device__ __forceinline__ void ne_row_sum(const int32_t* __restrict__ col, const float* __restrict__ w, const float4* __restrict__ X,
                                           int64_t beg, int64_t end, int64_t F4, int lane, float4 (&acc)[C])
{
    constexpr int G = 64 / L;
    const int g = lane / L, li = lane % L;
#pragma unroll
    for (int k = 0; k < C; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t e = beg + g;
    for (; e + 3 * G < end; e += 4 * G) {                    // four rows in flight per lane group
        int32_t c[4];
        float ww[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c[u] = col[e + u * G];
            ww[u] = w ? w[e + u * G] : 1.f;
        }
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int64_t cc = li + k * L;
            if (cc < F4) {
                float4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = X[(int64_t)c[u] * F4 + cc];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc[k].x += ww[u] * x[u].x; acc[k].y += ww[u] * x[u].y;
                    acc[k].z += ww[u] * x[u].z; acc[k].w += ww[u] * x[u].w;
                }
            }
        }
    }
    for (; e < end; e += G) {
        const int32_t c = col[e];
        const float ww = w ? w[e] : 1.f;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int64_t cc = li + k * L;
            if (cc < F4) {
                const float4 x = X[(int64_t)c * F4 + cc];
                acc[k].x += ww * x.x; acc[k].y += ww * x.y; acc[k].z += ww * x.z; acc[k].w += ww * x.w;
            }
        }
    }
    // lane groups -> group 0, always in the same order
#pragma unroll
    for (int off = L; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            acc[k].x += __shfl_xor(acc[k].x, off);
            acc[k].y += __shfl_xor(acc[k].y, off);
            acc[k].z += __shfl_xor(acc[k].z, off);
            acc[k].w += __shfl_xor(acc[k].w, off);
        }
    }
}

struct ne_epilogue {
    const float* a_self;        // nullable: 1
    const float* bias;          // nullable
    int relu;
    uint32_t drop_thr;          // 0: no dropout; else element (v, f) kept iff (draw64(seed, stream, v, f) >> 32) >= drop_thr
    float drop_scale;           // 1 / (1 - p)
    uint64_t h0;                // sgnn_tape_h0(seed, stream)
};

// out row v (group-0 lanes) = acc + a_self[v] X[v] + bias, then relu, then dropout
template <int L, int C>
__device__ __forceinline__ void ne_finish_row(const float4* __restrict__ X, int64_t v, int64_t F4, int lane, const float4 (&acc)[C],
                                              const ne_epilogue& ep, float4* __restrict__ out)
{
    if (lane >= L) return;
    const float a = ep.a_self ? ep.a_self[v] : 1.f;
    const uint64_t h1 = ep.drop_thr ? sgnn_tape_h1(ep.h0, (uint64_t)v) : 0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int64_t cc = lane + k * L;
        if (cc >= F4) continue;
        const float4 xs = X[v * F4 + cc];
        float4 y = acc[k];
        y.x += a * xs.x; y.y += a * xs.y; y.z += a * xs.z; y.w += a * xs.w;
        if (ep.bias) {
            const float4 b = reinterpret_cast<const float4*>(ep.bias)[cc];
            y.x += b.x; y.y += b.y; y.z += b.z; y.w += b.w;
        }
        float* Y = &y.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float t = Y[q];
            if (ep.relu) t = fmaxf(t, 0.f);
            if (ep.drop_thr) {
                const uint32_t u = (uint32_t)(sgnn_tape_draw(h1, (uint64_t)(cc * 4 + q)) >> 32);
                t = u >= ep.drop_thr ? t * ep.drop_scale : 0.f;
            }
            Y[q] = t;
        }
        out[v * F4 + cc] = y;
    }
}

// items [0, n_rows): row v = item, finished here unless it is longer than NE_CHUNK; items [n_rows, n_rows + n_chunks): chunk c of a
// long row (chunk_row[c], entries chunk_beg[c] .. +NE_CHUNK) -> partial[c]
template <int L, int C>
__global__ __launch_bounds__(64 * NE_WAVES) void ne_aggregate_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                     const float* __restrict__ w, const float4* __restrict__ X,
                                                                     int64_t n_rows, int64_t F4, const int32_t* __restrict__ chunk_row,
                                                                     const int64_t* __restrict__ chunk_beg, int64_t n_chunks,
                                                                     ne_epilogue ep, float4* __restrict__ out, float4* __restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * NE_WAVES + (threadIdx.x >> 6);
    float4 acc[C];
    if (item < n_rows) {
        const int64_t beg = rowptr[item], end = rowptr[item + 1];
        if (end - beg > NE_CHUNK) return;                                  // the chunk items and the finish launch own it
        ne_row_sum<L, C>(col, w, X, beg, end, F4, lane, acc);
        ne_finish_row<L, C>(X, item, F4, lane, acc, ep, out);
    } else if (item < n_rows + n_chunks) {
        const int64_t c = item - n_rows;
        const int64_t v = chunk_row[c], beg = chunk_beg[c];
        const int64_t end = min(beg + (int64_t)NE_CHUNK, rowptr[v + 1]);
        ne_row_sum<L, C>(col, w, X, beg, end, F4, lane, acc);
        if (lane < L) {
#pragma unroll
            for (int k = 0; k < C; ++k)
                if (lane + k * L < F4) partial[c * F4 + lane + k * L] = acc[k];
        }
    }
}

// one wavefront per long row: its chunk partials chunk_first[r] .. chunk_first[r + 1] in chunk order, then the epilogue
template <int L, int C>
__global__ __launch_bounds__(64 * NE_WAVES) void ne_aggregate_finish_kernel(const int32_t* __restrict__ long_rows,
                                                                            const int64_t* __restrict__ chunk_first, int64_t n_long,
                                                                            const float4* __restrict__ X, int64_t F4,
                                                                            const float4* __restrict__ partial, ne_epilogue ep,
                                                                            float4* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * NE_WAVES + (threadIdx.x >> 6);
    if (r >= n_long || lane >= L) return;
    float4 acc[C];
#pragma unroll
    for (int k = 0; k < C; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t c = chunk_first[r]; c < chunk_first[r + 1]; ++c) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int64_t cc = lane + k * L;
            if (cc < F4) {
                const float4 p = partial[c * F4 + cc];
                acc[k].x += p.x; acc[k].y += p.y; acc[k].z += p.z; acc[k].w += p.w;
            }
        }
    }
    ne_finish_row<L, C>(X, long_rows[r], F4, lane, acc, ep, out);
}

template <int L, int C>
static int ne_aggregate_run(const int64_t* rowptr, const int32_t* col, const float* w, const float* X, int64_t n_rows, int64_t F4,
                            const int32_t* chunk_row, const int64_t* chunk_beg, int64_t n_chunks, const int32_t* long_rows,
                            const int64_t* chunk_first, int64_t n_long, const ne_epilogue& ep, float* out, float* partial,
                            hipStream_t st)
{
    const int64_t items = n_rows + n_chunks;
    hipLaunchKernelGGL((ne_aggregate_kernel<L, C>), dim3((unsigned)((items + NE_WAVES - 1) / NE_WAVES)), dim3(64 * NE_WAVES), 0, st,
                       rowptr, col, w, (const float4*)X, n_rows, F4, chunk_row, chunk_beg, n_chunks, ep, (float4*)out,
                       (float4*)partial);
    SGNN_CHECK_LAUNCH();
    if (n_long > 0) {
        hipLaunchKernelGGL((ne_aggregate_finish_kernel<L, C>), dim3((unsigned)((n_long + NE_WAVES - 1) / NE_WAVES)),
                           dim3(64 * NE_WAVES), 0, st, long_rows, chunk_first, n_long, (const float4*)X, F4,
                           (const float4*)partial, ep, (float4*)out);
        SGNN_CHECK_LAUNCH();
    }
    return SGNN_OK;
}

extern "C" int64_t sgnn_ne_chunk_entries(void) { return NE_CHUNK; }

extern "C" int sgnn_ne_aggregate(const int64_t* rowptr, const int32_t* col, const float* w, const float* a_self, const float* X,
                                 const float* bias, int64_t n_rows, int64_t F, const int32_t* chunk_row, const int64_t* chunk_beg,
                                 int64_t n_chunks, const int32_t* long_rows, const int64_t* chunk_first, int64_t n_long,
                                 int relu, uint32_t drop_thr, float drop_scale, uint64_t seed, uint64_t stream_id, float* out,
                                 float* partial, void* stream)
{
    if (!rowptr || !X || !out || n_rows < 0 || n_chunks < 0 || n_long < 0 || (!col && n_rows > 0)) return SGNN_ERR_BAD_ARG;
    if ((n_chunks > 0 && (!chunk_row || !chunk_beg || !partial)) || (n_long > 0 && (!long_rows || !chunk_first)))
        return SGNN_ERR_BAD_ARG;
    if (F <= 0 || F % 4 != 0 || F > 512) return SGNN_ERR_UNSUPPORTED_D;
    if ((((uintptr_t)X | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)partial) & 15) != 0) return SGNN_ERR_BAD_ARG;
    if (n_rows == 0) return SGNN_OK;
    const ne_epilogue ep{a_self, bias, relu, drop_thr, drop_scale, sgnn_tape_h0(seed, stream_id)};
    const int64_t F4 = F / 4;
    hipStream_t st = (hipStream_t)stream;
#define NE_AGG(L, C) ne_aggregate_run<L, C>(rowptr, col, w, X, n_rows, F4, chunk_row, chunk_beg, n_chunks, long_rows, chunk_first, \
                                            n_long, ep, out, partial, st)
    if (F4 <= 8) return NE_AGG(8, 1);
    if (F4 <= 16) return NE_AGG(16, 1);
    if (F4 <= 32) return NE_AGG(32, 1);
    if (F4 <= 64) return NE_AGG(64, 1);
    return NE_AGG(64, 2);
#undef NE_AGG
}

// ---- gradient through relu -> dropout from the stored output --------------------------------------------------------------
__global__ __launch_bounds__(256) void ne_relu_drop_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ h,
                                                               float4* __restrict__ dst, int64_t n4, float scale)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 gg = g[i];
        const float4 hh = h[i];
        gg.x = hh.x > 0.f ? gg.x * scale : 0.f;
        gg.y = hh.y > 0.f ? gg.y * scale : 0.f;
        gg.z = hh.z > 0.f ? gg.z * scale : 0.f;
        gg.w = hh.w > 0.f ? gg.w * scale : 0.f;
        dst[i] = gg;
    }
}

extern "C" int sgnn_ne_relu_drop_bwd(const float* grad, const float* out, float* dst, int64_t n, float scale, void* stream)
{
    if (!grad || !out || !dst || n < 0 || n % 4 != 0) return SGNN_ERR_BAD_ARG;
    if ((((uintptr_t)grad | (uintptr_t)out | (uintptr_t)dst) & 15) != 0) return SGNN_ERR_BAD_ARG;
    if (n == 0) return SGNN_OK;
    hipLaunchKernelGGL(ne_relu_drop_bwd_kernel, dim3(sgnn_grid_for(n / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)grad, (const float4*)out, (float4*)dst, n / 4, scale);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

// ---- negative pairs ---------------------------------------------------------------------------------------------------------
// pair i, attempt a: d = draw64(seed, stream, item_base + i, a); u = 1 + ((d >> 32) * n_ids >> 32), v = 1 + ((d & 0xffffffff) *
// n_ids >> 32); the first attempt with u != v and v not in u's sorted adjacency row is taken; none of max_attempts: (0, 0)
__global__ __launch_bounds__(256) void ne_negatives_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col_sorted,
                                                           int64_t n_ids, int64_t n, uint64_t h0, int64_t item_base, int max_attempts,
                                                           int32_t* __restrict__ u_out, int32_t* __restrict__ v_out)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t h1 = sgnn_tape_h1(h0, (uint64_t)(item_base + i));
    int32_t ru = 0, rv = 0;
    for (int a = 0; a < max_attempts; ++a) {
        const uint64_t d = sgnn_tape_draw(h1, (uint64_t)a);
        const int32_t u = 1 + (int32_t)(((d >> 32) * (uint64_t)n_ids) >> 32);
        const int32_t v = 1 + (int32_t)(((d & 0xffffffffull) * (uint64_t)n_ids) >> 32);
        if (u == v) continue;
        const int64_t b = rowptr[u];
        if (sgnn_sorted_contains(col_sorted + b, (int32_t)(rowptr[u + 1] - b), v)) continue;
        ru = u; rv = v;
        break;
    }
    u_out[i] = ru;
    v_out[i] = rv;
}

extern "C" int sgnn_ne_negatives(const int64_t* rowptr, const int32_t* col_sorted, int64_t n_ids, int64_t n, uint64_t seed,
                                 uint64_t stream_id, int64_t item_base, int max_attempts, int32_t* u_out, int32_t* v_out, void* stream)
{
    if (!rowptr || !col_sorted || !u_out || !v_out || n < 0 || n_ids < 1 || n_ids >= (1ll << 31) - 1 || item_base < 0
        || max_attempts < 1) return SGNN_ERR_BAD_ARG;
    if (n == 0) return SGNN_OK;
    hipLaunchKernelGGL(ne_negatives_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col_sorted,
                       n_ids, n, sgnn_tape_h0(seed, stream_id), item_base, max_attempts, u_out, v_out);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

// ---- link loss ----------------------------------------------------------------------------------------------------------------
// pairs [0, n_pos) have label 1, the rest label 0.  s = sigmoid(z_u . z_v); the reference's term is -log_softmax(1 - s, s)[y]
// = lse - x_y with lse = log(e^(1-s) + e^s); d term / d s = 2 (q - y), q = sigmoid(2 s - 1); d / d dot = that * s (1 - s), with
// 1 - s taken as sigmoid(-dot): 1.f - s keeps only an absolute ulp of 1 (no digit at all once s rounds to 1, dot above ~17).
// grad[p] = inv_n * d term / d dot; loss = inv_n * sum of the terms (block partials in double, added in block order).
#define NE_LOSS_BLOCKS_MAX 4096
template <int L, int C>
__global__ __launch_bounds__(64 * NE_WAVES) void ne_link_loss_kernel(const float4* __restrict__ Z, int64_t F4, const int32_t* __restrict__ pu,
                                                                     const int32_t* __restrict__ pv, int64_t n_pairs, int64_t n_pos,
                                                                     double inv_n, float* __restrict__ s_out, float* __restrict__ g_out,
                                                                     double* __restrict__ partial)
{
    constexpr int G = 64 / L;
    constexpr int PER_BLOCK = NE_WAVES * G;
    __shared__ double terms[PER_BLOCK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / L, li = lane % L;
    double blk = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * PER_BLOCK; base < n_pairs; base += (int64_t)gridDim.x * PER_BLOCK) {
        const int64_t p = base + wave * G + g;
        float d = 0.f;
        if (p < n_pairs) {
            const int64_t u = pu[p], v = pv[p];
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const int64_t cc = li + k * L;
                if (cc < F4) {
                    const float4 a = Z[u * F4 + cc], b = Z[v * F4 + cc];
                    d += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
                }
            }
        }
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1) d += __shfl_xor(d, off);
        double term = 0.0;
        if (p < n_pairs && li == 0) {
            const float s = 1.f / (1.f + expf(-d)), sn = 1.f / (1.f + expf(d));      // sigmoid(d), sigmoid(-d) = 1 - s
            const float y = p < n_pos ? 1.f : 0.f;
            const float q = 1.f / (1.f + expf(1.f - 2.f * s));
            const float m = fmaxf(s, 1.f - s);
            const float lse = m + log1pf(expf(-fabsf(2.f * s - 1.f)));
            term = (double)(lse - (p < n_pos ? s : 1.f - s));
            s_out[p] = s;
            if (g_out) g_out[p] = (float)(inv_n * (double)(2.f * (q - y) * s * sn));
        }
        if (li == 0) terms[wave * G + g] = term;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int t = 0; t < PER_BLOCK; ++t) blk += terms[t];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = blk;
}

__global__ __launch_bounds__(256) void ne_loss_finish_kernel(const double* __restrict__ partial, int n_blocks, double inv_n,
                                                             float* __restrict__ loss)
{
    __shared__ double s[256];
    double a = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += 256) a += partial[b];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(s[0] * inv_n);
}

extern "C" int64_t sgnn_ne_link_loss_workspace_bytes(void) { return NE_LOSS_BLOCKS_MAX * (int64_t)sizeof(double); }

template <int L, int C>
static int ne_link_loss_run(const float* Z, int64_t F4, const int32_t* pu, const int32_t* pv, int64_t n_pairs, int64_t n_pos,
                            float* s_out, float* g_out, float* loss, double* partial, hipStream_t st)
{
    constexpr int PER_BLOCK = NE_WAVES * (64 / L);
    const int blocks = sgnn_grid_for(n_pairs, PER_BLOCK, NE_LOSS_BLOCKS_MAX);
    const double inv_n = 1.0 / (double)n_pairs;
    hipLaunchKernelGGL((ne_link_loss_kernel<L, C>), dim3(blocks), dim3(64 * NE_WAVES), 0, st, (const float4*)Z, F4, pu, pv, n_pairs,
                       n_pos, inv_n, s_out, g_out, partial);
    SGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(ne_loss_finish_kernel, dim3(1), dim3(256), 0, st, partial, blocks, inv_n, loss);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_ne_link_loss(const float* Z, int64_t F, const int32_t* pu, const int32_t* pv, int64_t n_pairs, int64_t n_pos,
                                 float* s_out, float* g_out, float* loss, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (!Z || !pu || !pv || !s_out || !loss || !workspace || n_pairs < 1 || n_pos < 0 || n_pos > n_pairs
        || workspace_bytes < sgnn_ne_link_loss_workspace_bytes()) return SGNN_ERR_BAD_ARG;
    if (F <= 0 || F % 4 != 0 || F > 512) return SGNN_ERR_UNSUPPORTED_D;
    if (((uintptr_t)Z & 15) != 0 || ((uintptr_t)workspace & 7) != 0) return SGNN_ERR_BAD_ARG;
    const int64_t F4 = F / 4;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (F4 <= 8) return ne_link_loss_run<8, 1>(Z, F4, pu, pv, n_pairs, n_pos, s_out, g_out, loss, part, st);
    if (F4 <= 16) return ne_link_loss_run<16, 1>(Z, F4, pu, pv, n_pairs, n_pos, s_out, g_out, loss, part, st);
    if (F4 <= 32) return ne_link_loss_run<32, 1>(Z, F4, pu, pv, n_pairs, n_pos, s_out, g_out, loss, part, st);
    if (F4 <= 64) return ne_link_loss_run<64, 1>(Z, F4, pu, pv, n_pairs, n_pos, s_out, g_out, loss, part, st);
    return ne_link_loss_run<64, 2>(Z, F4, pu, pv, n_pairs, n_pos, s_out, g_out, loss, part, st);
}

SGNN_DEFINE_WARM(node_emb)

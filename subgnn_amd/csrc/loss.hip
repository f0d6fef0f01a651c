// Loss and accuracy of a training / validation step in one pass over the logits: nn.CrossEntropyLoss() (mean over the
// batch, reference SubGNN/SubGNN.py:133, applied at SubGNN.py:1116-1124) and the exact-match accuracy the step logs
// (subgraph_utils.calc_accuracy, SubGNN/subgraph_utils.py:108-124).  The library form is log_softmax, an nll reduction
// that runs on ONE workgroup (48 us for 50k rows), argmax, compare, cast, mean, and in the backward two fills, the nll
// backward and the softmax backward: 12 launches.  Here: one kernel per direction + a one-wavefront finish.
//
// Class weights (torch's `weight` / `pos_weight` of the two loss modules built at SubGNN.py:133): every kernel body below is a
// template on WT; the bare kernels are its WT = 0 instantiations under their old names and argument lists, the weighted ones
// (ce_fwd_weighted_kernel, ...) kernels of their own that read the weight rows from global memory (any K).  Single-label: a
// counted row's loss and count are multiplied by w[y] -- the third partial becomes the sum of weights, which the finish writes
// to lse[B] as before; w[y] is read only for y in [0, K).  Multi-label: the mean stays over B K.
//
// Shaped losses (label smoothing and focal loss): a further compile-time axis SH on the same bodies (0: as above; 1:
// label smoothing eps, single-label only; 2: focal gamma).  The SH = 0 instantiations are the kernels above; SH > 0 are kernels of
// their own (ce_fwd_shaped_kernel<SH>, ce_bwd_shaped_kernel<SH>, bce_fwd_focal_kernel, bce_bwd_focal_kernel) that always take the
// weight rows (an absent one stands as ones) and a by-value LossShape {eps, gamma}.
// Every formula is written in loss_terms.h, which the fused head shares.  Partials, the finish kernels and the summation orders
// are those of the bare kernels.
#include "loss_terms.h"

// thread per row; per-workgroup partial sums added in a fixed order (bit-reproducible)
template <int WT, int SH = 0>
__device__ __forceinline__ void ce_fwd_body(const float* __restrict__ logits, const int64_t* __restrict__ labels, int64_t B, int32_t K,
                                            const float* __restrict__ weight, float* __restrict__ lse, float* __restrict__ partial_loss,
                                            float* __restrict__ partial_hits, float* __restrict__ partial_rows,
                                            const LossShape Sp = LossShape{0.f, 0.f})
{
    __shared__ float sh_l[256], sh_h[256], sh_n[256];
    const int64_t r = blockIdx.x * 256ll + threadIdx.x;
    float loss = 0.f, hit = 0.f, cnt = 0.f;
    if (r < B) {
        const float* x = logits + r * K;
        int am;
        const float l = loss_lse_argmax(x, K, am);
        lse[r] = l;
        const int64_t y = labels[r];
        if (y >= 0 && y < K) {
            const LossRow<SH != 0> w{weight};             // (the shaped kernels' row is nullable: an absent one stands as ones)
            hit = (am == (int32_t)y) ? 1.f : 0.f;
            cnt = WT ? w(y) : 1.f;
            loss = loss_sl_row<WT, SH>(x, K, y, l, cnt, w, Sp);
        }
        else if (y != SGNN_CE_IGNORE_INDEX) { loss = __builtin_nanf(""); cnt = 1.f; }
    }
    sh_l[threadIdx.x] = loss;
    sh_h[threadIdx.x] = hit;
    sh_n[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x < 64) {
        float a = (sh_l[threadIdx.x] + sh_l[threadIdx.x + 64]) + (sh_l[threadIdx.x + 128] + sh_l[threadIdx.x + 192]);
        float h = (sh_h[threadIdx.x] + sh_h[threadIdx.x + 64]) + (sh_h[threadIdx.x + 128] + sh_h[threadIdx.x + 192]);
        float n = (sh_n[threadIdx.x] + sh_n[threadIdx.x + 64]) + (sh_n[threadIdx.x + 128] + sh_n[threadIdx.x + 192]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); h += __shfl_xor(h, o, 64); n += __shfl_xor(n, o, 64); }
        if (threadIdx.x == 0) { partial_loss[blockIdx.x] = a; partial_hits[blockIdx.x] = h; partial_rows[blockIdx.x] = n; }
    }
}

__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int64_t B,
                                                     int32_t K, float* __restrict__ lse, float* __restrict__ partial_loss,
                                                     float* __restrict__ partial_hits, float* __restrict__ partial_rows)
{
    ce_fwd_body<0>(logits, labels, B, K, nullptr, lse, partial_loss, partial_hits, partial_rows);
}

__global__ __launch_bounds__(256) void ce_fwd_weighted_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              int64_t B, int32_t K, const float* __restrict__ weight,
                                                              float* __restrict__ lse, float* __restrict__ partial_loss,
                                                              float* __restrict__ partial_hits, float* __restrict__ partial_rows)
{
    ce_fwd_body<1>(logits, labels, B, K, weight, lse, partial_loss, partial_hits, partial_rows);
}

template <int SH>
__global__ __launch_bounds__(256) void ce_fwd_shaped_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                            int64_t B, int32_t K, const float* __restrict__ weight,
                                                            float* __restrict__ lse, float* __restrict__ partial_loss,
                                                            float* __restrict__ partial_hits, float* __restrict__ partial_rows,
                                                            const LossShape Sp)
{
    ce_fwd_body<1, SH>(logits, labels, B, K, weight, lse, partial_loss, partial_hits, partial_rows, Sp);
}

__global__ __launch_bounds__(64) void ce_finish_kernel(const float* __restrict__ partial_loss, const float* __restrict__ partial_hits,
                                                       const float* __restrict__ partial_rows, int64_t nblk, int64_t B,
                                                       float* __restrict__ loss, float* __restrict__ accuracy, float* __restrict__ rows)
{
    float a = 0.f, h = 0.f, n = 0.f;
    for (int64_t k = threadIdx.x; k < nblk; k += 64) { a += partial_loss[k]; h += partial_hits[k]; n += partial_rows[k]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); h += __shfl_xor(h, o, 64); n += __shfl_xor(n, o, 64); }
    if (threadIdx.x == 0) {
        loss[0] = a / n;                          // every row ignored: 0 / 0 = NaN, as the library gives
        rows[0] = n;                              // lse[B]: the divisor the backward uses (counts are exact in float up to 2^24 per partial sum tree)
        if (accuracy) accuracy[0] = h / (float)B;
    }
}

// thread per logit: d loss / d logits[r, k] (loss_sl_grad) at scale = grad_loss / lse[B], the divisor the finish left there
template <int WT, int SH = 0>
__device__ __forceinline__ void ce_bwd_body(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                            const float* __restrict__ lse, const float* __restrict__ grad_loss, int64_t B, int32_t K,
                                            const float* __restrict__ weight, float* __restrict__ grad_logits,
                                            const LossShape Sp = LossShape{0.f, 0.f})
{
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    const LossRow<SH != 0> w{weight};                       // (the shaped kernels' row is nullable: an absent one stands as ones)
    float W = 0.f;
    if (SH == 1) {                                          // W = sum of the class weights: strided sums, then a fixed tree
        __shared__ float sh_w[256];
        float s = 0.f;
        for (int32_t k = threadIdx.x; k < K; k += 256) s += w(k);
        sh_w[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh_w[threadIdx.x] += sh_w[threadIdx.x + o];
            __syncthreads();
        }
        W = sh_w[0];
    }
    if (t >= B * K) return;
    const int64_t r = t / K;
    const int32_t k = (int32_t)(t - r * K);
    const int64_t y = labels[r];
    const float scale = grad_loss[0] / lse[B];
    grad_logits[t] = (y >= 0 && y < K) ? loss_sl_grad<WT, SH>(logits[t], logits + r * K + y, K, k, y, lse[r], w, W, Sp, scale) : 0.f;
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ lse, const float* __restrict__ grad_loss, int64_t B,
                                                     int32_t K, float* __restrict__ grad_logits)
{
    ce_bwd_body<0>(logits, labels, lse, grad_loss, B, K, nullptr, grad_logits);
}

__global__ __launch_bounds__(256) void ce_bwd_weighted_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ lse, const float* __restrict__ grad_loss,
                                                              int64_t B, int32_t K, const float* __restrict__ weight,
                                                              float* __restrict__ grad_logits)
{
    ce_bwd_body<1>(logits, labels, lse, grad_loss, B, K, weight, grad_logits);
}

template <int SH>
__global__ __launch_bounds__(256) void ce_bwd_shaped_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                            const float* __restrict__ lse, const float* __restrict__ grad_loss,
                                                            int64_t B, int32_t K, const float* __restrict__ weight,
                                                            float* __restrict__ grad_logits, const LossShape Sp)
{
    ce_bwd_body<1, SH>(logits, labels, lse, grad_loss, B, K, weight, grad_logits, Sp);
}

static inline int64_t ce_blocks(int64_t B) { return (B + 255) / 256; }

extern "C" int64_t sgnn_cross_entropy_workspace_bytes(int64_t B)
{
    if (B < 0) return -1;
    return 3 * ce_blocks(B) * (int64_t)sizeof(float) + 16;
}

// weight: DEVICE row of K class weights, nullable (null: the bare kernel)
static int ce_fwd_launch(const float* logits, const int64_t* labels, int64_t B, int64_t K, float* lse, float* loss, float* accuracy,
                         void* workspace, int64_t workspace_bytes, void* stream, const float* weight, float eps = 0.f, float gamma = 0.f)
{
    if (!loss_shape_ok(false, eps, gamma)) return SGNN_ERR_BAD_ARG;
    if (!logits || !labels || !lse || !loss || B < 1 || K < 1 || K > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < sgnn_cross_entropy_workspace_bytes(B)) return SGNN_ERR_BAD_ARG;
    const int64_t nblk = ce_blocks(B);
    if (nblk > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    float* pl = (float*)workspace;
    float* ph = pl + nblk;
    float* pn = ph + nblk;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), block(256);
    const int32_t k = (int32_t)K;
    const LossShape Sp{eps, gamma};
    if (eps > 0.f) hipLaunchKernelGGL(ce_fwd_shaped_kernel<1>, grid, block, 0, st, logits, labels, B, k, weight, lse, pl, ph, pn, Sp);
    else if (gamma > 0.f) hipLaunchKernelGGL(ce_fwd_shaped_kernel<2>, grid, block, 0, st, logits, labels, B, k, weight, lse, pl, ph, pn, Sp);
    else if (weight) hipLaunchKernelGGL(ce_fwd_weighted_kernel, grid, block, 0, st, logits, labels, B, k, weight, lse, pl, ph, pn);
    else hipLaunchKernelGGL(ce_fwd_kernel, grid, block, 0, st, logits, labels, B, k, lse, pl, ph, pn);
    SGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(64), 0, st, pl, ph, pn, nblk, B, loss, accuracy, lse + B);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_cross_entropy_fwd(const float* logits, const int64_t* labels, int64_t B, int64_t K, float* lse, float* loss,
                                      float* accuracy, void* workspace, int64_t workspace_bytes, void* stream)
{
    return ce_fwd_launch(logits, labels, B, K, lse, loss, accuracy, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int sgnn_cross_entropy_fwd_weighted(const float* logits, const int64_t* labels, int64_t B, int64_t K, float* lse, float* loss,
                                               float* accuracy, void* workspace, int64_t workspace_bytes, void* stream,
                                               const float* class_weight)
{
    return ce_fwd_launch(logits, labels, B, K, lse, loss, accuracy, workspace, workspace_bytes, stream, class_weight);
}

extern "C" int sgnn_cross_entropy_fwd_shaped(const float* logits, const int64_t* labels, int64_t B, int64_t K, float* lse, float* loss,
                                             float* accuracy, void* workspace, int64_t workspace_bytes, void* stream,
                                             const float* class_weight, float label_smoothing, float focal_gamma)
{
    return ce_fwd_launch(logits, labels, B, K, lse, loss, accuracy, workspace, workspace_bytes, stream, class_weight, label_smoothing,
                         focal_gamma);
}

static int ce_bwd_launch(const float* logits, const int64_t* labels, const float* lse, const float* grad_loss, int64_t B, int64_t K,
                         float* grad_logits, void* stream, const float* weight, float eps = 0.f, float gamma = 0.f)
{
    if (!loss_shape_ok(false, eps, gamma)) return SGNN_ERR_BAD_ARG;
    if (!logits || !labels || !lse || !grad_loss || !grad_logits || B < 1 || K < 1 || K > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    if ((B * K + 255) / 256 > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((B * K + 255) / 256)), block(256);
    const int32_t k = (int32_t)K;
    const LossShape Sp{eps, gamma};
    if (eps > 0.f) hipLaunchKernelGGL(ce_bwd_shaped_kernel<1>, grid, block, 0, st, logits, labels, lse, grad_loss, B, k, weight, grad_logits, Sp);
    else if (gamma > 0.f) hipLaunchKernelGGL(ce_bwd_shaped_kernel<2>, grid, block, 0, st, logits, labels, lse, grad_loss, B, k, weight, grad_logits, Sp);
    else if (weight) hipLaunchKernelGGL(ce_bwd_weighted_kernel, grid, block, 0, st, logits, labels, lse, grad_loss, B, k, weight, grad_logits);
    else hipLaunchKernelGGL(ce_bwd_kernel, grid, block, 0, st, logits, labels, lse, grad_loss, B, k, grad_logits);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_cross_entropy_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_loss, int64_t B,
                                      int64_t K, float* grad_logits, void* stream)
{
    return ce_bwd_launch(logits, labels, lse, grad_loss, B, K, grad_logits, stream, nullptr);
}

extern "C" int sgnn_cross_entropy_bwd_weighted(const float* logits, const int64_t* labels, const float* lse, const float* grad_loss,
                                               int64_t B, int64_t K, float* grad_logits, void* stream, const float* class_weight)
{
    return ce_bwd_launch(logits, labels, lse, grad_loss, B, K, grad_logits, stream, class_weight);
}

extern "C" int sgnn_cross_entropy_bwd_shaped(const float* logits, const int64_t* labels, const float* lse, const float* grad_loss,
                                             int64_t B, int64_t K, float* grad_logits, void* stream, const float* class_weight,
                                             float label_smoothing, float focal_gamma)
{
    return ce_bwd_launch(logits, labels, lse, grad_loss, B, K, grad_logits, stream, class_weight, label_smoothing, focal_gamma);
}

// ---- multi-label: nn.BCEWithLogitsLoss() (mean over B x K, SubGNN.py:133 with several labels per subgraph) + the exact-match
// accuracy of su:108-124, for any K.  targets: int64 (B, K) indicator matrix, non-zero counts as 1.  A thread walks its row in k
// order, adding loss_ml_term; the row is a hit when loss_ml_hit holds in every column.  Either weight row may be absent: it stands
// as ones.  Same partials and the same fixed order as the single-label pair.
template <int WT, int SH = 0>
__device__ __forceinline__ void bce_fwd_body(const float* __restrict__ logits, const int64_t* __restrict__ targets, int64_t B, int32_t K,
                                             const float* __restrict__ weight, const float* __restrict__ pos_weight,
                                             float* __restrict__ partial_loss, float* __restrict__ partial_hits,
                                             const LossShape Sp = LossShape{0.f, 0.f})
{
    __shared__ float sh_l[256], sh_h[256];
    const int64_t r = blockIdx.x * 256ll + threadIdx.x;
    float loss = 0.f, hit = 0.f;
    if (r < B) {
        const float* x = logits + r * K;
        const int64_t* y = targets + r * K;
        const LossRow<true> cw{weight}, pw{pos_weight};
        bool all = true;
        for (int32_t k = 0; k < K; ++k) {
            const float v = x[k];
            const bool t = y[k] != 0;
            loss += loss_ml_term<WT, SH>(v, t, k, cw, pw, Sp);
            all = all && loss_ml_hit(v, t);
        }
        hit = all ? 1.f : 0.f;
    }
    sh_l[threadIdx.x] = loss;
    sh_h[threadIdx.x] = hit;
    __syncthreads();
    if (threadIdx.x < 64) {
        float a = (sh_l[threadIdx.x] + sh_l[threadIdx.x + 64]) + (sh_l[threadIdx.x + 128] + sh_l[threadIdx.x + 192]);
        float h = (sh_h[threadIdx.x] + sh_h[threadIdx.x + 64]) + (sh_h[threadIdx.x + 128] + sh_h[threadIdx.x + 192]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); h += __shfl_xor(h, o, 64); }
        if (threadIdx.x == 0) { partial_loss[blockIdx.x] = a; partial_hits[blockIdx.x] = h; }
    }
}

__global__ __launch_bounds__(256) void bce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets, int64_t B,
                                                      int32_t K, float* __restrict__ partial_loss, float* __restrict__ partial_hits)
{
    bce_fwd_body<0>(logits, targets, B, K, nullptr, nullptr, partial_loss, partial_hits);
}

__global__ __launch_bounds__(256) void bce_fwd_weighted_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                               int64_t B, int32_t K, const float* __restrict__ weight,
                                                               const float* __restrict__ pos_weight, float* __restrict__ partial_loss,
                                                               float* __restrict__ partial_hits)
{
    bce_fwd_body<1>(logits, targets, B, K, weight, pos_weight, partial_loss, partial_hits);
}

__global__ __launch_bounds__(256) void bce_fwd_focal_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                            int64_t B, int32_t K, const float* __restrict__ weight,
                                                            const float* __restrict__ pos_weight, float* __restrict__ partial_loss,
                                                            float* __restrict__ partial_hits, const LossShape Sp)
{
    bce_fwd_body<1, 2>(logits, targets, B, K, weight, pos_weight, partial_loss, partial_hits, Sp);
}

__global__ __launch_bounds__(64) void bce_finish_kernel(const float* __restrict__ partial_loss, const float* __restrict__ partial_hits,
                                                        int64_t nblk, int64_t B, int64_t K, float* __restrict__ loss,
                                                        float* __restrict__ accuracy)
{
    float a = 0.f, h = 0.f;
    for (int64_t k = threadIdx.x; k < nblk; k += 64) { a += partial_loss[k]; h += partial_hits[k]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); h += __shfl_xor(h, o, 64); }
    if (threadIdx.x == 0) {
        loss[0] = a / (float)(B * K);
        if (accuracy) accuracy[0] = h / (float)B;
    }
}

// thread per element: d loss / d logits[r, k] (loss_ml_grad) at scale = grad_loss / (B K); the bare kernel needs no column index
template <int WT, int SH = 0>
__device__ __forceinline__ void bce_bwd_body(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                             const float* __restrict__ grad_loss, int64_t n, int32_t K, const float* __restrict__ weight,
                                             const float* __restrict__ pos_weight, float* __restrict__ grad_logits,
                                             const LossShape Sp = LossShape{0.f, 0.f})
{
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    if (t >= n) return;
    const int32_t k = WT ? (int32_t)(t % K) : 0;
    grad_logits[t] = loss_ml_grad<WT, SH>(logits[t], targets[t] != 0, k, LossRow<true>{weight}, LossRow<true>{pos_weight}, Sp,
                                          grad_loss[0] / (float)n);
}

__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                      const float* __restrict__ grad_loss, int64_t n, float* __restrict__ grad_logits)
{
    bce_bwd_body<0>(logits, targets, grad_loss, n, 1, nullptr, nullptr, grad_logits);
}

__global__ __launch_bounds__(256) void bce_bwd_weighted_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                               const float* __restrict__ grad_loss, int64_t n, int32_t K,
                                                               const float* __restrict__ weight, const float* __restrict__ pos_weight,
                                                               float* __restrict__ grad_logits)
{
    bce_bwd_body<1>(logits, targets, grad_loss, n, K, weight, pos_weight, grad_logits);
}

__global__ __launch_bounds__(256) void bce_bwd_focal_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                            const float* __restrict__ grad_loss, int64_t n, int32_t K,
                                                            const float* __restrict__ weight, const float* __restrict__ pos_weight,
                                                            float* __restrict__ grad_logits, const LossShape Sp)
{
    bce_bwd_body<1, 2>(logits, targets, grad_loss, n, K, weight, pos_weight, grad_logits, Sp);
}

extern "C" int64_t sgnn_bce_logits_workspace_bytes(int64_t B)
{
    if (B < 0) return -1;
    return 2 * ce_blocks(B) * (int64_t)sizeof(float) + 16;
}

// weight / pos_weight: DEVICE rows of K floats, either nullable (both null: the bare kernel)
static int bce_fwd_launch(const float* logits, const int64_t* targets, int64_t B, int64_t K, float* loss, float* accuracy,
                          void* workspace, int64_t workspace_bytes, void* stream, const float* weight, const float* pos_weight,
                          float gamma = 0.f)
{
    if (!loss_shape_ok(false, 0.f, gamma)) return SGNN_ERR_BAD_ARG;
    if (!logits || !targets || !loss || B < 1 || K < 1 || K > 0x7fffffff || B > (int64_t)0x7fffffffffffffffll / K) return SGNN_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < sgnn_bce_logits_workspace_bytes(B)) return SGNN_ERR_BAD_ARG;
    const int64_t nblk = ce_blocks(B);
    if (nblk > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    float* pl = (float*)workspace;
    float* ph = pl + nblk;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), block(256);
    const int32_t k = (int32_t)K;
    if (gamma > 0.f) hipLaunchKernelGGL(bce_fwd_focal_kernel, grid, block, 0, st, logits, targets, B, k, weight, pos_weight, pl, ph, LossShape{0.f, gamma});
    else if (weight || pos_weight) hipLaunchKernelGGL(bce_fwd_weighted_kernel, grid, block, 0, st, logits, targets, B, k, weight, pos_weight, pl, ph);
    else hipLaunchKernelGGL(bce_fwd_kernel, grid, block, 0, st, logits, targets, B, k, pl, ph);
    SGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(64), 0, st, pl, ph, nblk, B, K, loss, accuracy);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_bce_logits_fwd(const float* logits, const int64_t* targets, int64_t B, int64_t K, float* loss, float* accuracy,
                                   void* workspace, int64_t workspace_bytes, void* stream)
{
    return bce_fwd_launch(logits, targets, B, K, loss, accuracy, workspace, workspace_bytes, stream, nullptr, nullptr);
}

extern "C" int sgnn_bce_logits_fwd_weighted(const float* logits, const int64_t* targets, int64_t B, int64_t K, float* loss, float* accuracy,
                                            void* workspace, int64_t workspace_bytes, void* stream, const float* weight,
                                            const float* pos_weight)
{
    return bce_fwd_launch(logits, targets, B, K, loss, accuracy, workspace, workspace_bytes, stream, weight, pos_weight);
}

extern "C" int sgnn_bce_logits_fwd_shaped(const float* logits, const int64_t* targets, int64_t B, int64_t K, float* loss, float* accuracy,
                                          void* workspace, int64_t workspace_bytes, void* stream, const float* weight,
                                          const float* pos_weight, float focal_gamma)
{
    return bce_fwd_launch(logits, targets, B, K, loss, accuracy, workspace, workspace_bytes, stream, weight, pos_weight, focal_gamma);
}

static int bce_bwd_launch(const float* logits, const int64_t* targets, const float* grad_loss, int64_t B, int64_t K, float* grad_logits,
                          void* stream, const float* weight, const float* pos_weight, float gamma = 0.f)
{
    if (!loss_shape_ok(false, 0.f, gamma)) return SGNN_ERR_BAD_ARG;
    if (!logits || !targets || !grad_loss || !grad_logits || B < 1 || K < 1 || B > (int64_t)0x7fffffffffffffffll / K) return SGNN_ERR_BAD_ARG;
    if ((B * K + 255) / 256 > 0x7fffffff) return SGNN_ERR_BAD_ARG;
    const bool bare = !(gamma > 0.f) && !weight && !pos_weight;
    if (!bare && K > 0x7fffffff) return SGNN_ERR_BAD_ARG;              // (only the bare kernel takes no column index)
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((B * K + 255) / 256)), block(256);
    const int64_t n = B * K;
    const int32_t k = (int32_t)K;
    if (gamma > 0.f) hipLaunchKernelGGL(bce_bwd_focal_kernel, grid, block, 0, st, logits, targets, grad_loss, n, k, weight, pos_weight, grad_logits, LossShape{0.f, gamma});
    else if (!bare) hipLaunchKernelGGL(bce_bwd_weighted_kernel, grid, block, 0, st, logits, targets, grad_loss, n, k, weight, pos_weight, grad_logits);
    else hipLaunchKernelGGL(bce_bwd_kernel, grid, block, 0, st, logits, targets, grad_loss, n, grad_logits);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

extern "C" int sgnn_bce_logits_bwd(const float* logits, const int64_t* targets, const float* grad_loss, int64_t B, int64_t K,
                                   float* grad_logits, void* stream)
{
    return bce_bwd_launch(logits, targets, grad_loss, B, K, grad_logits, stream, nullptr, nullptr);
}

extern "C" int sgnn_bce_logits_bwd_weighted(const float* logits, const int64_t* targets, const float* grad_loss, int64_t B, int64_t K,
                                            float* grad_logits, void* stream, const float* weight, const float* pos_weight)
{
    return bce_bwd_launch(logits, targets, grad_loss, B, K, grad_logits, stream, weight, pos_weight);
}

extern "C" int sgnn_bce_logits_bwd_shaped(const float* logits, const int64_t* targets, const float* grad_loss, int64_t B, int64_t K,
                                          float* grad_logits, void* stream, const float* weight, const float* pos_weight,
                                          float focal_gamma)
{
    return bce_bwd_launch(logits, targets, grad_loss, B, K, grad_logits, stream, weight, pos_weight, focal_gamma);
}

SGNN_DEFINE_WARM(loss)

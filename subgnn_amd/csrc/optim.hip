// Adam on one float32 buffer in one pass over memory: p, g, m, v read once, p, m, v written.  Update rule = torch.optim.Adam
// (no amsgrad):
//   m = m + (1 - b1) (gk - m);  v = b2 v + (1 - b2) gk gk;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// with the gradient term gk in one of two forms, chosen per launch:
//   L2 = false: gk = g * scale -- the caller's clip coefficient, a device scalar read on the fly (no host round trip), 1 when
//               absent: the owned slice of the sharded table (dist.ShardedTableAdam; reference SubGNN/SubGNN.py:1156-1161 +
//               train_config.py: Trainer(gradient_clip_val));
//   L2 = true:  gk = g + wd p -- torch.optim.Adam(weight_decay = wd)'s coupled L2: the node-embedding trainer (reference
//               prepare_dataset/train_node_emb.py:99).
// n any length: the float4 body covers n / 4 elements, one extra lane per remaining element.
#include "common.h"

template <bool L2>
__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n, float b1, float b2, float eps, float wd,
                                                        const float* __restrict__ grad_scale, float step_size, float rsqrt_bc2)
{
    const float gs = grad_scale ? grad_scale[0] : 1.f;
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4 + (n - n4 * 4); i += stride) {
        if (i < n4) {
            float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
            float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gk = L2 ? G[k] + wd * P[k] : G[k] * gs;
                M[k] = M[k] + (1.f - b1) * (gk - M[k]);
                V[k] = b2 * V[k] + (1.f - b2) * gk * gk;
                P[k] -= step_size * M[k] / (sqrtf(V[k]) * rsqrt_bc2 + eps);
            }
            reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
        } else {
            const int64_t j = n4 * 4 + (i - n4);
            const float gk = L2 ? g[j] + wd * p[j] : g[j] * gs;
            m[j] = m[j] + (1.f - b1) * (gk - m[j]);
            v[j] = b2 * v[j] + (1.f - b2) * gk * gk;
            p[j] -= step_size * m[j] / (sqrtf(v[j]) * rsqrt_bc2 + eps);
        }
    }
}

extern "C" int sgnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int64_t step, const float* grad_scale, void* stream)
{
    if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return SGNN_ERR_BAD_ARG;
    if (grad_scale && weight_decay != 0.f) return SGNN_ERR_BAD_ARG;       // one gradient form per launch
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return SGNN_ERR_BAD_ARG;
    if (n == 0) return SGNN_OK;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1), rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
    const dim3 grid(sgnn_grid_for(n / 4 + n % 4, 256));
    if (weight_decay != 0.f)
        hipLaunchKernelGGL(adam_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n,
                           beta1, beta2, eps, weight_decay, nullptr, step_size, rsqrt_bc2);
    else
        hipLaunchKernelGGL(adam_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n,
                           beta1, beta2, eps, 0.f, grad_scale, step_size, rsqrt_bc2);
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}


// ---- the whole optimizer tail in two launches -----------------------------------------------------------------------------
// clip_grad_norm_ + Adam over EVERY parameter (train_config.py: Trainer(gradient_clip_val); SubGNN/SubGNN.py:1156-1161).  As
// library calls a batch-sized step paid ~12 launches and ~155 us here (a multi-tensor norm + clean-up + stack, the coefficient,
// a multi-tensor multiply, torch's fused Adam in two launches of 40-50 us each -- it evaluates pow() in double per thread --
// a count kernel and the table's pass) of a 1.0-2.9 ms step.  Here: launch 1 = per-workgroup sums of squares of every gradient
// (+ the device step counts advance), launch 2 = every workgroup adds the partials in one fixed order (the same value in all
// of them), forms the coefficient and updates its chunk.  Tensors travel as kernel arguments (pointers of gradients change from
// step to step in eager mode and are frozen into a recorded step), OPT_MAXT per launch.
#define OPT_MAXT 72
#define OPT_EMA_MAXT 56                   // tensors per launch of the updates that also move a weight average (a fifth pointer each)
#define OPT_CHUNK 4096                    // floats per workgroup iteration: 256 lanes x 4 float4
#define OPT_MAX_BLOCKS 2048               // per tensor; larger tensors stride

template <int MAXT>
struct OptTensorsT {
    float* p[MAXT]; float* g[MAXT]; float* m[MAXT]; float* v[MAXT];
    long long n[MAXT];
    int blk[MAXT + 1];                    // first workgroup of tensor t inside this launch
    int zero[MAXT];
    int slot[MAXT];                       // which device step count belongs to tensor t
    int count;
    // one tensor of the launch may be a table of rows with a per-row "ever had a gradient" byte: a row whose gradient is all
    // zero and that never had one has m = v = 0, so Adam leaves it exactly as it is (update = step_size * 0 / (0 + eps)) --
    // it costs the read of its gradient instead of four reads and three or four writes.  A shard's subgraphs, border sets and
    // anchor patches reach ~40 % of a million-node table's rows (7 % for one of 8 strong-scaling shards), the same ones every pass.
    int rows_t;                           // index of that tensor in this launch, -1 = none
    int row_lanes;                        // float4 lanes per row: a power of two <= 64
    unsigned char* seen;
};
typedef OptTensorsT<OPT_MAXT> OptTensors;
// the same with the weight averages: e += (1 - d_s) (p_new - e) inside the update, d_s = ema_decay, or with ema_warmup
// min(ema_decay, (1 + s) / (10 + s)) at the tensor's step count s.  Kernel arguments end at 4 KB and OptTensors takes 3.7 of
// them: a fifth pointer per tensor does not fit beside 72 tensors, so these launches hold OPT_EMA_MAXT.
struct OptTensorsEma : OptTensorsT<OPT_EMA_MAXT> {
    float* e[OPT_EMA_MAXT];
    float ema_decay;
    int ema_warmup;
};
template <bool EMA> struct OptArgs { typedef OptTensors type; };
template <> struct OptArgs<true> { typedef OptTensorsEma type; };
// (the launch's other arguments take 72 bytes and the hidden ones 256)
static_assert(sizeof(OptTensors) == 3768 && sizeof(OptTensors) + 72 + 256 <= 4096, "OptTensors outgrew the kernel-argument segment");
static_assert(sizeof(OptTensorsEma) == 3392 && sizeof(OptTensorsEma) + 72 + 256 <= 4096, "OptTensorsEma outgrew the kernel-argument segment");

template <class TT>
__device__ __forceinline__ int opt_find(const TT& T, int b)
{
    int lo = 0, hi = T.count - 1;         // largest t with blk[t] <= b
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (T.blk[mid] <= b) lo = mid; else hi = mid - 1; }
    return lo;
}

__global__ __launch_bounds__(256) void optim_sumsq_kernel(const OptTensors T, float* __restrict__ partial, int64_t* __restrict__ counters)
{
    __shared__ float sh[256];
    const int b = blockIdx.x, t = opt_find(T, b), nb = T.blk[t + 1] - T.blk[t];
    const float* __restrict__ g = T.g[t];
    const int64_t n = T.n[t];
    if (counters && b == 0 && (int)threadIdx.x < T.count) counters[T.slot[threadIdx.x]] += 1;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if ((((uintptr_t)g) & 15) == 0) {
        const int64_t n4 = n >> 2;
        const float4* __restrict__ g4 = (const float4*)g;
        for (int64_t i = (int64_t)(b - T.blk[t]) * 256 + threadIdx.x; i < n4; i += (int64_t)nb * 256) {
            const float4 x = g4[i];
            a0 = fmaf(x.x, x.x, a0); a1 = fmaf(x.y, x.y, a1); a2 = fmaf(x.z, x.z, a2); a3 = fmaf(x.w, x.w, a3);
        }
        if (b == T.blk[t] && (int64_t)threadIdx.x < n - n4 * 4) { const float x = g[n4 * 4 + threadIdx.x]; a0 = fmaf(x, x, a0); }
    } else {
        for (int64_t i = (int64_t)(b - T.blk[t]) * 256 + threadIdx.x; i < n; i += (int64_t)nb * 256) { const float x = g[i]; a0 = fmaf(x, x, a0); }
    }
    sh[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (threadIdx.x < 64) {
        float v = (sh[threadIdx.x] + sh[threadIdx.x + 64]) + (sh[threadIdx.x + 128] + sh[threadIdx.x + 192]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (threadIdx.x == 0) partial[b] = v;
    }
}

#ifndef OPT_ROW_SLICES
#define OPT_ROW_SLICES 2
#endif
// EMA: the launch also moves the weight averages T.e (OptTensorsEma) of every element it steps -- one more read and one more
// write beside the parameter's, which is in registers here; an element that is not stepped (a skipped row, a tensor outside
// the launch) keeps its average: it advances with the tensor's own steps.  <false> is the update as it always was.
template <bool EMA>
__global__ __launch_bounds__(256) void optim_adam_kernel(const typename OptArgs<EMA>::type T, const float* __restrict__ partial, int n_partial,
                                                         float max_norm, float* __restrict__ coef_out, float lr, float b1, float b2, float eps,
                                                         long long host_step, const int64_t* __restrict__ counters,
                                                         const float* __restrict__ lr_table, long long lr_len)
{
    __shared__ double shd[256];
    const int b = blockIdx.x, t = opt_find(T, b), nb = T.blk[t + 1] - T.blk[t];
    float gs = 1.f;
    if (max_norm > 0.f) {                 // the same additions in the same order in every workgroup: one coefficient for all
        double acc = 0.0;
        for (int k = threadIdx.x; k < n_partial; k += 256) acc += (double)partial[k];
        shd[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) shd[threadIdx.x] += shd[threadIdx.x + w];
            __syncthreads();
        }
        const float total = (float)sqrt(shd[0]);
        // a NaN norm (a NaN gradient anywhere) gives a NaN coefficient, as torch's clamp(max_norm / (total + 1e-6), max=1)
        // does, so every parameter turns NaN as under clip_grad_norm_ (fminf would return 1 and step the others unclipped)
        gs = total != total ? total : fminf(max_norm / (total + 1e-6f), 1.f);
        if (coef_out && b == 0 && threadIdx.x == 0) { coef_out[0] = gs; coef_out[1] = total; }
    }
    const long long s = counters ? (long long)counters[T.slot[t]] : host_step;
    const double st = (double)s;
    // a learning-rate table on the device (a range test's schedule): step s takes entry min(s, lr_len) - 1, so one recording
    // replays every rate; the same double arithmetic as the host float, so a table of float(lr) is bit-identical to it
    const float lr_s = lr_table ? lr_table[(s < lr_len ? (s > 1 ? s : 1) : lr_len) - 1] : lr;
    const float step_size = (float)((double)lr_s / (1.0 - pow((double)b1, st)));
    const float rsqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, st)));
    float* __restrict__ p = T.p[t]; float* __restrict__ g = T.g[t]; float* __restrict__ m = T.m[t]; float* __restrict__ v = T.v[t];
    float* __restrict__ e = nullptr;
    float w = 0.f;                        // 1 - d_s, formed once per workgroup, in double (as step_size)
    if constexpr (EMA) {
        e = T.e[t];
        double d = (double)T.ema_decay;
        if (T.ema_warmup) { const double dw = (1.0 + st) / (10.0 + st); d = dw < d ? dw : d; }
        w = (float)(1.0 - d);
    }
    const int64_t n = T.n[t];
    const int zero = T.zero[t];
    if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)e)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        float4* p4 = (float4*)p; float4* g4 = (float4*)g; float4* m4 = (float4*)m; float4* v4 = (float4*)v; float4* e4 = (float4*)e;
        if (t == T.rows_t) {
            // (n = rows * 4 L and a wavefront's 64 consecutive float4 start at a multiple of 64: a row's lanes share a wavefront)
            const int L = T.row_lanes, lane = threadIdx.x & 63, sh = 31 - __builtin_clz(L);
            const unsigned long long rowmask = (L == 64 ? ~0ull : ((1ull << L) - 1ull)) << (lane & ~(L - 1));
            unsigned char* __restrict__ seen = T.seen;
            // OPT_ROW_SLICES row slices per thread and iteration (round 6), all loads of an iteration issued before the first is used: the
            // gradient slices first, then -- WITHOUT a branch: a lane whose row is skipped reads slot 0 of the tensor, a cached
            // line -- parameter and both moments of both slices.  One slice per iteration with its p / m / v loads behind a
            // branch on the gradient was two dependent memory round trips per 16 bytes of every stream: 2.8 TB/s.
            const int64_t stride = (int64_t)nb * 256;
            constexpr int U = OPT_ROW_SLICES;
            for (int64_t i0 = (int64_t)(b - T.blk[t]) * 256 + threadIdx.x; i0 < n4; i0 += U * stride) {
                float4 gg[U];
                int64_t idx[U];
                bool in[U], any[U], was[U], act[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    idx[u] = i0 + u * stride;
                    in[u] = idx[u] < n4;                         // (wave-uniform: n4 is a multiple of 64 here)
                    gg[u] = in[u] ? g4[idx[u]] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool nz = gg[u].x != 0.f || gg[u].y != 0.f || gg[u].z != 0.f || gg[u].w != 0.f;
                    any[u] = (__ballot(nz) & rowmask) != 0ull;
                    was[u] = in[u] ? seen[idx[u] >> sh] != 0 : false;
                    act[u] = in[u] && (any[u] || was[u] || gs != gs);        // a NaN coefficient poisons every row
                }
                float4 pp[U], mm[U], vv[U], ee[EMA ? U : 1];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t j = act[u] ? idx[u] : 0;
                    pp[u] = p4[j]; mm[u] = m4[j]; vv[u] = v4[j];
                    if constexpr (EMA) ee[u] = e4[j];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (act[u]) {
                        float* P = &pp[u].x; float* G = &gg[u].x; float* M = &mm[u].x; float* V = &vv[u].x;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float gk = G[k] * gs;
                            M[k] = M[k] + (1.f - b1) * (gk - M[k]);
                            V[k] = b2 * V[k] + (1.f - b2) * gk * gk;
                            P[k] -= step_size * M[k] / (sqrtf(V[k]) * rsqrt_bc2 + eps);
                            if constexpr (EMA) { float* E = &ee[u].x; E[k] = fmaf(w, P[k] - E[k], E[k]); }
                        }
                        p4[idx[u]] = pp[u]; m4[idx[u]] = mm[u]; v4[idx[u]] = vv[u];
                        if constexpr (EMA) e4[idx[u]] = ee[u];
                        if (zero && any[u]) g4[idx[u]] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (!was[u] && (lane & (L - 1)) == 0) seen[idx[u] >> sh] = 1;
                    }
                }
            }
            return;
        }
        for (int64_t i = (int64_t)(b - T.blk[t]) * 256 + threadIdx.x; i < n4; i += (int64_t)nb * 256) {
            float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i], ee;
            if constexpr (EMA) ee = e4[i];
            float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gk = G[k] * gs;
                M[k] = M[k] + (1.f - b1) * (gk - M[k]);
                V[k] = b2 * V[k] + (1.f - b2) * gk * gk;
                P[k] -= step_size * M[k] / (sqrtf(V[k]) * rsqrt_bc2 + eps);
                if constexpr (EMA) { float* E = &ee.x; E[k] = fmaf(w, P[k] - E[k], E[k]); }
            }
            p4[i] = pp; m4[i] = mm; v4[i] = vv;
            if constexpr (EMA) e4[i] = ee;
            if (zero) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (b == T.blk[t] && (int64_t)threadIdx.x < n - n4 * 4) {
            const int64_t i = n4 * 4 + threadIdx.x;
            const float gk = g[i] * gs;
            const float mk = m[i] + (1.f - b1) * (gk - m[i]);
            const float vk = b2 * v[i] + (1.f - b2) * gk * gk;
            m[i] = mk; v[i] = vk;
            const float pk = p[i] - step_size * mk / (sqrtf(vk) * rsqrt_bc2 + eps);
            p[i] = pk;
            if constexpr (EMA) e[i] = fmaf(w, pk - e[i], e[i]);
            if (zero) g[i] = 0.f;
        }
    } else {
        for (int64_t i = (int64_t)(b - T.blk[t]) * 256 + threadIdx.x; i < n; i += (int64_t)nb * 256) {
            const float gk = g[i] * gs;
            const float mk = m[i] + (1.f - b1) * (gk - m[i]);
            const float vk = b2 * v[i] + (1.f - b2) * gk * gk;
            m[i] = mk; v[i] = vk;
            const float pk = p[i] - step_size * mk / (sqrtf(vk) * rsqrt_bc2 + eps);
            p[i] = pk;
            if constexpr (EMA) e[i] = fmaf(w, pk - e[i], e[i]);
            if (zero) g[i] = 0.f;
        }
    }
}

struct OptSlots { int slot[OPT_MAXT]; int count; };
__global__ void optim_count_kernel(int64_t* counters, const OptSlots S) { if ((int)threadIdx.x < S.count) counters[S.slot[threadIdx.x]] += 1; }

static inline int opt_blocks(int64_t n)
{
    int64_t b = (n + OPT_CHUNK - 1) / OPT_CHUNK;
    return (int)(b < 1 ? 1 : (b > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : b));
}

extern "C" int64_t sgnn_optim_partials(const int64_t* numels, int64_t n_tensors)
{
    if (n_tensors < 0 || (n_tensors && !numels)) return -1;
    int64_t total = 0;
    for (int64_t i = 0; i < n_tensors; ++i) { if (numels[i] < 0) return -1; total += opt_blocks(numels[i]); }
    return total;
}

// one launch group = tensors [from, to): fills T, returns its workgroup count
template <class TT>
static int opt_fill(TT& T, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    const int64_t* numels, const int32_t* zero_grad, const int64_t* slots, int64_t from, int64_t to)
{
    int blocks = 0;
    T.count = (int)(to - from);
    for (int64_t i = from; i < to; ++i) {
        const int k = (int)(i - from);
        T.p[k] = params ? params[i] : nullptr; T.g[k] = grads[i];
        T.m[k] = exp_avg ? exp_avg[i] : nullptr; T.v[k] = exp_avg_sq ? exp_avg_sq[i] : nullptr;
        T.n[k] = numels[i]; T.blk[k] = blocks; T.zero[k] = zero_grad ? zero_grad[i] : 0; T.slot[k] = (int)(slots ? slots[i] : i);
        blocks += opt_blocks(numels[i]);
    }
    T.blk[T.count] = blocks;
    T.rows_t = -1; T.row_lanes = 1; T.seen = nullptr;
    return blocks;
}

extern "C" int sgnn_optim_sumsq(const float* const* grads, const int64_t* numels, int64_t n_tensors, float* partial,
                                int64_t* step_counters, const int64_t* counter_slots, void* stream)
{
    if (n_tensors < 0 || (n_tensors && (!grads || !numels || !partial))) return SGNN_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_tensors; ++i) if (!grads[i] || numels[i] < 0 || (((uintptr_t)grads[i]) & 3)) return SGNN_ERR_BAD_ARG;
    int64_t base = 0;
    for (int64_t from = 0; from < n_tensors; from += OPT_MAXT) {
        const int64_t to = from + OPT_MAXT < n_tensors ? from + OPT_MAXT : n_tensors;
        OptTensors T;
        const int blocks = opt_fill(T, nullptr, (float* const*)grads, nullptr, nullptr, numels, nullptr, counter_slots, from, to);
        hipLaunchKernelGGL(optim_sumsq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, T, partial + base, step_counters);
        SGNN_CHECK_LAUNCH();
        base += blocks;
    }
    return SGNN_OK;
}

extern "C" int sgnn_optim_count(int64_t* step_counters, const int64_t* counter_slots, int64_t n_tensors, void* stream)
{
    if (n_tensors < 0 || (n_tensors && !step_counters)) return SGNN_ERR_BAD_ARG;
    for (int64_t from = 0; from < n_tensors; from += OPT_MAXT) {
        OptSlots S;
        S.count = (int)(n_tensors - from < OPT_MAXT ? n_tensors - from : OPT_MAXT);
        for (int k = 0; k < S.count; ++k) S.slot[k] = (int)(counter_slots ? counter_slots[from + k] : from + k);
        hipLaunchKernelGGL(optim_count_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, step_counters, S);
        SGNN_CHECK_LAUNCH();
    }
    return SGNN_OK;
}

template <bool EMA>
static int optim_adam(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, float lr, const float* lr_table,
                      int64_t lr_len, float beta1, float beta2, float eps, const int64_t* steps, const int64_t* step_counters,
                      const int64_t* counter_slots, const int64_t* row_lens, unsigned char* const* row_seen,
                      const float* partial, int64_t n_partial, float max_norm, float* coef_out, float* const* ema, float ema_decay,
                      int ema_warmup, void* stream)
{
    constexpr int MAXT = EMA ? OPT_EMA_MAXT : OPT_MAXT;
    if (n_tensors < 0 || (n_tensors && (!params || !grads || !exp_avg || !exp_avg_sq || !numels))) return SGNN_ERR_BAD_ARG;
    if (EMA && ((n_tensors && !ema) || !(ema_decay >= 0.f && ema_decay < 1.f))) return SGNN_ERR_BAD_ARG;
    if ((steps == nullptr) == (step_counters == nullptr) && n_tensors) return SGNN_ERR_BAD_ARG;      // exactly one of the two
    if (max_norm > 0.f && (!partial || n_partial < 0 || n_partial > 0x7fffffffll)) return SGNN_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || numels[i] < 0 || (steps && steps[i] < 1)) return SGNN_ERR_BAD_ARG;
        if ((((uintptr_t)params[i]) | ((uintptr_t)grads[i]) | ((uintptr_t)exp_avg[i]) | ((uintptr_t)exp_avg_sq[i])) & 3) return SGNN_ERR_BAD_ARG;
        if (EMA && (!ema[i] || (((uintptr_t)ema[i]) & 3))) return SGNN_ERR_BAD_ARG;
    }
    int64_t from = 0;
    bool first = true;
    while (from < n_tensors) {
        int64_t to = from + 1;                     // a launch = up to MAXT consecutive tensors with the same host step count
        while (to < n_tensors && to - from < MAXT && (!steps || steps[to] == steps[from])) ++to;
        typename OptArgs<EMA>::type T;
        const int blocks = opt_fill(T, params, grads, exp_avg, exp_avg_sq, numels, zero_grad, counter_slots, from, to);
        if constexpr (EMA) {
            for (int64_t i = from; i < to; ++i) T.e[i - from] = ema[i];
            T.ema_decay = ema_decay; T.ema_warmup = ema_warmup;
        }
        for (int64_t i = from; i < to && row_lens && row_seen && T.rows_t < 0; ++i) {
            const int64_t D = row_lens[i];
            if (!row_seen[i] || D < 4 || D > 256 || (D & (D - 1)) != 0 || numels[i] % D != 0) continue;      // 1..64 float4 lanes per row
            if ((((uintptr_t)params[i]) | ((uintptr_t)grads[i]) | ((uintptr_t)exp_avg[i]) | ((uintptr_t)exp_avg_sq[i])) & 15) continue;
            if (EMA && (((uintptr_t)ema[i]) & 15)) continue;
            T.rows_t = (int)(i - from); T.row_lanes = (int)(D / 4); T.seen = row_seen[i];
        }
        hipLaunchKernelGGL(optim_adam_kernel<EMA>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, T, partial, (int)n_partial, max_norm,
                           first ? coef_out : nullptr, lr, beta1, beta2, eps, (long long)(steps ? steps[from] : 0), step_counters,
                           lr_table, (long long)lr_len);
        SGNN_CHECK_LAUNCH();
        first = false;
        from = to;
    }
    return SGNN_OK;
}

extern "C" int sgnn_optim_adam(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                               const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, float lr, float beta1, float beta2,
                               float eps, const int64_t* steps, const int64_t* step_counters, const int64_t* counter_slots,
                               const int64_t* row_lens, unsigned char* const* row_seen,
                               const float* partial, int64_t n_partial, float max_norm, float* coef_out, void* stream)
{
    return optim_adam<false>(params, grads, exp_avg, exp_avg_sq, numels, zero_grad, n_tensors, lr, nullptr, 0, beta1, beta2, eps, steps,
                             step_counters, counter_slots, row_lens, row_seen, partial, n_partial, max_norm, coef_out, nullptr, 0.f, 0,
                             stream);
}

extern "C" int sgnn_optim_adam_lr_table(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                        const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, const float* lr_table,
                                        int64_t lr_len, float beta1, float beta2, float eps, const int64_t* steps,
                                        const int64_t* step_counters, const int64_t* counter_slots, const int64_t* row_lens,
                                        unsigned char* const* row_seen, const float* partial, int64_t n_partial, float max_norm,
                                        float* coef_out, void* stream)
{
    if (!lr_table || lr_len < 1 || (((uintptr_t)lr_table) & 3)) return SGNN_ERR_BAD_ARG;
    return optim_adam<false>(params, grads, exp_avg, exp_avg_sq, numels, zero_grad, n_tensors, 0.f, lr_table, lr_len, beta1, beta2, eps,
                             steps, step_counters, counter_slots, row_lens, row_seen, partial, n_partial, max_norm, coef_out, nullptr,
                             0.f, 0, stream);
}

extern "C" int sgnn_optim_adam_ema(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                   const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, float lr, float beta1,
                                   float beta2, float eps, const int64_t* steps, const int64_t* step_counters,
                                   const int64_t* counter_slots, const int64_t* row_lens, unsigned char* const* row_seen,
                                   const float* partial, int64_t n_partial, float max_norm, float* coef_out, float* const* ema,
                                   float ema_decay, int ema_warmup, void* stream)
{
    return optim_adam<true>(params, grads, exp_avg, exp_avg_sq, numels, zero_grad, n_tensors, lr, nullptr, 0, beta1, beta2, eps, steps,
                            step_counters, counter_slots, row_lens, row_seen, partial, n_partial, max_norm, coef_out, ema, ema_decay,
                            ema_warmup, stream);
}

extern "C" int sgnn_optim_adam_ema_lr_table(float* const* params, float* const* grads, float* const* exp_avg,
                                            float* const* exp_avg_sq, const int64_t* numels, const int32_t* zero_grad,
                                            int64_t n_tensors, const float* lr_table, int64_t lr_len, float beta1, float beta2,
                                            float eps, const int64_t* steps, const int64_t* step_counters,
                                            const int64_t* counter_slots, const int64_t* row_lens, unsigned char* const* row_seen,
                                            const float* partial, int64_t n_partial, float max_norm, float* coef_out,
                                            float* const* ema, float ema_decay, int ema_warmup, void* stream)
{
    if (!lr_table || lr_len < 1 || (((uintptr_t)lr_table) & 3)) return SGNN_ERR_BAD_ARG;
    return optim_adam<true>(params, grads, exp_avg, exp_avg_sq, numels, zero_grad, n_tensors, 0.f, lr_table, lr_len, beta1, beta2, eps,
                            steps, step_counters, counter_slots, row_lens, row_seen, partial, n_partial, max_norm, coef_out, ema,
                            ema_decay, ema_warmup, stream);
}


// ---- exchange two lists of tensors in place ---------------------------------------------------------------------------------
// a[i] <-> b[i], numels[i] floats each: how the weight averages get under a recorded validation forward, which reads the
// parameters' own storage (optim.ClipAdam.swap_ema).  No temporary: every element is read from both sides and written to both
// by the one lane that owns it.  float4 where both pointers of a pair are 16-byte aligned (+ a scalar tail), scalar otherwise.
#define SWAP_MAXT 128
struct SwapTensors {
    float* a[SWAP_MAXT]; float* b[SWAP_MAXT];
    long long n[SWAP_MAXT];
    int blk[SWAP_MAXT + 1];
    int count;
};
static_assert(sizeof(SwapTensors) + 256 <= 4096, "SwapTensors outgrew the kernel-argument segment");

__global__ __launch_bounds__(256) void optim_swap_kernel(const SwapTensors T)
{
    const int b = blockIdx.x, t = opt_find(T, b), nb = T.blk[t + 1] - T.blk[t];
    float* __restrict__ x = T.a[t]; float* __restrict__ y = T.b[t];
    const int64_t n = T.n[t];
    const int64_t first = (int64_t)(b - T.blk[t]) * 256 + threadIdx.x, stride = (int64_t)nb * 256;
    if (((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        float4* x4 = (float4*)x; float4* y4 = (float4*)y;
        for (int64_t i = first; i < n4; i += stride) { const float4 u = x4[i], w = y4[i]; x4[i] = w; y4[i] = u; }
        if (b == T.blk[t] && (int64_t)threadIdx.x < n - n4 * 4) {
            const int64_t i = n4 * 4 + threadIdx.x;
            const float u = x[i], w = y[i]; x[i] = w; y[i] = u;
        }
    } else {
        for (int64_t i = first; i < n; i += stride) { const float u = x[i], w = y[i]; x[i] = w; y[i] = u; }
    }
}

extern "C" int sgnn_optim_swap(float* const* a, float* const* b, const int64_t* numels, int64_t n_tensors, void* stream)
{
    if (n_tensors < 0 || (n_tensors && (!a || !b || !numels))) return SGNN_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (numels[i] < 0 || (numels[i] && (!a[i] || !b[i])) || ((((uintptr_t)a[i]) | ((uintptr_t)b[i])) & 3)) return SGNN_ERR_BAD_ARG;
        // (two tensors that overlap without being the same one cannot be exchanged; the same one is its own exchange)
        const uintptr_t lo = (uintptr_t)a[i], hi = (uintptr_t)b[i], len = (uintptr_t)numels[i] * 4;
        if (lo != hi && lo < hi + len && hi < lo + len) return SGNN_ERR_BAD_ARG;
    }
    for (int64_t from = 0; from < n_tensors; from += SWAP_MAXT) {
        const int64_t to = from + SWAP_MAXT < n_tensors ? from + SWAP_MAXT : n_tensors;
        SwapTensors T;
        int blocks = 0, k = 0;
        for (int64_t i = from; i < to; ++i) {
            if (numels[i] == 0 || a[i] == b[i]) continue;
            T.a[k] = a[i]; T.b[k] = b[i]; T.n[k] = numels[i]; T.blk[k] = blocks;
            blocks += opt_blocks(numels[i]);
            ++k;
        }
        if (k == 0) continue;
        T.count = k; T.blk[k] = blocks;
        hipLaunchKernelGGL(optim_swap_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, T);
        SGNN_CHECK_LAUNCH();
    }
    return SGNN_OK;
}

SGNN_DEFINE_WARM(optim)

// The loss terms shared by the fused head (head.hip) and the stand-alone loss pairs (loss.hip): every per-element formula of
// nn.CrossEntropyLoss / nn.BCEWithLogitsLoss (SubGNN.py:133) and of their weighted, smoothed and focal forms is written here
// once, so that the head and the pair compute the same term to the bit.  The callers keep what differs between them: where the
// logits and the weight rows live, the partial sums, the divisor and the order of the additions.
//
// Compile-time axes, as on the kernel bodies: WT (class weights: the rows are read), SH (0: plain, 1: label smoothing eps,
// single-label only, 2: focal gamma; SH > 0 implies WT).  A weight row reaches a function through LossRow: <false> reads it
// unconditionally (the head's LDS rows, the pair's WT = 1, SH = 0 single-label kernels), <true> lets an absent row stand as ones.
//
// Single-label, a counted row (label y in [0, K)) with lse = log sum_k exp x_k, p_k = exp(x_k - lse), w = the class weights (1 in
// the bare kernels); D = the sum of the counted rows' w_y is the divisor, g the incoming gradient, scale = g / D:
//   plain      row loss w_y (lse - x_y); gradient (p_k - [k == y]) scale w_y
//   smoothing  row loss (1 - eps) w_y (lse - x_y) + (eps / K) sum_k w_k (lse - x_k); gradient [(1 - eps) w_y (p_k - [k == y]) +
//              (eps / K) (W p_k - w_k)] scale with W = sum_j w_j (the caller adds it once per workgroup in a fixed order)
//   focal      lp = x_y - lse, q = -expm1(lp): row loss w_y q^gamma (-lp); gradient w_y f (p_k - [k == y]) scale with
//              f = q^gamma (1 - gamma p_t lp / q), and loss = f = 0 at q = 0 (lp / q is of order 1: nothing overflows)
// Multi-label, an element x against its 0/1 target y, c = weight_k, L = 1 + (pos_weight_k - 1) y, e = exp(-|x|) (exp of a
// non-positive argument only: nothing overflows), scale = g / (B K):
//   plain      loss max(x, 0) - x y + log1p(e); gradient (sigmoid(x) - y) scale
//   weighted   loss c [(1 - y) x + L (log1p(e) + max(-x, 0))]; gradient c [(1 - y) - L sigmoid(-x)] scale
//   focal      z = x for a positive, -x for a negative, l = log1p(e) + max(-z, 0), q = sigmoid(-z), p_t = sigmoid(z), both from e:
//              loss c L q^gamma l; gradient -+ c L q^gamma (q + gamma p_t l) scale
//   hit        a row is a hit when 1 / (1 + exp(-x)) > 0.5 (float32, as torch.sigmoid(x) > 0.5 evaluates it: NOT x > 0) equals
//              y in every column
#pragma once
#include "common.h"

#define SGNN_CE_IGNORE_INDEX (-100ll)

struct LossShape { float eps, gamma; };                     // label smoothing | focal exponent (SH picks which one is read)

// label_smoothing in [0, 1) (single-label only), focal_gamma finite and >= 0, at most one of them non-zero
static inline bool loss_shape_ok(bool ml, float eps, float gamma)
{
    return eps >= 0.f && eps < 1.f && gamma >= 0.f && gamma <= 3.0e38f && !(eps > 0.f && gamma > 0.f) && !(ml && eps > 0.f);
}

// a row of K class weights, in LDS or global memory; NULLABLE: an absent row stands as ones, otherwise it is read unconditionally
template <bool NULLABLE>
struct LossRow {
    const float* w;
    __device__ __forceinline__ float operator()(int64_t k) const { return (NULLABLE && !w) ? 1.f : w[k]; }
};

// q^gamma of the focal losses, q in [0, 1]: exactly 0 at q = 0
__device__ __forceinline__ float loss_qpow(float q, float gamma) { return q > 0.f ? powf(q, gamma) : 0.f; }

// sigmoid that cannot overflow: exp of a non-positive argument only
__device__ __forceinline__ float loss_sigmoid(float x)
{
    const float e = expf(x >= 0.f ? -x : x);
    return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// log-sum-exp of a row of K logits; am = its first maximum, as argmax
__device__ __forceinline__ float loss_lse_argmax(const float* x, int K, int& am)
{
    float m = x[0];
    am = 0;
    for (int k = 1; k < K; ++k) { const float v = x[k]; if (v > m) { m = v; am = k; } }
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += expf(x[k] - m);
    return m + logf(sum);
}

// single-label: the loss of a counted row; l = its log-sum-exp, wy = w[y] (1 in the bare kernels)
template <int WT, int SH, class Row>
__device__ __forceinline__ float loss_sl_row(const float* x, int K, int64_t y, float l, float wy, const Row w, const LossShape Sp)
{
    if (SH == 1) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += w(k) * (l - x[k]);
        return (1.f - Sp.eps) * wy * (l - x[y]) + (Sp.eps / (float)K) * s;
    }
    if (SH == 2) {
        const float lp = x[y] - l, q = fmaxf(-expm1f(lp), 0.f);
        return wy * loss_qpow(q, Sp.gamma) * (-lp);
    }
    return WT ? wy * (l - x[y]) : l - x[y];
}

// single-label: d loss / d x_k of a counted row; xk = that logit, xy = where the label's logit stands (focal reads it), ls = the row's
// log-sum-exp, W = sum_j w_j (SH = 1 only)
template <int WT, int SH, class Row>
__device__ __forceinline__ float loss_sl_grad(float xk, const float* xy, int K, int k, int64_t y, float ls, const Row w, float W,
                                              const LossShape Sp, float scale)
{
    const float pk = expf(xk - ls), hot = k == (int)y ? 1.f : 0.f;
    if (SH == 1) return ((1.f - Sp.eps) * w(y) * (pk - hot) + (Sp.eps / (float)K) * (W * pk - w(k))) * scale;
    if (SH == 2) {
        const float lp = *xy - ls, q = fmaxf(-expm1f(lp), 0.f);
        const float f = q > 0.f ? powf(q, Sp.gamma) * (1.f - Sp.gamma * expf(lp) * (lp / q)) : 0.f;
        return w(y) * f * (pk - hot) * scale;
    }
    float v = (pk - hot) * scale;
    if (WT) v *= w(y);
    return v;
}

// multi-label: the loss of element x of column k against target t
template <int WT, int SH, class RowC, class RowP>
__device__ __forceinline__ float loss_ml_term(float x, bool t, int k, const RowC cw, const RowP pw, const LossShape Sp)
{
    if (SH == 2) {
        const float c = cw(k), L = t ? pw(k) : 1.f;
        const float z = t ? x : -x, e = expf(-fabsf(x)), inv = 1.f / (1.f + e);
        return c * L * loss_qpow(z >= 0.f ? e * inv : inv, Sp.gamma) * (log1pf(e) + fmaxf(-z, 0.f));
    }
    if (WT) {
        const float c = cw(k), L = t ? pw(k) : 1.f;
        return c * ((t ? 0.f : x) + L * (log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f)));
    }
    return fmaxf(x, 0.f) - (t ? x : 0.f) + log1pf(expf(-fabsf(x)));
}

// multi-label: d loss / d x of that element
template <int WT, int SH, class RowC, class RowP>
__device__ __forceinline__ float loss_ml_grad(float x, bool t, int k, const RowC cw, const RowP pw, const LossShape Sp, float scale)
{
    if (SH == 2) {
        const float c = cw(k), L = t ? pw(k) : 1.f;
        const float z = t ? x : -x, e = expf(-fabsf(x)), inv = 1.f / (1.f + e), q = z >= 0.f ? e * inv : inv, pt = z >= 0.f ? inv : e * inv;
        const float g = c * L * loss_qpow(q, Sp.gamma) * (q + Sp.gamma * pt * (log1pf(e) + fmaxf(-z, 0.f))) * scale;
        return t ? -g : g;
    }
    if (WT) {
        const float c = cw(k), L = t ? pw(k) : 1.f;
        return c * ((t ? 0.f : 1.f) - L * loss_sigmoid(-x)) * scale;
    }
    return (loss_sigmoid(x) - (t ? 1.f : 0.f)) * scale;
}

// multi-label: does element x predict its target t (torch.sigmoid(x) > 0.5 in float32)
__device__ __forceinline__ bool loss_ml_hit(float x, bool t) { return (1.f / (1.f + expf(-x)) > 0.5f) == t; }

// calc_dist (reference SubGNN/gamma.py:51-52) for the DTW kernels: dtw.hip (fastdtw) and dtw_exact.hip (the whole grid).
#pragma once
#include <hip/hip_runtime.h>

__device__ static inline double dtw_cost(double a, double b) {            // gamma.py:51-52
    const double mx = a > b ? a : b, mn = a > b ? b : a;
    return (mx + 1.0) / (mn + 1.0) - 1.0;
}

// The same cost from a1 = a + 1, b1 = b + 1 and their correctly rounded reciprocals ra, rb, without
// a divide instruction sequence: q0 = RN(mx * r), rem = mx - q0 * mn (exact in an fma),
// q = RN(q0 + rem * r) is the correctly rounded quotient mx / mn when r = RN(1 / mn) (Markstein's
// division step; it can only fail for divisors whose significand is all ones, and mn is a small
// dyadic rational here).  tests/test_oracle_integer.py::test_reciprocal_division_is_exact runs the
// identity on the CPU (oracle/division_check.c): exhaustively for integers up to 3000, and on random samples -- 10^7 pairs
// (x + 1) / 2^L with x < 2^22, L <= 7, and 10^7 pairs v + 1 with v a mean of 2^L int32 values up to 2^31 - 1, L <= 15.
__device__ __forceinline__ double dtw_cost_rcp(double a1, double ra, double b1, double rb) {
    // max / min with ONE division step (round 5; rounds 2-4 formed both quotients and took the larger: 8 fp64 instructions, this
    // is 7, and every one of them issues at half rate on gfx950): mx = max(a1, b1), mn = min(a1, b1), and the correctly rounded
    // reciprocal of mn is max(ra, rb) -- rounding is monotone, so a1 <= b1 implies RN(1 / a1) >= RN(1 / b1).  The quotient is
    // then the same correctly rounded mx / mn >= 1 the larger of the two quotients was (the direction the CPU test covers).
    const double mx = fmax(a1, b1), mn = fmin(a1, b1), r = fmax(ra, rb);
    const double q0 = __dmul_rn(mx, r);
    const double q = __fma_rn(__fma_rn(-q0, mn, mx), r, q0);
    return __dadd_rn(q, -1.0);
}

/* Test infrastructure (see oracle/__init__.py): checks on the CPU that the reciprocal-multiply
 * quotient the register DTW kernels use (subgnn_amd/csrc/dtw_cost.h: dtw_cost_rcp) is the
 * correctly rounded IEEE-754 quotient -- i.e. bit-identical to the `/` of the reference's
 * gamma.calc_dist (SubGNN/gamma.py:51-52) -- over the operands those kernels can meet: value + 1 for
 * degrees and their pairwise averages (dyadic rationals).
 *   q0 = RN(mx * r); rem = fma(-q0, mn, mx); q = fma(rem, r, q0)   with r = RN(1 / mn)
 * The quotient is checked both as max / min directly and as the larger of a / b and b / a (the form the kernel
 * had before it took max(ra, rb) as the reciprocal of min(a, b)): either must be the IEEE quotient max / min.
 * What is checked:
 *   1. EXHAUSTIVELY, every pair of integers 1 <= b <= a <= max_int (3000 in the test);
 *   2. n_random random pairs (x + 1) / 2^L, x < 2^22, L <= 7 (both operands of a pair on the same level L);
 *   3. n_wide random pairs v + 1 with v = m / 2^L, L <= 15 (DTW_MAX_LEVELS is 16: a series is halved at most 15
 *      times), m drawn so that v lies in [0, 2^w - 1] for a width w of 22..31 bits drawn per operand: the means of
 *      2^L int32 values up to 2^31 - 1, formed as the kernel forms them (v + 1.0, 1.0 / (v + 1.0)).
 * Parts 2 and 3 are samples, not proofs.
 * usage: division_check <max_int> <n_random> [<n_wide>]     prints "checked <count>" and "bad <count>" */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static inline double rcp_div(double mx, double mn, double r)
{
    const double q0 = mx * r;
    const double rem = fma(-q0, mn, mx);
    return fma(rem, r, q0);
}

static inline uint64_t next(uint64_t* s)
{
    *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17;
    return *s;
}

int main(int argc, char** argv)
{
    const int max_int = argc > 1 ? atoi(argv[1]) : 3000;
    const long n_random = argc > 2 ? atol(argv[2]) : 10000000L;
    const long n_wide = argc > 3 ? atol(argv[3]) : 0L;
    long bad = 0, n = 0;
    for (int b = 1; b <= max_int; ++b) {
        const double db = b, r = 1.0 / db;
        for (int a = b; a <= max_int; ++a, ++n) {
            const double da = a;
            if (rcp_div(da, db, r) != da / db) ++bad;
            if (fmax(rcp_div(da, db, r), rcp_div(db, da, 1.0 / da)) != da / db) ++bad;
        }
    }
    uint64_t s = 88172645463325252ull;
    for (long i = 0; i < n_random; ++i, ++n) {
        next(&s);
        const uint32_t x = (uint32_t)s & 0x3fffff, y = (uint32_t)(s >> 32) & 0x3fffff;      /* up to 2^22 */
        const int L = (int)((s >> 59) & 7);                                                  /* halved up to 7 times */
        double a = (double)(x + 1) / (double)(1 << L), b = (double)(y + 1) / (double)(1 << L);
        if (a < b) { const double t = a; a = b; b = t; }
        if (rcp_div(a, b, 1.0 / b) != a / b) ++bad;
        if (fmax(rcp_div(a, b, 1.0 / b), rcp_div(b, a, 1.0 / a)) != a / b) ++bad;
    }
    for (long i = 0; i < n_wide; ++i, ++n) {
        const uint64_t c = next(&s);
        const int L = (int)(c & 15);                                                         /* halved up to 15 times */
        const int wa = 22 + (int)((c >> 4) & 15) % 10, wb = 22 + (int)((c >> 8) & 15) % 10;   /* 22..31 bits */
        /* m in [0, (2^w - 1) 2^L]: at most 46 bits, exact in a double, and so are m / 2^L and m / 2^L + 1 */
        const uint64_t ma = next(&s) % ((((uint64_t)1 << wa) - 1) * ((uint64_t)1 << L) + 1);
        const uint64_t mb = next(&s) % ((((uint64_t)1 << wb) - 1) * ((uint64_t)1 << L) + 1);
        double a = (double)ma / (double)(1 << L) + 1.0, b = (double)mb / (double)(1 << L) + 1.0;
        if (a < b) { const double t = a; a = b; b = t; }
        if (rcp_div(a, b, 1.0 / b) != a / b) ++bad;
        if (fmax(rcp_div(a, b, 1.0 / b), rcp_div(b, a, 1.0 / a)) != a / b) ++bad;
    }
    printf("checked %ld\nbad %ld\n", n, bad);
    return bad != 0;
}

// Structure similarity 1/(1+DTW) over the WHOLE grid (structure_similarity_fn = 'dtw_exact'): the register-resident and the
// general DP kernel.
#include "common.h"
#include "dtw_cost.h"

// ---------------------------------------------------------------------------------------------
// 1 / (1 + DTW(x, y, dist=calc_dist)), the distance fastdtw (dtw.hip) approximates:
//   D[i][j] = min(D[i-1][j], D[i][j-1], D[i-1][j-1]) + calc_dist(x[i], y[j]),   D[-1][-1] = 0, every other border cell INF.
// The value is a minimum over warp paths: no predecessor rule can change it (rounding is monotone, so the minimum of
// the three sums IS the minimum of the three predecessors plus the cost), hence no tie_order here.
//
// One lane per (x row, y row) pair, fp64.  There are no pyramids, windows, predecessor words or back-traces: a
// pre-kernel writes value + 1 and its correctly rounded reciprocal of every series entry (what dtw_cost_rcp reads), x
// transposed and in the caller's processing order so that the lanes of a wavefront read consecutive addresses, y row-major
// (read wave-uniformly).  The DP runs column-major over one column of row values that is updated in place while j walks
// the y series.
// ---------------------------------------------------------------------------------------------
#define DTWX_THREADS 256
#define DTWX_BLOCKS 256                    // general kernel: 65536 lanes, each with a column of max_x_len doubles in the workspace
#define DTWX_NT ((int64_t)DTWX_THREADS * DTWX_BLOCKS)
#define DTWX_REG_BLOCKS (256 * 32)         // register kernels: many more workgroups than fit at once (a short tail), like dtw.hip
#define DTWX_R 32                          // longest x row of the register kernels

static inline int64_t dtwx_align8(int64_t b) { return (b + 7) / 8 * 8; }

extern "C" int64_t sgnn_dtw_exact_workspace_bytes(int64_t n_x, int64_t max_x_len, int64_t n_y, int64_t max_y_len) {
    if (max_x_len < 1) max_x_len = 1;
    if (max_y_len < 1) max_y_len = 1;
    return DTWX_NT * max_x_len * 8                                         // the general kernel's columns
         + 2 * (n_x * max_x_len * 8 + n_y * max_y_len * 8)                  // value + 1 and reciprocal of both sides
         + dtwx_align8(n_x * 4) + dtwx_align8(n_y * 4);                     // lengths
}

// value + 1 and RN(1 / (value + 1)) of every entry, one thread per slot of the padded (n, M) form.
// transposed != 0: entry e of series s at out[e * n + s], else at out[s * M + e]; rec follows the same layout.
// order (nullable): position s of the output holds series order[s].
__global__ void dtw_exact_prepare_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ val, int64_t n, int64_t M,
                                         int transposed, double* __restrict__ out, double* __restrict__ rec,
                                         int32_t* __restrict__ len_out, const int32_t* __restrict__ order)
{
    const int64_t total = n * M;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = transposed ? idx % n : idx / M, e = transposed ? idx / n : idx % M;
        const int64_t src = order ? order[s] : s;
        const int64_t b = ptr[src];
        int64_t len = ptr[src + 1] - b;
        if (len > M) len = M;                                  // (the caller's max_len bounds every row; never index past it)
        if (e == 0) len_out[s] = (int32_t)len;
        if (e < len) {
            const double v1 = (double)val[b + e] + 1.0;
            out[idx] = v1;
            rec[idx] = 1.0 / v1;
        }
    }
}

// ---- general kernel: any size.  The lane's column lives in the caller's workspace, element-interleaved across lanes. ----
__global__ __launch_bounds__(DTWX_THREADS) void dtw_exact_kernel(
    const double* __restrict__ xa, const double* __restrict__ xr, const int32_t* __restrict__ xlen, int64_t n_x,
    const double* __restrict__ ya, const double* __restrict__ yr, const int32_t* __restrict__ ylen, int64_t n_y, int64_t MY,
    float* __restrict__ out, double* __restrict__ wd)
{
    const int64_t NT = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    const int64_t total = n_x * n_y;
    for (int64_t pair = tid; pair < total; pair += NT) {
        // consecutive lanes: consecutive x rows, same y row
        const int64_t a = pair / n_x, r = pair % n_x;
        const int lx = xlen[r], ly = ylen[a];
        if (lx == 0 || ly == 0) { out[r * n_y + a] = 0.f; continue; }       // PAD, as sgnn_dtw_similarity
        for (int i = 0; i < lx; ++i) wd[(int64_t)i * NT + tid] = INF;
        double up = INF;
        for (int j = 0; j < ly; ++j) {
            const double y1 = ya[a * MY + j], yrc = yr[a * MY + j];
            double diag = j == 0 ? 0.0 : INF;
            up = INF;
            for (int i = 0; i < lx; ++i) {
                const double c = dtw_cost_rcp(xa[(int64_t)i * n_x + r], xr[(int64_t)i * n_x + r], y1, yrc);
                const double old = wd[(int64_t)i * NT + tid];
                up = __dadd_rn(fmin(fmin(old, diag), up), c);
                wd[(int64_t)i * NT + tid] = up;
                diag = old;
            }
        }
        out[r * n_y + a] = (float)(1.0 / (up + 1.0));
    }
}

// ---- register-resident kernels for x rows of at most DTWX_R entries ---------------------------------------------------
// One wavefront = 64 pairs that share the y row (wave-uniform: its entries arrive through scalar loads) and hold 64
// consecutive x rows of the caller's processing order, one pair per lane.  The lane's column (RMAX doubles), its x + 1 and
// their reciprocals stay in registers; the row loop is fully unrolled (static register indexing) and leaves, in steps of
// two rows, at the longest x row of the wavefront (a scalar branch: the processing order sorts by length first).  Rows
// past a lane's own length compute values nobody reads -- a cell depends on rows above it only.
//
// KEEP (x rows of at most 20 entries): the cost column is kept in registers as well, and a column whose y value repeats
// the previous one (sorted degree sequences: 41 % of the benchmark's columns) skips the seven instructions of dtw_cost_rcp
// per cell.  y is wave-uniform and every lane evaluates every cell of a column, so the test is one scalar comparison of the
// value's bits.  The fourth array costs a wavefront per SIMD (20 rows: 179 registers, two wavefronts instead of the three
// the plain form ran at with 145) and still wins on degree sequences: 2.89 against 3.30 ms on the benchmark's external
// side, 8.3 k against 11.3 k vector instructions per 64 pairs; on series without a single repeat it loses 13 % (3.74 against
// 3.30 ms) -- DESIGN.md section 5.  Four arrays of 32 doubles are all 256 registers a wavefront can have: 21-32 rows run
// the plain form.
template <int RMAX, int MINB, bool KEEP>
__global__ __launch_bounds__(DTWX_THREADS, MINB) void dtw_exact_reg_kernel(
    const double* __restrict__ xa, const double* __restrict__ xr, const int32_t* __restrict__ xlen, int64_t n_x,
    const double* __restrict__ ya, const double* __restrict__ yr, const int32_t* __restrict__ ylen, int64_t n_y, int64_t MY,
    float* __restrict__ out, const int32_t* __restrict__ x_order, const int64_t* __restrict__ x_live)
{
    const int64_t NT = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    // x_live = {first, count}: only these positions of the processing order hold non-empty rows (the caller sorted the
    // empty ones to the front and zeroed their output rows)
    const int64_t first_live = x_live ? x_live[0] : 0;
    const int64_t n_live = x_live ? x_live[1] : n_x;
    const int64_t chunks = (n_live + 63) / 64;                // a task = one y row x 64 consecutive positions
    const int64_t n_tasks = chunks * n_y;
    const int64_t n_waves = NT / 64;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (int64_t task = wave0; task < n_tasks; task += n_waves) {
        const int64_t a = task / chunks;
        const int64_t p0 = first_live + (task - a * chunks) * 64 + lane;   // position in the processing order: the
        const bool have = p0 < first_live + n_live;                        // prepared series are laid out by position
        const int64_t pos = have ? p0 : first_live;
        const int64_t r = x_order ? x_order[pos] : pos;
        const int ly = ylen[a];
        const int lx = have ? xlen[pos] : 0;
        int lxm = lx;                                                      // longest x row of the wavefront
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(lxm, d, 64); lxm = o > lxm ? o : lxm; }
        lxm = __builtin_amdgcn_readfirstlane(lxm);
        double x1[RMAX], xrc[RMAX], col[RMAX], cst[KEEP ? RMAX : 1];
#pragma unroll
        for (int i = 0; i < RMAX; ++i) {
            x1[i] = i < lx ? xa[(int64_t)i * n_x + pos] : 1.0;             // (i < lx <= max_x_len: inside the arrays)
            xrc[i] = i < lx ? xr[(int64_t)i * n_x + pos] : 1.0;
            col[i] = INF;
        }
        const long long* __restrict__ ybits = reinterpret_cast<const long long*>(ya + a * MY);
        const double* __restrict__ yrow_r = yr + a * MY;
        long long prev_bits = 0;
        for (int j = 0; j < ly; ++j) {
            const long long yb = ybits[j];
            const double y1 = __longlong_as_double(yb), yrc = yrow_r[j];
            if constexpr (KEEP) {
                if (j == 0 || yb != prev_bits) {
#pragma unroll
                    for (int i = 0; i < RMAX; ++i) {
                        if ((i & 1) == 0 && i >= lxm) break;
                        cst[i] = dtw_cost_rcp(x1[i], xrc[i], y1, yrc);
                    }
                }
                prev_bits = yb;
            }
            double diag = j == 0 ? 0.0 : INF, up = INF;
#pragma unroll
            for (int i = 0; i < RMAX; ++i) {
                if ((i & 1) == 0 && i >= lxm) break;
                const double c = KEEP ? cst[KEEP ? i : 0] : dtw_cost_rcp(x1[i], xrc[i], y1, yrc);
                const double old = col[i];
                up = __dadd_rn(fmin(fmin(old, diag), up), c);
                col[i] = up;
                diag = old;
            }
        }
        double result = 0.0;
#pragma unroll
        for (int i = 0; i < RMAX; ++i) result = i == lx - 1 ? col[i] : result;
        if (have) out[r * n_y + a] = (lx > 0 && ly > 0) ? (float)(1.0 / (result + 1.0)) : 0.f;
    }
}

// resident 256-thread blocks per CU (= wavefronts per SIMD) each instantiation is compiled for: DESIGN.md section 5
#define DTWX_MINB12 4
#define DTWX_MINB20 2
#define DTWX_MINB32 2

// ---- the x side prepared once (as dtw.hip's sgnn_dtw_prepare_rows: same header form, its own magic) -------------------------
// device buffer: value + 1 (n_x * MX doubles), reciprocals (the same), lengths
#define DTWX_ROWS_MAGIC 0x53474e4e44545758ll      // "SGNNDTWX"
#define DTWX_ROWS_HEAD 8
enum { DTWX_ROWS_ORDERED = 1, DTWX_ROWS_NATURAL = 2 };  // the register kernels' layout (positions follow x_order) / the general kernel's

static inline int dtwx_rows_layout(int64_t MX, int kernel, const int32_t* x_order) {
    return (MX <= DTWX_R && kernel == 0 && x_order) ? DTWX_ROWS_ORDERED : DTWX_ROWS_NATURAL;
}

extern "C" int64_t sgnn_dtwx_rows_bytes(int64_t n_x, int64_t max_x_len) {
    if (max_x_len < 1) max_x_len = 1;
    if (n_x < 0) n_x = 0;
    return 2 * n_x * max_x_len * 8 + dtwx_align8(n_x * 4);
}

extern "C" int64_t sgnn_dtwx_rows_workspace_bytes(int64_t n_x, int64_t max_x_len, int64_t n_y, int64_t max_y_len) {
    return sgnn_dtw_exact_workspace_bytes(n_x, max_x_len, n_y, max_y_len) - sgnn_dtwx_rows_bytes(n_x, max_x_len);
}

static void dtw_exact_prepare_rows(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t MX, int layout,
                                   const int32_t* x_order, char* rows, hipStream_t st)
{
    double* xa = (double*)rows;
    double* xr = xa + n_x * MX;
    int32_t* xlen = (int32_t*)(rows + 2 * n_x * MX * 8);
    hipLaunchKernelGGL(dtw_exact_prepare_kernel, dim3(sgnn_grid_for(n_x * MX, 256)), dim3(256), 0, st, x_ptr, x_val, n_x, MX, 1,
                       xa, xr, xlen, layout == DTWX_ROWS_ORDERED ? x_order : (const int32_t*)nullptr);
}

extern "C" int sgnn_dtwx_prepare_rows(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len, int kernel,
                                           const int32_t* x_order, void* rows, int64_t rows_bytes, int64_t* header, void* stream)
{
    if (!x_ptr || !x_val || !rows || !header || n_x < 0 || kernel < 0 || kernel > 1) return SGNN_ERR_BAD_ARG;
    if (max_x_len < 1) max_x_len = 1;
    if (max_x_len > 32767) return SGNN_ERR_SET_TOO_LARGE;
    if (rows_bytes < sgnn_dtwx_rows_bytes(n_x, max_x_len)) return SGNN_ERR_BAD_ARG;
    const int layout = dtwx_rows_layout(max_x_len, kernel, x_order);
    header[0] = 0;                                       // (not valid until the launch has been queued)
    if (n_x > 0) {
        dtw_exact_prepare_rows(x_ptr, x_val, n_x, max_x_len, layout, x_order, (char*)rows, (hipStream_t)stream);
        SGNN_CHECK_LAUNCH();
    }
    header[1] = layout; header[2] = n_x; header[3] = max_x_len; header[4] = (int64_t)(intptr_t)rows; header[5] = rows_bytes;
    header[6] = header[7] = 0;
    header[0] = DTWX_ROWS_MAGIC;
    return SGNN_OK;
}

// the y side + the DP launch over prepared x rows.  ``workspace``: the general kernel's columns, y values, y reciprocals, y lengths
static int dtw_exact_run_rows(const char* rows, int64_t n_x, int64_t MX, const int64_t* y_ptr, const int32_t* y_val, int64_t n_y,
                              int64_t MY, int kernel, const int32_t* x_order, const int64_t* x_live, float* out, void* workspace,
                              hipStream_t st)
{
    char* w = (char*)workspace;
    double* wd = (double*)w;               w += DTWX_NT * MX * 8;
    double* ya = (double*)w;               w += n_y * MY * 8;
    double* yr = (double*)w;               w += n_y * MY * 8;
    int32_t* ylen = (int32_t*)w;
    const double* xa = (const double*)rows;
    const double* xr = xa + n_x * MX;
    const int32_t* xlen = (const int32_t*)(rows + 2 * n_x * MX * 8);
    const bool use_reg = MX <= DTWX_R && kernel == 0;
    hipLaunchKernelGGL(dtw_exact_prepare_kernel, dim3(sgnn_grid_for(n_y * MY, 256)), dim3(256), 0, st, y_ptr, y_val, n_y, MY, 0,
                       ya, yr, ylen, (const int32_t*)nullptr);
    SGNN_CHECK_LAUNCH();
    if (use_reg) {
#define DTWX_LAUNCH(RMAX, MINB, KEEP) \
        hipLaunchKernelGGL((dtw_exact_reg_kernel<RMAX, MINB, KEEP>), dim3(DTWX_REG_BLOCKS), dim3(DTWX_THREADS), 0, st, \
                           xa, xr, xlen, n_x, ya, yr, ylen, n_y, MY, out, x_order, x_live)
        if (MX <= 12) DTWX_LAUNCH(12, DTWX_MINB12, true);
        else if (MX <= 20) DTWX_LAUNCH(20, DTWX_MINB20, true);
        else DTWX_LAUNCH(32, DTWX_MINB32, false);
#undef DTWX_LAUNCH
    } else {
        hipLaunchKernelGGL(dtw_exact_kernel, dim3(DTWX_BLOCKS), dim3(DTWX_THREADS), 0, st, xa, xr, xlen, n_x, ya, yr, ylen, n_y, MY,
                           out, wd);
    }
    SGNN_CHECK_LAUNCH();
    return SGNN_OK;
}

static int dtw_exact_run(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len,
                         const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                         int kernel, const int32_t* x_order, const int64_t* x_live, float* out, void* workspace,
                         int64_t workspace_bytes, void* stream)
{
    if (!x_ptr || !x_val || !y_ptr || !y_val || !out || !workspace || n_x < 0 || n_y < 0) return SGNN_ERR_BAD_ARG;
    if (kernel < 0 || kernel > 1) return SGNN_ERR_BAD_ARG;
    if (max_x_len < 1) max_x_len = 1;
    if (max_y_len < 1) max_y_len = 1;
    if (max_x_len > 32767 || max_y_len > 32767) return SGNN_ERR_SET_TOO_LARGE;
    if (workspace_bytes < sgnn_dtw_exact_workspace_bytes(n_x, max_x_len, n_y, max_y_len)) return SGNN_ERR_BAD_ARG;
    if (n_x * n_y == 0) return SGNN_OK;
    // the x rows prepared into the tail of the per-call workspace, then the one launch path
    char* rows = (char*)workspace + sgnn_dtwx_rows_workspace_bytes(n_x, max_x_len, n_y, max_y_len);
    dtw_exact_prepare_rows(x_ptr, x_val, n_x, max_x_len, dtwx_rows_layout(max_x_len, kernel, x_order), x_order, rows,
                           (hipStream_t)stream);
    SGNN_CHECK_LAUNCH();
    return dtw_exact_run_rows(rows, n_x, max_x_len, y_ptr, y_val, n_y, max_y_len, kernel, x_order, x_live, out, workspace,
                              (hipStream_t)stream);
}

static int dtw_exact_run_prepared(const int64_t* header, int64_t n_x, int64_t max_x_len,
                                  const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                  int kernel, const int32_t* x_order, const int64_t* x_live, float* out, void* workspace,
                                  int64_t workspace_bytes, void* stream)
{
    if (!header || !y_ptr || !y_val || !out || !workspace || n_x < 0 || n_y < 0) return SGNN_ERR_BAD_ARG;
    if (kernel < 0 || kernel > 1) return SGNN_ERR_BAD_ARG;
    if (max_x_len < 1) max_x_len = 1;
    if (max_y_len < 1) max_y_len = 1;
    if (max_x_len > 32767 || max_y_len > 32767) return SGNN_ERR_SET_TOO_LARGE;
    if (header[0] != DTWX_ROWS_MAGIC || header[2] != n_x || header[3] != max_x_len || !header[4]) return SGNN_ERR_BAD_ARG;
    if (header[1] != dtwx_rows_layout(max_x_len, kernel, x_order)) return SGNN_ERR_BAD_ARG;
    if (header[5] < sgnn_dtwx_rows_bytes(n_x, max_x_len)) return SGNN_ERR_BAD_ARG;
    if (workspace_bytes < sgnn_dtwx_rows_workspace_bytes(n_x, max_x_len, n_y, max_y_len)) return SGNN_ERR_BAD_ARG;
    if (n_x * n_y == 0) return SGNN_OK;
    return dtw_exact_run_rows((const char*)(intptr_t)header[4], n_x, max_x_len, y_ptr, y_val, n_y, max_y_len, kernel, x_order, x_live,
                              out, workspace, (hipStream_t)stream);
}

extern "C" int sgnn_dtw_exact_similarity(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len,
                                         const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                         int kernel, const int32_t* x_order, float* out, void* workspace,
                                         int64_t workspace_bytes, void* stream)
{
    return dtw_exact_run(x_ptr, x_val, n_x, max_x_len, y_ptr, y_val, n_y, max_y_len, kernel, x_order, nullptr, out, workspace,
                         workspace_bytes, stream);
}

extern "C" int sgnn_dtw_exact_similarity_live(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len,
                                              const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                              int kernel, const int32_t* x_order, const int64_t* x_live_range, float* out,
                                              void* workspace, int64_t workspace_bytes, void* stream)
{
    if (x_live_range && !x_order) return SGNN_ERR_BAD_ARG;
    return dtw_exact_run(x_ptr, x_val, n_x, max_x_len, y_ptr, y_val, n_y, max_y_len, kernel, x_order, x_live_range, out,
                         workspace, workspace_bytes, stream);
}

extern "C" int sgnn_dtwx_similarity_rows(const int64_t* rows_header, int64_t n_x, int64_t max_x_len,
                                              const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                              int kernel, const int32_t* x_order, float* out, void* workspace,
                                              int64_t workspace_bytes, void* stream)
{
    return dtw_exact_run_prepared(rows_header, n_x, max_x_len, y_ptr, y_val, n_y, max_y_len, kernel, x_order, nullptr, out,
                                  workspace, workspace_bytes, stream);
}

extern "C" int sgnn_dtwx_similarity_rows_live(const int64_t* rows_header, int64_t n_x, int64_t max_x_len,
                                                   const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                                   int kernel, const int32_t* x_order, const int64_t* x_live_range, float* out,
                                                   void* workspace, int64_t workspace_bytes, void* stream)
{
    if (x_live_range && !x_order) return SGNN_ERR_BAD_ARG;
    return dtw_exact_run_prepared(rows_header, n_x, max_x_len, y_ptr, y_val, n_y, max_y_len, kernel, x_order, x_live_range, out,
                                  workspace, workspace_bytes, stream);
}

SGNN_DEFINE_WARM(dtw_exact)

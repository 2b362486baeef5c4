// gaussian.hip -- the score of "Instance Selection for GANs" (scripts/data_scripts/run_instance_selection.py of the reference: one full-covariance
// Gaussian fitted to the detector features, every row scored by its log-likelihood) on the device: the Mahalanobis part.
//
// Replaces (scikit-learn on host arrays, float32 throughout for float32 features):
//   run_instance_selection.py:29-33   GaussianMixture(1).fit(X).score_samples(X): ((X - mu) @ precisions_chol)^2 summed per row
//
// maha[i] = sum_j ( sum_{k <= j} (rows[i,k] - mu[k]) P[k,j] )^2 with P upper triangular (the precision Cholesky factor L^-T, L L^T = Sigma).
//
// Contract (include/tdgp.h): every row value widened fp32 -> fp64 (exact), d = x - mu rounded once in fp64, the contraction on
// v_mfma_f64_16x16x4_f64 with fp64 accumulation, squares and their sums in fp64; nothing held in fp32; P is never read below its diagonal;
// no atomics, one writer per value; a row's result is a fixed function of that row, mu, P and F.
//
//   gm_tile            one 64-row x 64-column tile of y = d P: 4 waves as 2 x 2, each 32 x 32 = 2 x 2 MFMA tiles (32 accumulator registers).
//                      K loop over k < min(F, 64 (tj + 1)) -- the zero half of the triangle is never visited -- 32 per step: the rows' strip
//                      staged as fp32 ([row][k], 34-float rows: the 16 x 2 fragment reads of a wave half fall on 32 distinct banks), mu's strip
//                      and P's strip as fp64 ([k][column], 80-double rows: the two k rows of a wave half fall on opposite halves of the bank
//                      row), through registers into two LDS buffers, one barrier per step; d is formed at the fragment read.  Elements of P
//                      with k > j, and everything past n or F, are staged as zeros without a load.  Then y^2, the two MFMA tiles of a lane
//                      added, a butterfly over the 16 lanes of a row, the two column waves added through LDS: q_t of the 64 rows, the same
//                      order of additions for every position a row can take in a tile.
//   gm_direct_kernel   block = one row tile; walks the column tiles in order: total = q_0, total += q_1, ...
//   gm_split_kernel    block = one (row tile, column tile): workspace[tj][row] = q_tj;  gm_merge_kernel adds them in the same order.
#include "common.h"
#include <algorithm>

namespace {

constexpr int GM_T = 64;                             // tile edge, rows and columns
constexpr int GM_C = 32;                             // k per step
constexpr int GM_LDA = 34;                           // floats per staged row of `rows`
constexpr int GM_LDB = 80;                           // doubles per staged k row of P
constexpr int GM_THREADS = 256;
constexpr int GM_DIRECT_TILES = 512;                 // this many row tiles fill the device (256 CUs x 2 resident blocks) on their own
constexpr int GM_MAX_F = 16384;
constexpr int64_t GM_MAX_N = (int64_t)1 << 31;

struct GmPlan { int t1; int64_t row_tiles; bool split; };

inline bool gm_shape_ok(int64_t n, int F) { return n >= 0 && n < GM_MAX_N && F >= 1 && F <= GM_MAX_F; }
inline GmPlan gm_plan(int64_t n, int F) {
    GmPlan p;
    p.t1 = cdiv(F, GM_T);
    p.row_tiles = cdiv64(n, GM_T);
    p.split = p.t1 > 1 && p.row_tiles < GM_DIRECT_TILES;       // one column tile has nothing to split
    return p;
}

struct GmShared {
    float a[2][GM_T * GM_LDA];
    double b[2][GM_C * GM_LDB];
    double mu[2][GM_C];
    double red[2][GM_T];
};

// q of rows i0 .. i0 + 63 for column tile tj; on return thread t < 64 holds q of row i0 + t (rows past n: unspecified, never stored).
// To be reached by the whole block; ends behind a barrier only for the staging buffers, `red` is safe until the next call's first barrier.
__device__ __forceinline__ double gm_tile(GmShared& sh, const float* __restrict__ rows, int64_t n, int F, const double* __restrict__ mu,
                                          const double* __restrict__ P, int64_t i0, int tj) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wi = w >> 1, wj = w & 1, lc = lane & 15, lk = lane >> 4;
    const int j0 = tj * GM_T;
    const int kend = min(F, j0 + GM_T);
    const int ksteps = (kend + GM_C - 1) / GM_C;

    // staging: thread t moves k (t & 31) of rows (t >> 5) + 8 i, column (t & 63) of P's k rows (t >> 6) + 4 i, and (t < 32) mu[k]
    const int ak = t & 31, ar = t >> 5, bj = t & 63, bk = t >> 6;
    const bool jin = j0 + bj < F;
    float ra[GM_T / 8];
    double rb[GM_C / 4], rm = 0.0;
    auto fetch = [&](int ks) {
        const int k0 = ks * GM_C;
        const bool kin = k0 + ak < F;
#pragma unroll
        for (int i = 0; i < GM_T / 8; i++) {
            const int64_t r = i0 + ar + 8 * i;
            ra[i] = kin && r < n ? rows[r * F + k0 + ak] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < GM_C / 4; i++) {
            const int k = k0 + bk + 4 * i;
            rb[i] = jin && k <= j0 + bj ? P[(int64_t)k * F + j0 + bj] : 0.0;          // k <= j < F: on or above the diagonal, inside the matrix
        }
        if (t < GM_C) rm = k0 + t < F ? mu[k0 + t] : 0.0;
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int i = 0; i < GM_T / 8; i++) sh.a[buf][(ar + 8 * i) * GM_LDA + ak] = ra[i];
#pragma unroll
        for (int i = 0; i < GM_C / 4; i++) sh.b[buf][(bk + 4 * i) * GM_LDB + bj] = rb[i];
        if (t < GM_C) sh.mu[buf][t] = rm;
    };

    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[a][b][e] = 0.0;

    fetch(0);
    put(0);
    __syncthreads();
    for (int ks = 0; ks < ksteps; ks++) {
        const int cur = ks & 1;
        const bool more = ks + 1 < ksteps;                                      // block-uniform
        if (more) fetch(ks + 1);
        const float* const A = sh.a[cur];
        const double* const B = sh.b[cur];
        const double* const M = sh.mu[cur];
#pragma unroll
        for (int kk = 0; kk < GM_C / 4; kk++) {
            const int kq = kk * 4 + lk;
            const double m = M[kq];
            double fa[2], fb[2];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                fa[s] = (double)A[(wi * 32 + s * 16 + lc) * GM_LDA + kq] - m;
                fb[s] = B[kq * GM_LDB + wj * 32 + s * 16 + lc];
            }
            mfma_f64_2x2(fa, fb, acc);
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }

    // the wave's output starts at row i0 + wi*32, column j0 + wj*32 (element map: common.h)
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double y0 = acc[a][0][e], y1 = acc[a][1][e];
            double s = y0 * y0 + y1 * y1;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) s += shfl_xor_f64(s, d);           // x + y on both sides of a pair: the 16 lanes end with the same bits
            if (lc == 0) sh.red[wj][wi * 32 + a * 16 + lk + 4 * e] = s;
        }
    __syncthreads();
    return t < GM_T ? sh.red[0][t] + sh.red[1][t] : 0.0;
}

__global__ __launch_bounds__(GM_THREADS) void gm_direct_kernel(const float* __restrict__ rows, int64_t n, int F, int t1, const double* __restrict__ mu,
                                                               const double* __restrict__ P, double* __restrict__ maha) {
    __shared__ __attribute__((aligned(16))) GmShared sh;
    const int64_t i0 = (int64_t)blockIdx.x * GM_T;
    double total = 0.0;
    for (int tj = 0; tj < t1; tj++) {
        const double q = gm_tile(sh, rows, n, F, mu, P, i0, tj);
        total = tj == 0 ? q : total + q;
    }
    if (threadIdx.x < GM_T && i0 + threadIdx.x < n) maha[i0 + threadIdx.x] = total;
}

__global__ __launch_bounds__(GM_THREADS) void gm_split_kernel(const float* __restrict__ rows, int64_t n, int F, int t1, const double* __restrict__ mu,
                                                              const double* __restrict__ P, double* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) GmShared sh;
    const int64_t i0 = (int64_t)blockIdx.x * GM_T;
    const int tj = t1 - 1 - (int)blockIdx.y;                                    // the longest K loops first
    const double q = gm_tile(sh, rows, n, F, mu, P, i0, tj);
    if (threadIdx.x < GM_T && i0 + threadIdx.x < n) ws[(int64_t)tj * n + i0 + threadIdx.x] = q;
}

__global__ __launch_bounds__(GM_THREADS) void gm_merge_kernel(const double* __restrict__ ws, int64_t n, int t1, double* __restrict__ maha) {
    const int64_t i = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
    if (i >= n) return;
    double total = ws[i];
    for (int tj = 1; tj < t1; tj++) total += ws[(int64_t)tj * n + i];
    maha[i] = total;
}

}  // namespace

TDGP_API int tdgp_gaussian_maha_mode(int64_t n, int F) {
    if (!gm_shape_ok(n, F)) return -1;
    return gm_plan(n, F).split ? TDGP_MAHA_SPLIT : TDGP_MAHA_DIRECT;
}

TDGP_API int64_t tdgp_gaussian_maha_workspace_bytes(int64_t n, int F) {
    if (!gm_shape_ok(n, F)) return -1;
    const GmPlan p = gm_plan(n, F);
    if (!p.split || n == 0) return 16;                                          // direct: the workspace is not touched
    return (int64_t)p.t1 * n * 8;
}

TDGP_API int tdgp_gaussian_maha(const float* rows, int64_t n, int F, const double* mu, const double* P, double* maha, void* workspace,
                                int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(gm_shape_ok(n, F), TDGP_EINVAL, "gaussian_maha: n = %lld, F = %d outside 0 <= n < 2^31, 1 <= F <= %d", (long long)n, F, GM_MAX_F);
    if (n == 0) return TDGP_OK;                                                  // nothing to score, whatever the pointers
    TDGP_CHECK(rows && mu && P && maha && workspace, TDGP_EINVAL, "gaussian_maha: null pointer");
    TDGP_CHECK(((uintptr_t)rows & 3) == 0 && (((uintptr_t)mu | (uintptr_t)P | (uintptr_t)maha | (uintptr_t)workspace) & 7) == 0, TDGP_EINVAL,
               "gaussian_maha: rows must be 4-byte aligned, mu / P / maha / workspace 8-byte aligned");
    const int64_t need = tdgp_gaussian_maha_workspace_bytes(n, F);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EINVAL, "gaussian_maha: workspace of %lld bytes, %lld needed (workspace too small)",
               (long long)workspace_bytes, (long long)need);
    const GmPlan p = gm_plan(n, F);
    hipStream_t st = (hipStream_t)stream;
    if (!p.split) {
        TDGP_LAUNCH("gm_direct_kernel", gm_direct_kernel, dim3((unsigned)p.row_tiles), dim3(GM_THREADS), 0, st, rows, n, F, p.t1, mu, P, maha);
        TDGP_LAUNCH_CHECK();
        return TDGP_OK;
    }
    double* ws = (double*)workspace;
    TDGP_LAUNCH("gm_split_kernel", gm_split_kernel, dim3((unsigned)p.row_tiles, (unsigned)p.t1), dim3(GM_THREADS), 0, st, rows, n, F, p.t1, mu, P, ws);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("gm_merge_kernel", gm_merge_kernel, dim3((unsigned)cdiv64(n, GM_THREADS)), dim3(GM_THREADS), 0, st, (const double*)ws, n, p.t1, maha);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// pair_dist.hip -- the differential distance of the perceptual path length (src/metrics/perceptual_path_length.py:88-89):
//   lpips_t0, lpips_t1 = features.chunk(2);  dist = (lpips_t0 - lpips_t1).square().sum(1) / epsilon ** 2
// over rows as wide as an LPIPS feature stack (7 995 392 floats per 256^2 image for the reference's VGG16).  In torch that is two full-width
// temporaries and an fp32 sum of squares of differences that sit next to cancellation.  Here: one read of the two rows, the difference in
// fp32 (one rounding), its square and every addition in fp64, one rounding of the scaled sum.
//
// The summation tree is a function of W alone (include/tdgp.h):
//   * a row is cut into segments of PD_SEG elements; segment s of row i is block (s, i);
//   * inside a segment element j belongs to thread (j / 4) % PD_BLOCK, quad (j / 4) / PD_BLOCK -- by its INDEX, not by its address, so that
//     the alignment of a row (4 bytes only when W % 4 != 0, and different for the two rows of a pair and from call to call) changes how a
//     quad is loaded (one 16-byte load where its address allows, four 4-byte loads otherwise) and never which sum it enters;
//   * a thread adds its quads in order, the 64 lanes of a wave are summed by the DPP scan (wave_sum_f64), the four wave totals in order;
//   * pd_finish_kernel adds the segment partials of a row in index order (lane l takes partials l, l + 64, ..., then the same wave sum).
// A row that fits one segment is finished by its own block; no launch follows.  No atomics, one writer per partial and per output: the same
// bytes on every run and in whatever call a row is computed.  This is a streaming reduction: it is not the expensive part of the metric (the
// generator and the caller's detector are); what it buys is the defined arithmetic and the absent temporaries.
#include "common.h"

namespace {

constexpr int PD_BLOCK = 256;
constexpr int PD_QUADS = 16;                                  // quads of 4 elements per thread and segment
constexpr int64_t PD_SEG = (int64_t)PD_BLOCK * PD_QUADS * 4;  // 16384 elements = 64 KiB of each row per block

static inline int64_t pd_segments(int64_t W) { return (W + PD_SEG - 1) / PD_SEG; }

// elements [j, j + 4) of a row, the ones at or past `end` read as 0
__device__ __forceinline__ float4 pd_load(const float* __restrict__ row, int64_t j, int64_t end) {
    const float* p = row + j;
    if (j + 4 <= end) {
        if (((uintptr_t)p & 15u) == 0) return *reinterpret_cast<const float4*>(p);
        return make_float4(p[0], p[1], p[2], p[3]);
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < end) v.x = p[0];
    if (j + 1 < end) v.y = p[1];
    if (j + 2 < end) v.z = p[2];
    return v;
}

__device__ __forceinline__ double pd_sq(float a, float b) {
    const float d = a - b;                                    // fp32, one rounding
    return (double)d * (double)d;
}

// the total of a block's per-thread values in every thread of wave 0 (PD_BLOCK / 64 wave totals added in order)
__device__ __forceinline__ double pd_block_sum(double v, double* sh) {
    const double w = wave_sum_f64(v);
    if (lane_id() == 0) sh[threadIdx.x >> 6] = w;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int k = 1; k < PD_BLOCK / 64; k++) s += sh[k];
    return s;
}

__global__ __launch_bounds__(PD_BLOCK) void pd_partial_kernel(const float* __restrict__ feats, int64_t n, int64_t W, double inv_scale,
                                                              float* __restrict__ out, double* __restrict__ partial, int segments) {
    __shared__ double sh[PD_BLOCK / 64];
    const int64_t i = blockIdx.y, s = blockIdx.x;
    const float* __restrict__ a = feats + i * W;
    const float* __restrict__ b = feats + (n + i) * W;
    const int64_t j0 = s * PD_SEG, end = min(j0 + PD_SEG, W);
    double acc = 0.0;
#pragma unroll 4
    for (int q = 0; q < PD_QUADS; q++) {
        const int64_t j = j0 + ((int64_t)q * PD_BLOCK + threadIdx.x) * 4;
        if (j < end) {
            const float4 x = pd_load(a, j, end), y = pd_load(b, j, end);
            acc += pd_sq(x.x, y.x);
            acc += pd_sq(x.y, y.y);
            acc += pd_sq(x.z, y.z);
            acc += pd_sq(x.w, y.w);
        }
    }
    const double total = pd_block_sum(acc, sh);
    if (threadIdx.x == 0) {
        if (segments == 1) out[i] = (float)(total * inv_scale);
        else partial[i * segments + s] = total;
    }
}

// one wave per row
__global__ __launch_bounds__(64) void pd_finish_kernel(const double* __restrict__ partial, int segments, double inv_scale, float* __restrict__ out) {
    const int64_t i = blockIdx.x;
    const double* __restrict__ p = partial + i * segments;
    double acc = 0.0;
    for (int k = threadIdx.x; k < segments; k += 64) acc += p[k];
    const double total = wave_sum_f64(acc);
    if (threadIdx.x == 0) out[i] = (float)(total * inv_scale);
}

static int pd_check_shape(int64_t n, int64_t W) {
    TDGP_CHECK(W >= 1 && n >= 0, TDGP_EINVAL, "pair_sqdist: n = %lld pairs of W = %lld features: need n >= 0 and W >= 1", (long long)n, (long long)W);
    TDGP_CHECK(W < ((int64_t)1 << 31), TDGP_EUNSUPPORTED, "pair_sqdist: W = %lld features per row, at most 2^31 - 1", (long long)W);
    TDGP_CHECK(n <= 65535, TDGP_EUNSUPPORTED, "pair_sqdist: n = %lld pairs per call, at most 65535", (long long)n);
    return TDGP_OK;
}

}  // namespace

TDGP_API int64_t tdgp_pair_sqdist_workspace_bytes(int64_t n, int64_t W) {
    if (pd_check_shape(n, W) != TDGP_OK) return -1;
    const int64_t segments = pd_segments(W);
    return segments == 1 ? 0 : ((n * segments * 8 + 15) & ~(int64_t)15);
}

TDGP_API int tdgp_pair_sqdist(const float* feats, int64_t n, int64_t W, double inv_scale, float* out, void* workspace, int64_t workspace_bytes,
                              tdgp_stream_t stream) {
    const int rc = pd_check_shape(n, W);
    if (rc != TDGP_OK) return rc;
    if (n == 0) return TDGP_OK;
    TDGP_CHECK(feats && out, TDGP_EINVAL, "pair_sqdist: null pointer");
    TDGP_CHECK(((uintptr_t)feats & 3) == 0 && ((uintptr_t)out & 3) == 0, TDGP_EINVAL, "pair_sqdist: feats and out must be 4-byte aligned");
    const int64_t need = tdgp_pair_sqdist_workspace_bytes(n, W);
    TDGP_CHECK(need == 0 || (workspace && ((uintptr_t)workspace & 7) == 0), TDGP_EINVAL, "pair_sqdist: the workspace must be given, 8-byte aligned");
    TDGP_CHECK(workspace_bytes >= need, TDGP_EWORKSPACE, "pair_sqdist: workspace of %lld bytes, %lld needed (workspace too small)",
               (long long)workspace_bytes, (long long)need);
    const int segments = (int)pd_segments(W);
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    TDGP_LAUNCH("pd_partial_kernel", pd_partial_kernel, dim3((unsigned)segments, (unsigned)n), dim3(PD_BLOCK), 0, st, feats, n, W, inv_scale, out, partial,
                segments);
    TDGP_LAUNCH_CHECK();
    if (segments > 1) {
        TDGP_LAUNCH("pd_finish_kernel", pd_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, (const double*)partial, segments, inv_scale, out);
        TDGP_LAUNCH_CHECK();
    }
    return TDGP_OK;
}

// iso_surface.hip -- the per-ray tail of a shape frame: densities along a ray -> first crossing of a density level -> its refinement -> a
// stencil for the normal -> a shade (shapes.py: render_shape_views).  Nothing in the reference does this on the rays (its
// scripts/extract_geometry.py stops at a mesh file); the three kernels sit between passes of the field kernels:
//   field (ray mode, S) -> iso_bracket -> field (ray mode, N) -> iso_locate -> field (coords mode, 7 points per ray) -> iso_shade
// Arithmetic contract (include/tdgp.h): every fp32 operation rounded once in the order written (the library is built with
// -ffp-contract=off), `/` and sqrtf correctly rounded, ordered comparisons (a NaN compares false), one writer per output element, no
// atomics, no workspace: the same bytes on every run, and a numpy float32 restatement reproduces them bit for bit (tests/shapes_reference.py).
// Memory-light kernels kept plain: no LDS, the first crossing comes from a ballot over the ray's lane group.
#include "common.h"
#include "shade.h"

namespace {

// sigma as pointer + element stride: stride 4 on column 3 of the field kernels' rgbs [., 4] reads them in place.  One dword per sample: a
// 16-byte load of the row written in the source is narrowed by the compiler to the one component that is used (the lines fetched are the same).
__device__ __forceinline__ float load_sigma(const float* __restrict__ sigma, int64_t stride, int64_t i) { return sigma[i * stride]; }

// First lane of this ray's group of L adjacent lanes (L a power of two <= 64) whose predicate holds, or -1.  Every lane of the wave calls it.
__device__ __forceinline__ int first_in_group(bool pred, int L) {
    const uint64_t mask = __ballot(pred);
    const int base = lane_id() & ~(L - 1);
    const uint64_t mine = (mask >> base) & (L == 64 ? ~0ull : ((1ull << L) - 1ull));
    return mine ? __ffsll((unsigned long long)mine) - 1 : -1;
}

// One ray per group of L lanes.  Rows longer than 64 (L == 64: one ray per wave, so the loop is wave-uniform) walk in chunks of 64 and stop at
// the first chunk with a crossing.
__global__ __launch_bounds__(256) void iso_bracket_kernel(const float* __restrict__ sigma, int64_t stride, const float* __restrict__ t, int64_t rays, int S,
                                                          int N, int lg, float level, int32_t* __restrict__ idx_out, float* __restrict__ t_fine) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ray = gid >> lg;
    const int L = 1 << lg, l = (int)(gid & (L - 1));
    const bool live = ray < rays;
    int idx = S;
    for (int k0 = 0; k0 < S; k0 += 64) {
        const int k = k0 + l;
        bool hit = false;
        if (live && k < S) hit = load_sigma(sigma, stride, ray * S + k) >= level;
        const int f = first_in_group(hit, L);
        if (f >= 0) { idx = k0 + f; break; }
    }
    if (!live) return;
    if (l == 0) idx_out[ray] = idx;
    const float* tr = t + ray * S;
    float lo, hi;
    if (idx == 0) { lo = hi = tr[0]; }
    else if (idx == S) { lo = hi = tr[S - 1]; }
    else { lo = tr[idx - 1]; hi = tr[idx]; }
    const bool inside = idx >= 1 && idx <= S - 1;
    const float fn = (float)N;
    for (int j = l; j < N; j += L) {
        float v = hi;                                                    // the known crossing is the last fine sample; idx == 0 / S: lo == hi
        if (inside && j < N - 1) v = lo + (hi - lo) * ((float)(j + 1) / fn);
        t_fine[ray * N + j] = v;
    }
}

// One ray per group of L lanes over its N <= 64 fine samples; the 21 floats of its stencil points are spread over the group.
__global__ __launch_bounds__(256) void iso_locate_kernel(const float* __restrict__ sigma, int64_t stride, const float* __restrict__ t, const int32_t* __restrict__ idx_in,
                                                         const float* __restrict__ sigma_f, int64_t stride_f, const float* __restrict__ t_fine,
                                                         const float* __restrict__ ray_o, const float* __restrict__ ray_d, int64_t rays, int S, int N, int lg,
                                                         float level, float h, float t_miss, float* __restrict__ t_hit, int32_t* __restrict__ status,
                                                         float* __restrict__ points) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ray = gid >> lg;
    const int L = 1 << lg, l = (int)(gid & (L - 1));
    const bool live = ray < rays;
    bool hit = false;
    if (live && l < N) hit = load_sigma(sigma_f, stride_f, ray * N + l) >= level;
    const int f = first_in_group(hit, L);
    if (!live) return;
    int idx = idx_in[ray];
    idx = idx < 0 ? 0 : (idx > S ? S : idx);                            // a row index outside [0, S] never becomes an address
    float th;
    int st;
    if (idx == S) { st = 0; th = t_miss; }
    else if (idx == 0) { st = 2; th = t[ray * S]; }
    else {
        st = 1;
        const int j = f >= 0 ? f : N - 1;
        const float s_hi = load_sigma(sigma_f, stride_f, ray * N + j);
        const float t_hi = t_fine[ray * N + j];
        float s_lo, t_lo;
        if (j == 0) { s_lo = load_sigma(sigma, stride, ray * S + idx - 1); t_lo = t[ray * S + idx - 1]; }
        else { s_lo = load_sigma(sigma_f, stride_f, ray * N + j - 1); t_lo = t_fine[ray * N + j - 1]; }
        float a = (level - s_lo) / (s_hi - s_lo);
        if (!(a >= 0.0f && a <= 1.0f)) a = 1.0f;                        // NaN, infinities, a flat pair: the high side
        th = t_lo + (t_hi - t_lo) * a;
    }
    if (l == 0) { t_hit[ray] = th; status[ray] = st; }
    for (int p = l; p < 21; p += L) {
        const int m = p / 3, c = p - 3 * m;
        float x = ray_o[ray * 3 + c] + ray_d[ray * 3 + c] * th;
        if (m >= 1 && ((m - 1) >> 1) == c) x = (m & 1) ? x + h : x - h;
        points[ray * 21 + p] = x;
    }
}

__global__ __launch_bounds__(256) void iso_shade_kernel(const float* __restrict__ stencil, const int32_t* __restrict__ status, const float* __restrict__ ray_d,
                                                        int64_t rays, ShadeParams q, float* __restrict__ rgb, float* __restrict__ normal) {
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= rays) return;
    const float* row = stencil + ray * 28;                              // 7 rows of (r, g, b, sigma): the colour of row 0, sigma of rows 1..6
    float sg[7];
#pragma unroll
    for (int i = 1; i < 7; i++) sg[i] = row[4 * i + 3];
    const int st = status[ray];
    const float d[3] = {ray_d[ray * 3 + 0], ray_d[ray * 3 + 1], ray_d[ray * 3 + 2]};
    float out[3], n[3];
    if (st == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { out[c] = q.background[c]; n[c] = 0.0f; }
    } else {
        const float g[3] = {sg[1] - sg[2], sg[3] - sg[4], sg[5] - sg[6]};
        const float gq = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        const float dn = ray_norm(d);
        if (gq > 0.0f && gq < __builtin_inff()) {
            const float r = sqrtf(gq);
#pragma unroll
            for (int c = 0; c < 3; c++) n[c] = (-g[c]) / r;
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) n[c] = (-d[c]) / dn;
        }
        const float col[3] = {row[0], row[1], row[2]};
        shade_hit(q, n, d, [&](int c) { return col[c] * 0.5f + 0.5f; }, out);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[ray * 3 + c] = out[c];
    if (normal) {
#pragma unroll
        for (int c = 0; c < 3; c++) normal[ray * 3 + c] = n[c];
    }
}

int lane_group_log2(int n) {                 // log2 of min(64, smallest power of two >= n)
    int lg = 0;
    while ((1 << lg) < n && lg < 6) lg++;
    return lg;
}

const int64_t ISO_RAYS_MAX = (int64_t)1 << 30;      // rays x 64 lanes / 256 stays a valid grid; rays x 512 samples a valid int64 offset

}  // namespace

TDGP_API int tdgp_iso_bracket(const float* sigma, int64_t sigma_stride, const float* t, int64_t rays, int S, int N, float level, int32_t* idx, float* t_fine,
                              tdgp_stream_t stream) {
    TDGP_CHECK(sigma && t && idx && t_fine, TDGP_EINVAL, "iso_bracket: null pointer");
    TDGP_CHECK(rays >= 0 && rays <= ISO_RAYS_MAX && sigma_stride >= 1, TDGP_EINVAL, "iso_bracket: bad shape");
    TDGP_CHECK(S >= 2 && N >= 1, TDGP_EINVAL, "iso_bracket: need S >= 2 and N >= 1 (got S=%d, N=%d)", S, N);
    TDGP_CHECK(S <= 512 && N <= 64, TDGP_EUNSUPPORTED, "iso_bracket: at most 512 coarse and 64 fine samples per ray (got S=%d, N=%d)", S, N);
    if (rays == 0) return TDGP_OK;
    const int lg = lane_group_log2(S);
    const dim3 grid((unsigned)cdiv64(rays << lg, 256));
    TDGP_LAUNCH("iso_bracket_kernel", iso_bracket_kernel, grid, dim3(256), 0, (hipStream_t)stream, sigma, sigma_stride, t, rays, S, N, lg, level, idx, t_fine);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_iso_locate(const float* sigma, int64_t sigma_stride, const float* t, const int32_t* idx, const float* sigma_fine, int64_t sigma_fine_stride,
                             const float* t_fine, const float* ray_o, const float* ray_d, int64_t rays, int S, int N, float level, float h, float t_miss,
                             float* t_hit, int32_t* status, float* points, tdgp_stream_t stream) {
    TDGP_CHECK(sigma && t && idx && sigma_fine && t_fine && ray_o && ray_d && t_hit && status && points, TDGP_EINVAL, "iso_locate: null pointer");
    TDGP_CHECK(rays >= 0 && rays <= ISO_RAYS_MAX && sigma_stride >= 1 && sigma_fine_stride >= 1, TDGP_EINVAL, "iso_locate: bad shape");
    TDGP_CHECK(S >= 2 && N >= 1, TDGP_EINVAL, "iso_locate: need S >= 2 and N >= 1 (got S=%d, N=%d)", S, N);
    TDGP_CHECK(S <= 512 && N <= 64, TDGP_EUNSUPPORTED, "iso_locate: at most 512 coarse and 64 fine samples per ray (got S=%d, N=%d)", S, N);
    if (rays == 0) return TDGP_OK;
    const int lg = lane_group_log2(N);
    const dim3 grid((unsigned)cdiv64(rays << lg, 256));
    TDGP_LAUNCH("iso_locate_kernel", iso_locate_kernel, grid, dim3(256), 0, (hipStream_t)stream, sigma, sigma_stride, t, idx, sigma_fine, sigma_fine_stride, t_fine,
                ray_o, ray_d, rays, S, N, lg, level, h, t_miss, t_hit, status, points);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_iso_shade(const float* stencil, const int32_t* status, const float* ray_d, int64_t rays, int mode, const float* light, float ambient,
                            const float* albedo, const float* background, float* rgb, float* normal, tdgp_stream_t stream) {
    TDGP_CHECK(stencil && status && ray_d && albedo && background && rgb, TDGP_EINVAL, "iso_shade: null pointer");
    TDGP_CHECK(rays >= 0 && rays <= ISO_RAYS_MAX, TDGP_EINVAL, "iso_shade: bad shape");
    TDGP_CHECK(mode >= 0 && mode <= 2, TDGP_EINVAL, "iso_shade: mode must be 0 (shaded), 1 (normals) or 2 (colour), got %d", mode);
    if (rays == 0) return TDGP_OK;
    const ShadeParams q = shade_params(mode, light, ambient, albedo, background);
    TDGP_LAUNCH("iso_shade_kernel", iso_shade_kernel, dim3((unsigned)cdiv64(rays, 256)), dim3(256), 0, (hipStream_t)stream, stencil, status, ray_d,
                rays, q, rgb, normal);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

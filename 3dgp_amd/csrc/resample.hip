// resample.hip -- anti-aliased resampling of 8-bit images and 16-bit depth maps with Pillow's arithmetic (include/tdgp.h, tdgp_resample_*):
// the operation behind the reference's dataset scripts (scripts/utils.py:116-120 `center_resize_crop`, the eval transform of
// scripts/data_scripts/extract_features.py), which reach it through torchvision -> PIL.Image.resize.
//
// Two separable passes, horizontal first, each a table-driven tap loop: output index i reads `n` source samples from `first` on and weighs
// them with row i of the coefficient table (bounds [out, 2] = (first, n), coeffs [out, ksize]; the host builds both in float64).
//   8 bit : int32 coefficients on a 2^22 scale, ss = 2^21 + sum pixel * k in int32, out = clip(ss >> 22, 0, 255);
//   16 bit: float64 coefficients, ss = 0.0; ss += double(pixel) * k in tap order, every product and sum rounded on its own (__dmul_rn /
//           __dadd_rn never fuse), v = int(ss +- 0.5); the stored value is Pillow's byte pair (see rs_round).
// The horizontal pass rounds to the sample type; its rows are the only intermediate and live in the caller's workspace.  A pass whose size
// does not change is not run: the other one reads the source / writes the destination directly.
//
// Layout.  The traffic is bytes and both passes are bound by it, so the lanes of a wave always walk CONSECUTIVE samples of one row:
//   horizontal: a lane owns one output sample (ox, c) of RS_ROWS consecutive rows; neighbouring lanes read overlapping windows of the same
//               source lines, a coefficient is fetched once for the RS_ROWS rows it serves;
//   vertical  : a lane owns one output sample of one output row and walks DOWN the intermediate rows; every tap is one fully coalesced
//               row segment and the coefficient is uniform over the block.
// No atomics, no LDS, one writer per output sample: the same bytes on every run.  Table entries are clamped to the source extent before
// they are used, so a damaged table gives wrong pixels, never an access outside the images.
#include "common.h"

namespace {

constexpr int RS_BLOCK = 256;
constexpr int RS_ROWS = 4;                // rows per lane in the horizontal pass
constexpr int RS_MAX_SIZE = 32768;        // per axis, source and destination
constexpr int64_t RS_MAX_BATCH = 65535;   // grid.z

struct rs_norm {
    float mean[3], std[3];
};

__device__ __forceinline__ int32_t rs_zero(int32_t) { return 1 << 21; }
__device__ __forceinline__ double rs_zero(double) { return 0.0; }
__device__ __forceinline__ int32_t rs_mac(int32_t ss, uint8_t p, int32_t k) { return ss + (int32_t)p * k; }
__device__ __forceinline__ double rs_mac(double ss, uint16_t p, double k) { return __dadd_rn(ss, __dmul_rn((double)p, k)); }

__device__ __forceinline__ uint8_t rs_round(int32_t ss, int) {
    const int32_t v = ss >> 22;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
// Pillow stores hi = clip(v >> 8, 0, 255), lo = clip(v % 256, 0, 255) (C's %): a negative v gives 0, a v above 65535 gives 0xFF00 | (v & 255).
__device__ __forceinline__ uint16_t rs_round(double ss, int saturate) {
    const double r = ss < 0.0 ? ss - 0.5 : ss + 0.5;
    const int32_t v = (int32_t)fmin(fmax(r, -2147483648.0), 2147483647.0);
    if (v <= 0) return 0;
    if (v > 65535) return (uint16_t)(saturate ? 65535 : (0xFF00 | (v & 255)));
    return (uint16_t)v;
}

// (first, n) of output index i, clamped to a source of `in_size` samples and a table of `ks` coefficients per row
__device__ __forceinline__ void rs_bounds(const int32_t* __restrict__ bounds, int i, int in_size, int ks, int& first, int& n) {
    first = bounds[2 * i];
    n = bounds[2 * i + 1];
    first = first < 0 ? 0 : (first > in_size - 1 ? in_size - 1 : first);
    n = n < 0 ? 0 : n;
    n = n > ks ? ks : n;
    n = n > in_size - first ? in_size - first : n;
}

// dst[b][y][j], j = (ox - ox0) * C + c over n_ox output columns from ox0 on, for the `rows` rows of src
template <typename P, typename K>
__global__ __launch_bounds__(RS_BLOCK) void rs_hpass_kernel(const P* __restrict__ src, int64_t src_item, int64_t src_row, int C, int in_w, int rows,
                                                            const int32_t* __restrict__ bounds, const K* __restrict__ coeffs, int ks, int ox0, int n_ox,
                                                            P* __restrict__ dst, int64_t dst_item, int64_t dst_row, int saturate) {
    const int j = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (j >= n_ox * C) return;
    const int oxr = j / C, c = j - oxr * C, ox = ox0 + oxr;
    const int r0 = blockIdx.y * RS_ROWS;
    const int nr = rows - r0 < RS_ROWS ? rows - r0 : RS_ROWS;
    int first, n;
    rs_bounds(bounds, ox, in_w, ks, first, n);
    const K* __restrict__ k = coeffs + (int64_t)ox * ks;
    const P* __restrict__ s = src + (int64_t)blockIdx.z * src_item + (int64_t)r0 * src_row + (int64_t)first * C + c;
    K acc[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) acc[r] = rs_zero(K());
    for (int t = 0; t < n; t++) {
        const K kk = k[t];
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++)
            if (r < nr) acc[r] = rs_mac(acc[r], s[(int64_t)r * src_row + (int64_t)t * C], kk);
    }
    P* __restrict__ d = dst + (int64_t)blockIdx.z * dst_item + (int64_t)r0 * dst_row + j;
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++)
        if (r < nr) d[(int64_t)r * dst_row] = rs_round(acc[r], saturate);
}

// dst[b][oy - oy0][j] over the row_elems samples of a row; bounds == nullptr: the identity (a copy of rows oy0 ...)
template <typename P, typename K>
__global__ __launch_bounds__(RS_BLOCK) void rs_vpass_kernel(const P* __restrict__ src, int64_t src_item, int64_t src_row, int row_elems, int in_h,
                                                            const int32_t* __restrict__ bounds, const K* __restrict__ coeffs, int ks, int oy0,
                                                            P* __restrict__ dst, int64_t dst_item, int64_t dst_row, int saturate) {
    const int j = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (j >= row_elems) return;
    const int oy = oy0 + (int)blockIdx.y;
    const P* __restrict__ s = src + (int64_t)blockIdx.z * src_item + j;
    P* __restrict__ d = dst + (int64_t)blockIdx.z * dst_item + (int64_t)blockIdx.y * dst_row + j;
    if (bounds == nullptr) {
        *d = s[(int64_t)oy * src_row];
        return;
    }
    int first, n;
    rs_bounds(bounds, oy, in_h, ks, first, n);
    const K* __restrict__ k = coeffs + (int64_t)oy * ks;
    s += (int64_t)first * src_row;
    K acc = rs_zero(K());
    for (int t = 0; t < n; t++) acc = rs_mac(acc, s[(int64_t)t * src_row], k[t]);
    *d = rs_round(acc, saturate);
}

// the vertical pass of the detector input: a lane owns one output pixel (all C channels) of one output row, rounds each channel to the
// byte the resized image would hold and stores ((float(v) / 255) - mean[c]) / std[c] channel-first, every operation rounded on its own
__global__ __launch_bounds__(RS_BLOCK) void rs_vpass_f32_kernel(const uint8_t* __restrict__ src, int64_t src_item, int64_t src_row, int C, int n_cols,
                                                                int in_h, const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs, int ks,
                                                                int oy0, int n_oy, float* __restrict__ dst, rs_norm norm) {
    const int x = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (x >= n_cols) return;
    const int oy = oy0 + (int)blockIdx.y;
    const uint8_t* __restrict__ s = src + (int64_t)blockIdx.z * src_item + (int64_t)x * C;
    int first = oy, n = 1;
    const int32_t* __restrict__ k = nullptr;
    if (bounds != nullptr) {
        rs_bounds(bounds, oy, in_h, ks, first, n);
        k = coeffs + (int64_t)oy * ks;
    }
    s += (int64_t)first * src_row;
    int32_t acc[3] = {1 << 21, 1 << 21, 1 << 21};
    for (int t = 0; t < n; t++) {
        const int32_t kk = k ? k[t] : (1 << 22);
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (c < C) acc[c] = rs_mac(acc[c], s[(int64_t)t * src_row + c], kk);
    }
    const int64_t plane = (int64_t)n_oy * n_cols;
    float* __restrict__ d = dst + (int64_t)blockIdx.z * C * plane + (int64_t)blockIdx.y * n_cols + x;
#pragma unroll
    for (int c = 0; c < 3; c++)
        if (c < C) d[c * plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)rs_round(acc[c], 0), 255.0f), norm.mean[c]), norm.std[c]);
}

struct rs_shape {
    int64_t B;
    int H, W, C, x0, y0, w, h, oh, ow;
};

static int rs_check(const char* what, const rs_shape& s, const void* hb, const void* hk, int hks, const void* vb, const void* vk, int vks) {
    TDGP_CHECK(s.B >= 0, TDGP_EINVAL, "%s: B = %lld", what, (long long)s.B);
    TDGP_CHECK(s.B <= RS_MAX_BATCH, TDGP_EUNSUPPORTED, "%s: B = %lld images per call, at most %lld", what, (long long)s.B, (long long)RS_MAX_BATCH);
    TDGP_CHECK(s.H >= 1 && s.W >= 1 && s.oh >= 1 && s.ow >= 1, TDGP_EINVAL, "%s: source %d x %d, destination %d x %d: sizes must be positive", what, s.W,
               s.H, s.ow, s.oh);
    TDGP_CHECK(s.H <= RS_MAX_SIZE && s.W <= RS_MAX_SIZE && s.oh <= RS_MAX_SIZE && s.ow <= RS_MAX_SIZE, TDGP_EUNSUPPORTED,
               "%s: source %d x %d, destination %d x %d: at most %d samples per axis", what, s.W, s.H, s.ow, s.oh, RS_MAX_SIZE);
    TDGP_CHECK(s.C == 1 || s.C == 3, TDGP_EUNSUPPORTED, "%s: C = %d channels, 1 or 3 are supported", what, s.C);
    TDGP_CHECK(s.w >= 1 && s.h >= 1 && s.x0 >= 0 && s.y0 >= 0 && s.x0 <= s.W - s.w && s.y0 <= s.H - s.h, TDGP_EINVAL,
               "%s: crop window (x0 %d, y0 %d, w %d, h %d) does not lie inside the %d x %d source", what, s.x0, s.y0, s.w, s.h, s.W, s.H);
    TDGP_CHECK((hb != nullptr) == (s.ow != s.w) && (hb != nullptr) == (hk != nullptr), TDGP_EINVAL,
               "%s: the horizontal tables are given exactly when the width changes (%d -> %d)", what, s.w, s.ow);
    TDGP_CHECK((vb != nullptr) == (s.oh != s.h) && (vb != nullptr) == (vk != nullptr), TDGP_EINVAL,
               "%s: the vertical tables are given exactly when the height changes (%d -> %d)", what, s.h, s.oh);
    TDGP_CHECK((!hb || hks >= 1) && (!vb || vks >= 1), TDGP_EINVAL, "%s: ksize must be positive (%d, %d)", what, hks, vks);
    return TDGP_OK;
}

static int64_t rs_workspace(int64_t B, int h, int w, int oh, int ow_kept, int ow, int C, int sample_bytes) {
    return (ow != w && oh != h) ? B * h * (int64_t)ow_kept * C * sample_bytes : 0;
}

template <typename P, typename K>
static int rs_run(const char* what, const P* src, const rs_shape& s, const int32_t* hb, const K* hk, int hks, const int32_t* vb, const K* vk, int vks,
                  P* dst, int saturate, void* workspace, int64_t workspace_bytes, hipStream_t st) {
    const int rc = rs_check(what, s, hb, hk, hks, vb, vk, vks);
    if (rc != TDGP_OK) return rc;
    if (s.B == 0) return TDGP_OK;
    TDGP_CHECK(src && dst, TDGP_EINVAL, "%s: null pointer", what);
    TDGP_CHECK(((uintptr_t)src % sizeof(P)) == 0 && ((uintptr_t)dst % sizeof(P)) == 0, TDGP_EINVAL, "%s: misaligned image pointer", what);
    const int64_t need = rs_workspace(s.B, s.h, s.w, s.oh, s.ow, s.ow, s.C, (int)sizeof(P));
    TDGP_CHECK(need == 0 || (workspace && ((uintptr_t)workspace % sizeof(P)) == 0), TDGP_EINVAL, "%s: the workspace must be given, aligned to a sample", what);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed (workspace too small)", what, (long long)workspace_bytes,
               (long long)need);
    const int64_t src_row = (int64_t)s.W * s.C, src_item = (int64_t)s.H * src_row;
    const P* win = src + (int64_t)s.y0 * src_row + (int64_t)s.x0 * s.C;
    const int64_t dst_row = (int64_t)s.ow * s.C, dst_item = (int64_t)s.oh * dst_row;
    const int row_elems = s.ow * s.C;
    const dim3 block(RS_BLOCK);
    const P* vsrc = win;
    int64_t vsrc_row = src_row, vsrc_item = src_item;
    if (hb) {
        P* mid = vb ? (P*)workspace : dst;                       // [B, h, ow, C]
        const int64_t mid_item = (int64_t)s.h * dst_row;
        const dim3 grid((unsigned)cdiv(row_elems, RS_BLOCK), (unsigned)cdiv(s.h, RS_ROWS), (unsigned)s.B);
        TDGP_LAUNCH("rs_hpass_kernel", (rs_hpass_kernel<P, K>), grid, block, 0, st, win, src_item, src_row, s.C, s.w, s.h, hb, hk, hks, 0, s.ow, mid, mid_item,
                    dst_row, vb ? 0 : saturate);
        TDGP_LAUNCH_CHECK();
        vsrc = mid;
        vsrc_row = dst_row;
        vsrc_item = mid_item;
    }
    if (vb || !hb) {
        const dim3 grid((unsigned)cdiv(row_elems, RS_BLOCK), (unsigned)s.oh, (unsigned)s.B);
        TDGP_LAUNCH("rs_vpass_kernel", (rs_vpass_kernel<P, K>), grid, block, 0, st, vsrc, vsrc_item, vsrc_row, row_elems, s.h, vb, vk, vks, 0, dst, dst_item,
                    dst_row, saturate);
        TDGP_LAUNCH_CHECK();
    }
    return TDGP_OK;
}

}  // namespace

TDGP_API int64_t tdgp_resample_workspace_bytes(int64_t B, int h, int w, int oh, int ow, int C, int sample_bytes) {
    if (B < 0 || h < 1 || w < 1 || oh < 1 || ow < 1 || C < 1 || (sample_bytes != 1 && sample_bytes != 2)) return -1;
    return rs_workspace(B, h, w, oh, ow, ow, C, sample_bytes);
}

TDGP_API int tdgp_resample_u8(const uint8_t* src, int64_t B, int H, int W, int C, int x0, int y0, int w, int h, const int32_t* hbounds,
                              const int32_t* hcoeffs, int hksize, const int32_t* vbounds, const int32_t* vcoeffs, int vksize, uint8_t* dst, int oh, int ow,
                              void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    const rs_shape s = {B, H, W, C, x0, y0, w, h, oh, ow};
    return rs_run<uint8_t, int32_t>("resample_u8", src, s, hbounds, hcoeffs, hksize, vbounds, vcoeffs, vksize, dst, 0, workspace, workspace_bytes,
                                    (hipStream_t)stream);
}

TDGP_API int tdgp_resample_u16(const uint16_t* src, int64_t B, int H, int W, int x0, int y0, int w, int h, const int32_t* hbounds, const double* hcoeffs,
                               int hksize, const int32_t* vbounds, const double* vcoeffs, int vksize, uint16_t* dst, int oh, int ow, int saturate,
                               void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    const rs_shape s = {B, H, W, 1, x0, y0, w, h, oh, ow};
    TDGP_CHECK(saturate == 0 || saturate == 1, TDGP_EINVAL, "resample_u16: saturate = %d, 0 (Pillow's bytes) or 1", saturate);
    TDGP_CHECK((!hcoeffs || ((uintptr_t)hcoeffs & 7) == 0) && (!vcoeffs || ((uintptr_t)vcoeffs & 7) == 0), TDGP_EINVAL,
               "resample_u16: the coefficient tables must be 8-byte aligned");
    return rs_run<uint16_t, double>("resample_u16", src, s, hbounds, hcoeffs, hksize, vbounds, vcoeffs, vksize, dst, saturate, workspace, workspace_bytes,
                                    (hipStream_t)stream);
}

TDGP_API int64_t tdgp_resample_u8_to_f32_workspace_bytes(int64_t B, int h, int w, int oh, int ow, int C, int cw) {
    if (B < 0 || h < 1 || w < 1 || oh < 1 || ow < 1 || C < 1 || cw < 1 || cw > ow) return -1;
    return ow != w ? B * h * (int64_t)cw * C : 0;
}

TDGP_API int tdgp_resample_u8_to_f32(const uint8_t* src, int64_t B, int H, int W, int C, int x0, int y0, int w, int h, const int32_t* hbounds,
                                     const int32_t* hcoeffs, int hksize, const int32_t* vbounds, const int32_t* vcoeffs, int vksize, int oh, int ow, int cx0,
                                     int cy0, int cw, int ch, const float* mean, const float* std, float* dst, void* workspace, int64_t workspace_bytes,
                                     tdgp_stream_t stream) {
    const char* what = "resample_u8_to_f32";
    const rs_shape s = {B, H, W, C, x0, y0, w, h, oh, ow};
    const int rc = rs_check(what, s, hbounds, hcoeffs, hksize, vbounds, vcoeffs, vksize);
    if (rc != TDGP_OK) return rc;
    TDGP_CHECK(cw >= 1 && ch >= 1 && cx0 >= 0 && cy0 >= 0 && cx0 <= ow - cw && cy0 <= oh - ch, TDGP_EINVAL,
               "%s: second crop (x0 %d, y0 %d, w %d, h %d) does not lie inside the %d x %d resized image", what, cx0, cy0, cw, ch, ow, oh);
    TDGP_CHECK(mean && std, TDGP_EINVAL, "%s: mean and std (host, C floats each) must be given", what);
    if (B == 0) return TDGP_OK;
    TDGP_CHECK(src && dst, TDGP_EINVAL, "%s: null pointer", what);
    TDGP_CHECK(((uintptr_t)dst & 3) == 0, TDGP_EINVAL, "%s: dst must be 4-byte aligned", what);
    const int64_t need = tdgp_resample_u8_to_f32_workspace_bytes(B, h, w, oh, ow, C, cw);
    TDGP_CHECK(need == 0 || workspace, TDGP_EINVAL, "%s: the workspace must be given", what);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed (workspace too small)", what, (long long)workspace_bytes,
               (long long)need);
    rs_norm norm = {};
    for (int c = 0; c < C; c++) {
        TDGP_CHECK(std[c] != 0.0f, TDGP_EINVAL, "%s: std[%d] is zero", what, c);
        norm.mean[c] = mean[c];
        norm.std[c] = std[c];
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t src_row = (int64_t)W * C, src_item = (int64_t)H * src_row;
    const uint8_t* win = src + (int64_t)y0 * src_row + (int64_t)x0 * C;
    const dim3 block(RS_BLOCK);
    // the columns the second crop keeps are the only ones the horizontal pass produces; with an unchanged width they are read in place
    const uint8_t* vsrc = win + (int64_t)cx0 * C;
    int64_t vsrc_row = src_row, vsrc_item = src_item;
    if (hbounds) {
        uint8_t* mid = (uint8_t*)workspace;                       // [B, h, cw, C]
        const int64_t mid_row = (int64_t)cw * C, mid_item = (int64_t)h * mid_row;
        const dim3 grid((unsigned)cdiv(cw * C, RS_BLOCK), (unsigned)cdiv(h, RS_ROWS), (unsigned)B);
        TDGP_LAUNCH("rs_hpass_kernel", (rs_hpass_kernel<uint8_t, int32_t>), grid, block, 0, st, win, src_item, src_row, C, w, h, hbounds, hcoeffs, hksize, cx0,
                    cw, mid, mid_item, mid_row, 0);
        TDGP_LAUNCH_CHECK();
        vsrc = mid;
        vsrc_row = mid_row;
        vsrc_item = mid_item;
    }
    const dim3 grid((unsigned)cdiv(cw, RS_BLOCK), (unsigned)ch, (unsigned)B);
    TDGP_LAUNCH("rs_vpass_f32_kernel", rs_vpass_f32_kernel, grid, block, 0, st, vsrc, vsrc_item, vsrc_row, C, cw, h, vbounds, vcoeffs, vksize, cy0, ch, dst,
                norm);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

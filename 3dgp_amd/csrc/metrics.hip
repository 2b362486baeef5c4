// metrics.hip -- the device side of the non-flatness score (src/metrics/non_flatness_score.py): the quantile behind `cut_quantile` without a
// sort, and depth maps reduced to per-image histograms before anything crosses to the host.
//
// Replaces (device-wide torch ops + host round trips in the reference and in this package's first version):
//   tri_plane_renderer.py:324-326, 366-368   torch.quantile(activated densities, q): a full sort to learn two order statistics
//   non_flatness_score.py:12-15, 30          clamp + torch.histc per depth map on HOST tensors (65 536 floats per image fetched; 64 counts needed)
//
// tdgp_quantile_select is a most-significant-digit radix select over an order-preserving 32-bit key, three passes of 11 / 11 / 10 bits:
//   qs_zero_kernel          the 48 KiB of global histograms + the state words
//   qs_hist_kernel<P>       grid-stride over x (16-byte loads; head and tail scalar): elements whose key continues the prefix of a followed
//                           rank are counted by their next digit in an LDS histogram, whose non-empty bins are then added to the global one
//   qs_pick_kernel<P>       ONE block: scan the 2048 bins, find the bin holding each rank, extend the prefix, reduce the rank to the bin
// The two ranks (k_lo, k_hi <= k_lo + 1) are followed together; while their prefixes coincide (nearly always) one histogram serves both.
// After the third pick the prefix IS the key of the order statistic, hence the value: no gather pass.  Counts are integers, so the result
// does not depend on the order the atomics arrive in.  Only vector atomics (LDS and global uint32 adds / or) are used.
//
// Activated densities cluster (most of a volume is empty: softplus -> near 0, relu -> exactly 0), and a flat depth map is ONE histogram bin:
// hist_add() therefore peels up to two groups of equal bins off a wave with ballots (one add of the group's size by its first lane) before
// the remaining lanes add individually -- the dominant bin is hit by the first peel with the probability of its own share.
#include "common.h"
#include <math.h>

namespace {

constexpr int QS_BLOCK = 256;
constexpr int QS_MAX_BLOCKS = 2048;
constexpr int QS_BINS = 2048;                       // 11 bits; the last pass uses the first 1024
constexpr int QS_PASSES = 3;
constexpr int QS_STATE_WORDS = 16;                  // [0] prefix_lo [1] prefix_hi [2] rank_lo [3] rank_hi (within the prefix) [4] any NaN
constexpr int64_t QS_WS_BYTES = (int64_t)(QS_STATE_WORDS + QS_PASSES * 2 * QS_BINS) * 4;
constexpr uint32_t QS_NAN_KEY = 0xffffffffu;        // the key of a NaN bit pattern itself: no number maps to it

__host__ __device__ constexpr int qs_shift(int P) { return P == 0 ? 21 : (P == 1 ? 10 : 0); }
__host__ __device__ constexpr int qs_bits(int P) { return P == 2 ? 10 : 11; }

// order-preserving key: negatives bit-flipped, non-negatives with the sign bit set; -0.0 keyed as +0.0, every NaN as QS_NAN_KEY
__device__ __forceinline__ uint32_t qs_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return v != v ? QS_NAN_KEY : k;
}
__device__ __forceinline__ float qs_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// h[bin] += 1 for every lane with `valid`; to be reached by the whole wave (the ballots are taken over it)
__device__ __forceinline__ void hist_add(uint32_t* h, bool valid, uint32_t bin) {
    unsigned long long live = __ballot(valid);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (!live) break;                                           // wave-uniform
        const int leader = __ffsll((long long)live) - 1;
        const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
        const bool m = valid && bin == lb;
        const unsigned long long mm = __ballot(m);
        if (lane_id() == leader) atomicAdd(&h[lb], (uint32_t)__popcll(mm));
        valid = valid && !m;
        live &= ~mm;
    }
    if (valid) atomicAdd(&h[bin], 1u);
}

__global__ __launch_bounds__(QS_BLOCK) void qs_zero_kernel(uint32_t* __restrict__ ws, int words, uint32_t k_lo, uint32_t k_hi) {
    for (int i = blockIdx.x * QS_BLOCK + threadIdx.x; i < words; i += gridDim.x * QS_BLOCK)
        ws[i] = i == 2 ? k_lo : (i == 3 ? k_hi : 0u);
}

template <int P>
__device__ __forceinline__ void qs_count(uint32_t* h, bool valid, float v, uint32_t pre_lo, uint32_t pre_hi, bool two, bool& nan) {
    constexpr int SH = qs_shift(P), BITS = qs_bits(P);
    const uint32_t k = qs_key(v);
    const uint32_t bin = (k >> SH) & ((1u << BITS) - 1u);
    if (P == 0) {
        nan = nan || (valid && k == QS_NAN_KEY);
        hist_add(h, valid, bin);
    } else {
        hist_add(h, valid && ((k ^ pre_lo) >> (SH + BITS)) == 0u, bin);
        if (two) hist_add(h + QS_BINS, valid && ((k ^ pre_hi) >> (SH + BITS)) == 0u, bin);     // `two` is uniform over the grid
    }
}

template <int P>
__global__ __launch_bounds__(QS_BLOCK) void qs_hist_kernel(const float* __restrict__ x, int64_t n, uint32_t* __restrict__ ws) {
    __shared__ uint32_t h[2 * QS_BINS];
    for (int i = threadIdx.x; i < 2 * QS_BINS; i += QS_BLOCK) h[i] = 0u;
    const uint32_t pre_lo = P ? ws[0] : 0u, pre_hi = P ? ws[1] : 0u;
    const bool two = pre_lo != pre_hi;
    __syncthreads();
    // x[head ...] is 16-byte aligned; nv whole float4 follow, then n - head - 4 nv < 4 scalars
    const int64_t head = min((int64_t)(((16u - (uint32_t)((uintptr_t)x & 15u)) & 15u) >> 2), n);
    const int64_t nv = (n - head) >> 2;
    const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);
    bool nan = false;
    for (int64_t base = (int64_t)blockIdx.x * QS_BLOCK; base < nv; base += (int64_t)gridDim.x * QS_BLOCK) {      // block-uniform trip count
        const int64_t i = base + threadIdx.x;
        const bool valid = i < nv;
        const float4 v = valid ? xv[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        qs_count<P>(h, valid, v.x, pre_lo, pre_hi, two, nan);
        qs_count<P>(h, valid, v.y, pre_lo, pre_hi, two, nan);
        qs_count<P>(h, valid, v.z, pre_lo, pre_hi, two, nan);
        qs_count<P>(h, valid, v.w, pre_lo, pre_hi, two, nan);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {                      // head and tail: at most 3 + 3 scalars, by the first wave of block 0
        const int64_t tail0 = head + 4 * nv;
        const int t = threadIdx.x;
        const bool valid = t < 3 ? (int64_t)t < head : (t < 6 && tail0 + (t - 3) < n);
        const int64_t idx = t < 3 ? (int64_t)t : tail0 + (t - 3);
        const float v = valid ? x[idx] : 0.f;
        qs_count<P>(h, valid, v, pre_lo, pre_hi, two, nan);
    }
    __syncthreads();
    uint32_t* __restrict__ g = ws + QS_STATE_WORDS + P * 2 * QS_BINS;
    for (int i = threadIdx.x; i < (two ? 2 : 1) * QS_BINS; i += QS_BLOCK) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&g[i], c);
    }
    if (P == 0 && nan) atomicOr(&ws[4], 1u);
}

// torch.lerp as torch's GPU kernel evaluates it (ATen Lerp.cuh: the form is chosen by the weight): the device compiler contracts each form
// into ONE fused multiply-add -- measured on gfx950 against torch.lerp, 65 536 random triples: 0 mismatches with the fused forms, 236 (tensor
// weight) / 2212 (scalar weight) with separately rounded products.  This library is built with -ffp-contract=off, so the fusion is spelled out.
__device__ __forceinline__ float qs_lerp(float a, float b, float w) {
    const float d = b - a;
    return fabsf(w) < 0.5f ? fmaf_(w, d, a) : fmaf_(-d, 1.0f - w, b);
}

// ONE block.  Each thread owns 8 consecutive bins; the exclusive scan of the 256 partial sums places the rank in one thread's run.
template <int P>
__global__ __launch_bounds__(QS_BLOCK) void qs_pick_kernel(uint32_t* __restrict__ ws, float weight, float* __restrict__ out3) {
    __shared__ uint32_t part[2][QS_BLOCK];
    constexpr int PER = QS_BINS / QS_BLOCK;
    const int t = threadIdx.x;
    const uint32_t pre[2] = {ws[0], ws[1]};
    const uint32_t rank[2] = {ws[2], ws[3]};
    const bool two = pre[0] != pre[1];
    const uint32_t* g = ws + QS_STATE_WORDS + P * 2 * QS_BINS;
    uint32_t c[2][PER], s[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < PER; j++) {
        c[0][j] = g[t * PER + j];
        c[1][j] = two ? g[QS_BINS + t * PER + j] : c[0][j];
        s[0] += c[0][j];
        s[1] += c[1][j];
    }
    part[0][t] = s[0];
    part[1][t] = s[1];
    __syncthreads();
    for (int d = 1; d < QS_BLOCK; d <<= 1) {                       // Hillis-Steele, inclusive
        uint32_t a0 = 0u, a1 = 0u;
        if (t >= d) { a0 = part[0][t - d]; a1 = part[1][t - d]; }
        __syncthreads();
        part[0][t] += a0;
        part[1][t] += a1;
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        uint32_t before = part[r][t] - s[r];
        if (rank[r] >= before && rank[r] - before < s[r]) {         // exactly one thread: rank < the total by construction
#pragma unroll
            for (int j = 0; j < PER; j++) {
                if (rank[r] - before < c[r][j]) {
                    ws[r] = pre[r] | ((uint32_t)(t * PER + j) << qs_shift(P));
                    ws[2 + r] = rank[r] - before;
                    break;
                }
                before += c[r][j];
            }
        }
    }
    if (P == QS_PASSES - 1) {
        __syncthreads();                                            // the two writers' stores, block scope
        if (t == 0) {
            const float a = qs_value(ws[0]), b = qs_value(ws[1]);
            const bool nan = ws[4] != 0u;
            const float qn = __uint_as_float(0x7fc00000u);
            out3[0] = nan ? qn : a;
            out3[1] = nan ? qn : b;
            out3[2] = nan ? qn : qs_lerp(a, b, weight);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- depth histograms
constexpr int DH_BLOCK = 256;
constexpr int DH_RUN = 4096;                        // pixels of one image per block
constexpr int DH_MAX_BINS = 1024;

__global__ __launch_bounds__(DH_BLOCK) void dh_zero_kernel(int32_t* __restrict__ hist, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * DH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * DH_BLOCK) hist[i] = 0;
}

// torch.histc on a CPU fp32 tensor after the score's clamp (non_flatness_score.py:12, 30): bin = (int)((x - lo) * bins / (hi - lo)), the
// upper end point folded into the last bin; the product is rounded BEFORE the division (ATen HistogramKernel.cpp, linear bins), three
// roundings, none fused.  Dividing first gives the same bin only where `bins` or `hi - lo` is a power of two; elsewhere values next to a
// bin edge change sides.  NaN is counted nowhere (torch.clamp keeps it, histc drops it).
__global__ __launch_bounds__(DH_BLOCK) void depth_histc_kernel(const float* __restrict__ depth, int64_t pixels, float lo, float hi, int bins,
                                                               int32_t* __restrict__ hist) {
    __shared__ uint32_t h[DH_MAX_BINS];
    for (int i = threadIdx.x; i < bins; i += DH_BLOCK) h[i] = 0u;
    __syncthreads();
    const float* __restrict__ row = depth + (int64_t)blockIdx.y * pixels;
    const int64_t p0 = (int64_t)blockIdx.x * DH_RUN;
    const float range = hi - lo, fb = (float)bins;
#pragma unroll 4
    for (int k = 0; k < DH_RUN / DH_BLOCK; k++) {                  // block-uniform trip count: hist_add's ballots see whole waves
        const int64_t p = p0 + k * DH_BLOCK + threadIdx.x;
        const bool inside = p < pixels;
        const float v = inside ? row[p] : lo;
        const float x = fminf(fmaxf(v, lo), hi);
        int b = (int)((x - lo) * fb / range);
        b = min(b, bins - 1);
        hist_add(h, inside && v == v, (uint32_t)b);
    }
    __syncthreads();
    int32_t* __restrict__ g = hist + (int64_t)blockIdx.y * bins;
    for (int i = threadIdx.x; i < bins; i += DH_BLOCK) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&g[i], (int32_t)c);
    }
}

}  // namespace

TDGP_API int64_t tdgp_quantile_select_workspace_bytes(int64_t n) {
    if (n < 1 || n > (int64_t)INT32_MAX) return -1;
    return QS_WS_BYTES;
}

TDGP_API int tdgp_quantile_select(const float* x, int64_t n, int64_t k_lo, int64_t k_hi, float weight, float* out3, void* workspace,
                                  int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(x && out3 && workspace, TDGP_EINVAL, "quantile_select: null pointer");
    TDGP_CHECK(n >= 1 && n <= (int64_t)INT32_MAX, TDGP_EINVAL, "quantile_select: n = %lld outside [1, 2^31 - 1]", (long long)n);
    TDGP_CHECK(k_lo >= 0 && k_lo <= k_hi && k_hi <= k_lo + 1 && k_hi < n, TDGP_EINVAL,
               "quantile_select: ranks (%lld, %lld) need 0 <= k_lo <= k_hi <= k_lo + 1 and k_hi < n = %lld", (long long)k_lo, (long long)k_hi, (long long)n);
    TDGP_CHECK(((uintptr_t)x & 3) == 0 && ((uintptr_t)out3 & 3) == 0 && ((uintptr_t)workspace & 15) == 0, TDGP_EINVAL,
               "quantile_select: x / out3 must be 4-byte aligned and the workspace 16-byte aligned");
    TDGP_CHECK(workspace_bytes >= QS_WS_BYTES, TDGP_EINVAL, "quantile_select: workspace of %lld bytes, %lld needed (workspace too small)",
               (long long)workspace_bytes, (long long)QS_WS_BYTES);
    uint32_t* ws = (uint32_t*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const int words = (int)(QS_WS_BYTES / 4);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(QS_MAX_BLOCKS, cdiv64(n / 4, QS_BLOCK)));
    TDGP_LAUNCH("qs_zero_kernel", qs_zero_kernel, dim3(cdiv(words, QS_BLOCK * 4)), dim3(QS_BLOCK), 0, st, ws, words, (uint32_t)k_lo, (uint32_t)k_hi);
    TDGP_LAUNCH_CHECK();
#define QS_PASS(P)                                                                                                          \
    TDGP_LAUNCH("qs_hist_kernel", qs_hist_kernel<P>, dim3(grid), dim3(QS_BLOCK), 0, st, x, n, ws);                       \
    TDGP_LAUNCH_CHECK();                                                                                                    \
    TDGP_LAUNCH("qs_pick_kernel", qs_pick_kernel<P>, dim3(1), dim3(QS_BLOCK), 0, st, ws, weight, out3);                  \
    TDGP_LAUNCH_CHECK();
    QS_PASS(0)
    QS_PASS(1)
    QS_PASS(2)
#undef QS_PASS
    return TDGP_OK;
}

TDGP_API int tdgp_depth_histc(const float* depth, int64_t images, int64_t pixels, float lo, float hi, int bins, int32_t* hist, tdgp_stream_t stream) {
    TDGP_CHECK(depth && hist, TDGP_EINVAL, "depth_histc: null pointer");
    TDGP_CHECK(bins >= 2 && bins <= DH_MAX_BINS, TDGP_EINVAL, "depth_histc: %d bins outside [2, %d]", bins, DH_MAX_BINS);
    TDGP_CHECK(pixels >= 1 && pixels < ((int64_t)1 << 24), TDGP_EINVAL, "depth_histc: %lld pixels per image outside [1, 2^24)", (long long)pixels);
    TDGP_CHECK(images >= 1 && images <= 65535, TDGP_EINVAL, "depth_histc: %lld images outside [1, 65535]", (long long)images);
    TDGP_CHECK(hi > lo && isfinite(lo) && isfinite(hi), TDGP_EINVAL, "depth_histc: range [%g, %g] must be finite and non-empty", (double)lo, (double)hi);
    hipStream_t st = (hipStream_t)stream;
    const int64_t cells = images * bins;
    TDGP_LAUNCH("dh_zero_kernel", dh_zero_kernel, dim3((int)std::min<int64_t>(1024, cdiv64(cells, DH_BLOCK))), dim3(DH_BLOCK), 0, st, hist, cells);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("depth_histc_kernel", depth_histc_kernel, dim3((unsigned)cdiv64(pixels, DH_RUN), (unsigned)images), dim3(DH_BLOCK), 0, st, depth, pixels,
                lo, hi, bins, hist);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

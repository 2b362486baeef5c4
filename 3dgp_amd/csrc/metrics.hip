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
#include "device_scan.h"
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

// the order-preserving f32_key (device_scan.h) with -0.0 keyed as +0.0 and every NaN as QS_NAN_KEY; key_f32 is its inverse
__device__ __forceinline__ uint32_t qs_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    const uint32_t k = f32_bits_key(u);
    return v != v ? QS_NAN_KEY : k;
}

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
            const float a = key_f32(ws[0]), b = key_f32(ws[1]);
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

// ---------------------------------------------------------------------------------------------------------------- precision / recall k-NN
// The two distance passes of src/metrics/precision_recall.py (torch.cdist in fp16 over 10 000 x 10 000 blocks, every block copied to the
// host, kthvalue / <= there) as ONE tile loop with two epilogues; the distance matrix exists only in accumulator registers.
//
// Contract (include/tdgp.h): features rounded to fp16; d2(i,j) = max(|a_i|^2 + |b_j|^2 - 2 a_i.b_j, 0) with the dot product on
// v_mfma_f32_32x32x16_f16 (fp32 accumulation) and the norms summed in fp32 from the rounded values; d = sqrtf(d2), correctly rounded;
// d rounded once to fp16 (RNE, overflow -> +inf); everything downstream compares those fp16 values; NaN sorts last and compares false.
//
// x -> h(x) = fp16(sqrtf(x)) is monotone, so the tile loop never takes a root: the (k+1)-th smallest h(d2) IS h((k+1)-th smallest d2),
// and h(d2) <= kth[j] IS d2 <= thr[j] with thr[j] the largest fp32 whose h is <= kth[j] (pr_thr_kernel finds it by bisection over the
// bit patterns with the very sqrtf / conversion of the contract).  d2 >= +0 as fp32 bits is an order-preserving uint32 key; a NaN of
// either sign keys above +inf.
//
//   pr_pack_kernel          one wave per row: fp32 -> fp16 (zero padded to Fpad), the row's fp32 norm
//   pr_tile_kernel<EPI,LS>  block = 128 rows x up to PR_JT tiles of 128 columns; 4 waves as 2 x 2, each 64 x 64 = 2 x 2 MFMA tiles.
//                           The COLUMN set is the A operand and the row set the B operand, so a lane holds one row (lane & 31) and 16
//                           columns per tile in its registers: its running state is per row.  K loop: 32 halves per step, register
//                           staged into two LDS buffers (80-byte rows: conflict-free ds_read_b128), one barrier per step.
//       EPI 0 (kth)         per lane and row a sorted list of the LS (4 or 8) smallest keys, one min/max chain per element; at the end
//                           of the block the 4 lists of a row (2 lane halves x 2 column waves) are merged through LDS and the block
//                           writes its list to workspace[split][row][LS]
//       EPI 1 (member)      per lane one bit, any(d2 <= thr[j]); OR-ed through LDS; workspace[split][row] one byte
//   pr_kth_merge_kernel     one thread per row: the lists of all splits -> the (k+1)-th key -> sqrtf -> fp16
//   pr_member_merge_kernel  one thread per probe: OR over the splits
// No atomics, no kernel waits on another block, every partial has one writer: identical bytes from run to run, independent of block order.
namespace {

constexpr int PR_BM = 128;                           // tile side, rows and columns
constexpr int PR_BK = 32;                            // halves per K step (two 32x32x16 MFMA steps)
constexpr int PR_LDK = 40;                           // halves per LDS row: 80 bytes, 5 16-byte slots -> 16 consecutive rows hit 16 distinct slots
constexpr int PR_JT = 8;                             // column tiles per block
constexpr int PR_THREADS = 256;
constexpr int PR_MAX_K1 = 8;
constexpr int64_t PR_MAX_ROWS = (int64_t)1 << 24;
constexpr int PR_MAX_FPAD = 1 << 16;
constexpr uint32_t PR_KEY_LAST = 0xffffffffu;
constexpr int PR_TILE_HALVES = PR_BM * PR_LDK;

typedef _Float16 pr_f16x8 __attribute__((ext_vector_type(8)));
typedef float pr_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float pr_nan() { return __uint_as_float(0x7fc00000u); }

// fp16 bits of the contract's distance for a clamped d2 (NaN canonical)
__device__ __forceinline__ uint16_t pr_dist_bits(float d2) {
    const float d = sqrtf(d2);
    const uint16_t b = __half_as_ushort(__float2half_rn(d));
    return d != d ? (uint16_t)0x7e00u : b;
}

template <int LS>
__device__ __forceinline__ void pr_insert(uint32_t (&l)[LS], uint32_t x) {
#pragma unroll
    for (int t = LS - 1; t > 0; t--) l[t] = max(l[t - 1], min(l[t], x));       // the median of (l[t-1] <= l[t], x)
    l[0] = min(l[0], x);
}

__global__ __launch_bounds__(PR_THREADS) void pr_pack_kernel(const float* __restrict__ x, int64_t n, int F, int Fpad, uint16_t* __restrict__ out,
                                                             float* __restrict__ norms) {
    const int64_t row = (int64_t)blockIdx.x * (PR_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n) return;                                                       // wave-uniform
    const float* __restrict__ src = x + row * F;
    uint16_t* __restrict__ dst = out + row * Fpad;
    float s = 0.f;
    for (int c = lane_id(); c < Fpad; c += 64) {
        const __half h = __float2half_rn(c < F ? src[c] : 0.f);
        const float v = __half2float(h);
        s += v * v;
        dst[c] = __half_as_ushort(h);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane_id() == 0) norms[row] = s;
}

// kth [n] fp16 bits -> thr [n] fp32: the largest d2 with fp16(sqrtf(d2)) <= kth (NaN where none: a NaN or negative kth)
__global__ __launch_bounds__(PR_THREADS) void pr_thr_kernel(const uint16_t* __restrict__ kth, int64_t n, float* __restrict__ thr) {
    const int64_t j = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (j >= n) return;
    const float T = __half2float(__ushort_as_half(kth[j]));
    auto pred = [T](uint32_t key) { return __half2float(__ushort_as_half(pr_dist_bits(__uint_as_float(key)))) <= T; };
    uint32_t lo = 0u, hi = 0x7f800000u;
    float r;
    if (!pred(lo)) {
        r = pr_nan();
    } else if (pred(hi)) {
        r = __uint_as_float(hi);
    } else {
        while (hi - lo > 1u) {                                                  // pred(lo) holds, pred(hi) does not: 31 steps
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (pred(mid)) lo = mid; else hi = mid;
        }
        r = __uint_as_float(lo);
    }
    thr[j] = r;
}

// EPI 0: out = uint32 lists [splits][nr][LS].  EPI 1: out = bytes [splits][nr]; cthr = thr of the columns.
template <int EPI, int LS>
__global__ __launch_bounds__(PR_THREADS) void pr_tile_kernel(const uint16_t* __restrict__ rows, const float* __restrict__ rnorm, int64_t nr,
                                                             const uint16_t* __restrict__ cols, const float* __restrict__ cnorm,
                                                             const float* __restrict__ cthr, int64_t nc, int Fpad, void* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint16_t stage[2][2][PR_TILE_HALVES];      // [buffer][0 columns (A) / 1 rows (B)]
    __shared__ __attribute__((aligned(16))) float cn[PR_BM];                            // norms of the tile's columns, NaN past nc
    __shared__ __attribute__((aligned(16))) float ct[PR_BM];                            // EPI 1: their thresholds, NaN past nc
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wi = w & 1, wj = w >> 1, r = lane & 31, h = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * PR_BM;
    const int64_t jtiles = (nc + PR_BM - 1) / PR_BM;
    const int64_t jt0 = (int64_t)blockIdx.y * PR_JT, jt1 = min(jtiles, jt0 + PR_JT);
    const int ksteps = Fpad / PR_BK;

    // staging: thread t moves 16-byte chunk (t & 3) of rows (t >> 2) and 64 + (t >> 2) of each operand
    const int srow = t >> 2, schunk = (t & 3) * 8;
    const uint16_t* const bsrc0 = rows + min(i0 + srow, nr - 1) * Fpad + schunk;
    const uint16_t* const bsrc1 = rows + min(i0 + srow + 64, nr - 1) * Fpad + schunk;
    const int soff0 = srow * PR_LDK + schunk, soff1 = (srow + 64) * PR_LDK + schunk;
    float na[2];
#pragma unroll
    for (int it = 0; it < 2; it++) na[it] = rnorm[min(i0 + wi * 64 + it * 32 + r, nr - 1)];

    uint32_t list[2][LS];
#pragma unroll
    for (int it = 0; it < 2; it++)
#pragma unroll
        for (int e = 0; e < LS; e++) list[it][e] = PR_KEY_LAST;
    uint32_t hit[2] = {0u, 0u};

    for (int64_t jt = jt0; jt < jt1; jt++) {
        const int64_t j0 = jt * PR_BM;
        const uint16_t* const asrc0 = cols + min(j0 + srow, nc - 1) * Fpad + schunk;
        const uint16_t* const asrc1 = cols + min(j0 + srow + 64, nc - 1) * Fpad + schunk;
        if (t < PR_BM) {
            const bool in = j0 + t < nc;
            cn[t] = in ? cnorm[j0 + t] : pr_nan();
            if (EPI == 1) ct[t] = in ? cthr[j0 + t] : pr_nan();
        }
        pr_f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[a][b][e] = 0.f;

        auto ld = [](const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); };
        auto st = [](uint16_t* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; };
        uint4 ga0 = ld(asrc0), ga1 = ld(asrc1), gb0 = ld(bsrc0), gb1 = ld(bsrc1);
        st(&stage[0][0][soff0], ga0);
        st(&stage[0][0][soff1], ga1);
        st(&stage[0][1][soff0], gb0);
        st(&stage[0][1][soff1], gb1);
        __syncthreads();
        for (int ks = 0; ks < ksteps; ks++) {
            const int cur = ks & 1;
            const bool more = ks + 1 < ksteps;                                  // block-uniform
            if (more) {
                const int ko = (ks + 1) * PR_BK;
                ga0 = ld(asrc0 + ko);
                ga1 = ld(asrc1 + ko);
                gb0 = ld(bsrc0 + ko);
                gb1 = ld(bsrc1 + ko);
            }
#pragma unroll
            for (int kk = 0; kk < PR_BK / 16; kk++) {
                pr_f16x8 fa[2], fb[2];
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    fa[s] = *reinterpret_cast<const pr_f16x8*>(&stage[cur][0][(wj * 64 + s * 32 + r) * PR_LDK + kk * 16 + h * 8]);
                    fb[s] = *reinterpret_cast<const pr_f16x8*>(&stage[cur][1][(wi * 64 + s * 32 + r) * PR_LDK + kk * 16 + h * 8]);
                }
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
            if (more) {
                st(&stage[cur ^ 1][0][soff0], ga0);
                st(&stage[cur ^ 1][0][soff1], ga1);
                st(&stage[cur ^ 1][1][soff0], gb0);
                st(&stage[cur ^ 1][1][soff1], gb1);
            }
            __syncthreads();
        }
        // accumulator element e of tile (a, b): column j0 + wj*64 + a*32 + 8*(e >> 2) + 4*h + (e & 3), row i0 + wi*64 + b*32 + r
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int jl = wj * 64 + a * 32 + 8 * g + 4 * h;
                const float4 nb = *reinterpret_cast<const float4*>(&cn[jl]);
                float4 th = make_float4(0.f, 0.f, 0.f, 0.f);
                if (EPI == 1) th = *reinterpret_cast<const float4*>(&ct[jl]);
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    auto element = [&](float dot, float nbe, float the) {
                        const float d2 = fmaf_(-2.0f, dot, na[b] + nbe);                            // 2 * dot is exact: one rounding
                        if (EPI == 0) pr_insert<LS>(list[b], d2 < 0.f ? 0u : __float_as_uint(d2));   // the sum of two norms is never -0
                        else hit[b] |= d2 <= the ? 1u : 0u;                                          // a negative d2 clamps to 0 <= thr
                    };
                    element(acc[a][b][4 * g + 0], nb.x, th.x);
                    element(acc[a][b][4 * g + 1], nb.y, th.y);
                    element(acc[a][b][4 * g + 2], nb.z, th.z);
                    element(acc[a][b][4 * g + 3], nb.w, th.w);
                }
            }
        __syncthreads();                                                        // cn / ct and the staging buffers are rewritten next
    }

    if (EPI == 0) {
        uint32_t* lds = reinterpret_cast<uint32_t*>(&stage[0][0][0]);           // [128 rows][4 sources][LS]: 16 KiB at LS = 8
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < LS; e++) lds[((wi * 64 + b * 32 + r) * 4 + wj * 2 + h) * LS + e] = list[b][e];
        __syncthreads();
        if (t < PR_BM && i0 + t < nr) {
            uint32_t m[LS];
#pragma unroll
            for (int e = 0; e < LS; e++) m[e] = PR_KEY_LAST;
#pragma unroll
            for (int s = 0; s < 4 * LS; s++) pr_insert<LS>(m, lds[t * 4 * LS + s]);
            uint32_t* dst = reinterpret_cast<uint32_t*>(out) + ((int64_t)blockIdx.y * nr + i0 + t) * LS;
#pragma unroll
            for (int e = 0; e < LS; e++) dst[e] = m[e];
        }
    } else {
        uint32_t* lds = reinterpret_cast<uint32_t*>(&stage[0][0][0]);           // [128 rows][4 sources]
#pragma unroll
        for (int b = 0; b < 2; b++) lds[(wi * 64 + b * 32 + r) * 4 + wj * 2 + h] = hit[b];
        __syncthreads();
        if (t < PR_BM && i0 + t < nr) {
            const uint32_t any = lds[t * 4] | lds[t * 4 + 1] | lds[t * 4 + 2] | lds[t * 4 + 3];
            reinterpret_cast<uint8_t*>(out)[(int64_t)blockIdx.y * nr + i0 + t] = (uint8_t)any;
        }
    }
}

template <int LS>
__global__ __launch_bounds__(PR_THREADS) void pr_kth_merge_kernel(const uint32_t* __restrict__ lists, int64_t nr, int splits, int k1,
                                                                  uint16_t* __restrict__ kth) {
    const int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= nr) return;
    uint32_t m[LS];
#pragma unroll
    for (int e = 0; e < LS; e++) m[e] = PR_KEY_LAST;
    for (int s = 0; s < splits; s++) {
        const uint32_t* src = lists + ((int64_t)s * nr + i) * LS;
#pragma unroll
        for (int e = 0; e < LS; e++) pr_insert<LS>(m, src[e]);
    }
    uint32_t key = m[0];
#pragma unroll
    for (int e = 1; e < LS; e++) key = e == k1 - 1 ? m[e] : key;
    kth[i] = pr_dist_bits(__uint_as_float(key));
}

__global__ __launch_bounds__(PR_THREADS) void pr_member_merge_kernel(const uint8_t* __restrict__ part, int64_t np, int splits, uint8_t* __restrict__ member) {
    const int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= np) return;
    uint8_t any = 0;
    for (int s = 0; s < splits; s++) any |= part[(int64_t)s * np + i];
    member[i] = any ? 1 : 0;
}

inline int64_t pr_splits(int64_t nc) { return cdiv64(cdiv64(nc, PR_BM), PR_JT); }
inline int pr_list_size(int k1) { return k1 <= 4 ? 4 : 8; }
inline int64_t pr_align16(int64_t b) { return (b + 15) & ~(int64_t)15; }
inline bool pr_shape_ok(int64_t n) { return n >= 1 && n <= PR_MAX_ROWS; }

}  // namespace

TDGP_API int tdgp_pr_pack(const float* x, int64_t n, int F, uint16_t* packed, int Fpad, float* norms, tdgp_stream_t stream) {
    TDGP_CHECK(x && packed && norms, TDGP_EINVAL, "pr_pack: null pointer");
    TDGP_CHECK(pr_shape_ok(n), TDGP_EINVAL, "pr_pack: %lld rows outside [1, %lld]", (long long)n, (long long)PR_MAX_ROWS);
    TDGP_CHECK(F >= 1 && Fpad >= F && Fpad % PR_BK == 0 && Fpad <= PR_MAX_FPAD, TDGP_EINVAL,
               "pr_pack: F = %d, Fpad = %d need 1 <= F <= Fpad <= %d and Fpad a multiple of %d", F, Fpad, PR_MAX_FPAD, PR_BK);
    TDGP_CHECK(((uintptr_t)packed & 15) == 0, TDGP_EINVAL, "pr_pack: the packed rows must be 16-byte aligned");
    TDGP_LAUNCH("pr_pack_kernel", pr_pack_kernel, dim3((unsigned)cdiv64(n, PR_THREADS / 64)), dim3(PR_THREADS), 0, (hipStream_t)stream, x, n, F, Fpad,
                packed, norms);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_pr_kth_workspace_bytes(int64_t nr, int64_t nc, int k1) {
    if (!pr_shape_ok(nr) || !pr_shape_ok(nc) || k1 < 1 || k1 > PR_MAX_K1) return -1;
    return pr_align16(pr_splits(nc) * nr * pr_list_size(k1) * 4);
}

TDGP_API int tdgp_pr_kth(const uint16_t* rows, const float* row_norms, int64_t nr, const uint16_t* cols, const float* col_norms, int64_t nc, int Fpad,
                         int k1, uint16_t* kth, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(rows && row_norms && cols && col_norms && kth && workspace, TDGP_EINVAL, "pr_kth: null pointer");
    TDGP_CHECK(pr_shape_ok(nr) && pr_shape_ok(nc), TDGP_EINVAL, "pr_kth: %lld rows x %lld columns outside [1, %lld]", (long long)nr, (long long)nc,
               (long long)PR_MAX_ROWS);
    TDGP_CHECK(k1 >= 1 && k1 <= PR_MAX_K1, TDGP_EINVAL, "pr_kth: k + 1 = %d outside [1, %d]", k1, PR_MAX_K1);
    TDGP_CHECK(k1 <= nc, TDGP_EINVAL, "pr_kth: k + 1 = %d exceeds the %lld columns (k + 1 > Nc)", k1, (long long)nc);
    TDGP_CHECK(Fpad >= PR_BK && Fpad % PR_BK == 0 && Fpad <= PR_MAX_FPAD, TDGP_EINVAL, "pr_kth: Fpad = %d must be a multiple of %d in [%d, %d]", Fpad, PR_BK,
               PR_BK, PR_MAX_FPAD);
    TDGP_CHECK((((uintptr_t)rows | (uintptr_t)cols | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)kth & 1) == 0, TDGP_EINVAL,
               "pr_kth: packed rows and workspace must be 16-byte aligned");
    const int64_t need = tdgp_pr_kth_workspace_bytes(nr, nc, k1);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EINVAL, "pr_kth: workspace of %lld bytes, %lld needed (workspace too small)", (long long)workspace_bytes,
               (long long)need);
    hipStream_t st = (hipStream_t)stream;
    const int splits = (int)pr_splits(nc);
    const dim3 grid((unsigned)cdiv64(nr, PR_BM), (unsigned)splits);
    const float* none = nullptr;
    if (pr_list_size(k1) == 4) {
        TDGP_LAUNCH("pr_tile_kernel_kth", (pr_tile_kernel<0, 4>), grid, dim3(PR_THREADS), 0, st, rows, row_norms, nr, cols, col_norms, none, nc, Fpad, workspace);
        TDGP_LAUNCH_CHECK();
        TDGP_LAUNCH("pr_kth_merge_kernel", pr_kth_merge_kernel<4>, dim3((unsigned)cdiv64(nr, PR_THREADS)), dim3(PR_THREADS), 0, st,
                    (const uint32_t*)workspace, nr, splits, k1, kth);
    } else {
        TDGP_LAUNCH("pr_tile_kernel_kth", (pr_tile_kernel<0, 8>), grid, dim3(PR_THREADS), 0, st, rows, row_norms, nr, cols, col_norms, none, nc, Fpad, workspace);
        TDGP_LAUNCH_CHECK();
        TDGP_LAUNCH("pr_kth_merge_kernel", pr_kth_merge_kernel<8>, dim3((unsigned)cdiv64(nr, PR_THREADS)), dim3(PR_THREADS), 0, st,
                    (const uint32_t*)workspace, nr, splits, k1, kth);
    }
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_pr_member_workspace_bytes(int64_t np, int64_t nc) {
    if (!pr_shape_ok(np) || !pr_shape_ok(nc)) return -1;
    return pr_align16(nc * 4) + pr_align16(pr_splits(nc) * np);
}

TDGP_API int tdgp_pr_member(const uint16_t* probes, const float* probe_norms, int64_t np, const uint16_t* cols, const float* col_norms,
                            const uint16_t* kth, int64_t nc, int Fpad, uint8_t* member, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(probes && probe_norms && cols && col_norms && kth && member && workspace, TDGP_EINVAL, "pr_member: null pointer");
    TDGP_CHECK(pr_shape_ok(np) && pr_shape_ok(nc), TDGP_EINVAL, "pr_member: %lld probes x %lld columns outside [1, %lld]", (long long)np, (long long)nc,
               (long long)PR_MAX_ROWS);
    TDGP_CHECK(Fpad >= PR_BK && Fpad % PR_BK == 0 && Fpad <= PR_MAX_FPAD, TDGP_EINVAL, "pr_member: Fpad = %d must be a multiple of %d in [%d, %d]", Fpad,
               PR_BK, PR_BK, PR_MAX_FPAD);
    TDGP_CHECK((((uintptr_t)probes | (uintptr_t)cols | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)kth & 1) == 0, TDGP_EINVAL,
               "pr_member: packed rows and workspace must be 16-byte aligned");
    const int64_t need = tdgp_pr_member_workspace_bytes(np, nc);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EINVAL, "pr_member: workspace of %lld bytes, %lld needed (workspace too small)", (long long)workspace_bytes,
               (long long)need);
    hipStream_t st = (hipStream_t)stream;
    const int splits = (int)pr_splits(nc);
    float* thr = (float*)workspace;
    uint8_t* part = (uint8_t*)workspace + pr_align16(nc * 4);
    TDGP_LAUNCH("pr_thr_kernel", pr_thr_kernel, dim3((unsigned)cdiv64(nc, PR_THREADS)), dim3(PR_THREADS), 0, st, kth, nc, thr);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("pr_tile_kernel_member", (pr_tile_kernel<1, 4>), dim3((unsigned)cdiv64(np, PR_BM), (unsigned)splits), dim3(PR_THREADS), 0, st, probes,
                probe_norms, np, cols, col_norms, (const float*)thr, nc, Fpad, (void*)part);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("pr_member_merge_kernel", pr_member_merge_kernel, dim3((unsigned)cdiv64(np, PR_THREADS)), dim3(PR_THREADS), 0, st, (const uint8_t*)part, np,
                splits, member);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- FID feature moments
// The raw moments behind the Frechet distance (src/metrics/metric_utils.py:128-161: per feature block `x.sum(0)` and `x.T @ x` in fp64 on
// HOST arrays): s1 += sum of rows, s2 += rows^T rows, for fp32 rows on the device.
//
// Contract (include/tdgp.h): every row value widened fp32 -> fp64 (exact), every product formed in fp64 (exact: 24 + 24 <= 53 bits), only the
// additions round; the Gram part on v_mfma_f64_16x16x4_f64; s2 symmetric bit for bit; no atomics; the partition a function of (n, F) alone.
//
//   mom_tile_kernel<DIRECT>  block = one 64 x 64 tile of s2 ON OR ABOVE the diagonal x one run of rows; 4 waves as 2 x 2, each 32 x 32 = 2 x 2
//                            MFMA tiles (32 accumulator registers).  K loop: 32 rows per step, the two column strips of the rows staged as
//                            fp32 through registers into two LDS buffers (80-float rows: the 4 x 16 fragment reads of a wave half fall on 32
//                            distinct banks), widened at the fragment read, one barrier per step.  A diagonal block stages one strip, skips the
//                            wave below the diagonal and also sums its strip's columns (s1).  Values past n or F are staged as zeros.
//       DIRECT (one run)     adds the tile to s2 in place and writes it to both sides of the diagonal (transposed through LDS, so both
//                            stores are row-contiguous); of a diagonal tile only the elements on or above the diagonal are used
//       otherwise            writes the tile and the column sums to workspace[run]
//   mom_merge_kernel         block = one tile: s2 + the runs' partials in run order, then the same two-sided store; s1 likewise
namespace {

constexpr int MOM_T = 64;                            // tile edge of s2
constexpr int MOM_C = 32;                            // rows per K step
constexpr int MOM_LD = 80;                           // floats per staged LDS row
constexpr int MOM_THREADS = 256;
constexpr int MOM_RUN_MIN = 512;                     // a run of rows is at least this long ...
constexpr int MOM_BLOCKS = 2048;                     // ... and tiles x runs stays within this many blocks
constexpr int MOM_MAX_F = 16384;
constexpr int64_t MOM_MAX_N = (int64_t)1 << 31;
constexpr int MOM_TLD = MOM_T + 1;                   // doubles per row of the epilogue tile
constexpr int MOM_LDS_BYTES = 2 * 2 * MOM_C * MOM_LD * 4;
static_assert(MOM_LDS_BYTES >= MOM_T * MOM_TLD * 8, "the epilogue tile reuses the staging buffers");

struct MomPlan { int t1; int64_t tiles; int64_t run_rows; int64_t runs; };

inline MomPlan mom_plan(int64_t n, int F) {
    MomPlan p;
    p.t1 = cdiv(F, MOM_T);
    p.tiles = (int64_t)p.t1 * (p.t1 + 1) / 2;
    const int64_t max_runs = std::max<int64_t>(1, MOM_BLOCKS / p.tiles);
    p.run_rows = cdiv64(std::max<int64_t>(MOM_RUN_MIN, cdiv64(n, max_runs)), MOM_C) * MOM_C;
    p.runs = std::max<int64_t>(1, cdiv64(n, p.run_rows));
    return p;
}
inline bool mom_shape_ok(int64_t n, int F) { return n >= 0 && n < MOM_MAX_N && F >= 1 && F <= MOM_MAX_F; }

// linear index over the tiles on or above the diagonal, row by row -> (ti <= tj)
__device__ __forceinline__ void mom_tile_of(int idx, int t1, int& ti, int& tj) {
    int i = 0;
    while (idx >= t1 - i) { idx -= t1 - i; i++; }
    ti = i;
    tj = i + idx;
}

// the finished tile in LDS (`tile[r][c]` = s2[f0 + r][g0 + c]) -> both sides of the diagonal; a diagonal tile is read on or above its diagonal only
__device__ __forceinline__ void mom_store_tile(const double* tile, double* __restrict__ s2, int F, int f0, int g0, bool diag) {
    for (int idx = threadIdx.x; idx < MOM_T * MOM_T; idx += MOM_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        if (diag) {
            if (f0 + r < F && f0 + c < F) s2[(int64_t)(f0 + r) * F + f0 + c] = r <= c ? tile[r * MOM_TLD + c] : tile[c * MOM_TLD + r];
        } else {
            if (f0 + r < F && g0 + c < F) s2[(int64_t)(f0 + r) * F + g0 + c] = tile[r * MOM_TLD + c];
            if (g0 + r < F && f0 + c < F) s2[(int64_t)(g0 + r) * F + f0 + c] = tile[c * MOM_TLD + r];
        }
    }
}

template <bool DIRECT>
__global__ __launch_bounds__(MOM_THREADS) void mom_tile_kernel(const float* __restrict__ rows, int64_t n, int F, int t1, int64_t run_rows,
                                                               double* __restrict__ s1, double* __restrict__ s2, double* __restrict__ ws2,
                                                               double* __restrict__ ws1) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[MOM_LDS_BYTES];
    __shared__ double red[MOM_THREADS / 64][MOM_T];
    float* const stage = reinterpret_cast<float*>(lds_raw);                     // [buffer][0 strip f / 1 strip g][MOM_C][MOM_LD]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wi = w >> 1, wj = w & 1, lc = lane & 15, lk = lane >> 4;
    int ti, tj;
    mom_tile_of((int)blockIdx.x, t1, ti, tj);
    const bool diag = ti == tj;
    const int f0 = ti * MOM_T, g0 = tj * MOM_T;
    const int64_t k0 = (int64_t)blockIdx.y * run_rows, k1 = min(n, k0 + run_rows);
    const int ksteps = (int)((k1 - k0 + MOM_C - 1) / MOM_C);
    const bool work = !diag || wi <= wj;                                         // wave-uniform

    // staging: thread t moves column (t & 63) of rows (t >> 6) + 4 i of each strip
    const int sc = t & 63, sr = t >> 6;
    const bool fin = f0 + sc < F, gin = !diag && g0 + sc < F;
    const float* const fsrc = rows + f0 + sc;
    const float* const gsrc = rows + g0 + sc;
    float rf[MOM_C / 4], rg[MOM_C / 4];
    auto fetch = [&](int ks) {
        const int64_t kb = k0 + (int64_t)ks * MOM_C + sr;
#pragma unroll
        for (int i = 0; i < MOM_C / 4; i++) {
            const int64_t k = kb + 4 * i;
            rf[i] = fin && k < k1 ? fsrc[k * F] : 0.f;
            rg[i] = gin && k < k1 ? gsrc[k * F] : 0.f;
        }
    };
    auto put = [&](int buf) {
        float* const a = stage + (buf * 2 + 0) * MOM_C * MOM_LD + sr * MOM_LD + sc;
        float* const b = stage + (buf * 2 + 1) * MOM_C * MOM_LD + sr * MOM_LD + sc;
#pragma unroll
        for (int i = 0; i < MOM_C / 4; i++) {
            a[4 * i * MOM_LD] = rf[i];
            if (!diag) b[4 * i * MOM_LD] = rg[i];
        }
    };

    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[a][b][e] = 0.0;
    double colsum = 0.0;

    fetch(0);
    put(0);
    __syncthreads();
    for (int ks = 0; ks < ksteps; ks++) {
        const int cur = ks & 1;
        const bool more = ks + 1 < ksteps;                                      // block-uniform
        if (more) fetch(ks + 1);
        const float* const A = stage + (cur * 2 + 0) * MOM_C * MOM_LD;
        const float* const B = diag ? A : stage + (cur * 2 + 1) * MOM_C * MOM_LD;
        if (work) {
#pragma unroll
            for (int kk = 0; kk < MOM_C / 4; kk++) {
                const int kr = (kk * 4 + lk) * MOM_LD;
                double fa[2], fb[2];
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    fa[s] = (double)A[kr + wi * 32 + s * 16 + lc];
                    fb[s] = (double)B[kr + wj * 32 + s * 16 + lc];
                }
                mfma_f64_2x2(fa, fb, acc);
            }
        }
        if (diag) {
#pragma unroll
            for (int i = 0; i < MOM_C / 4; i++) colsum += (double)A[(sr * (MOM_C / 4) + i) * MOM_LD + sc];
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }

    // column sums of a diagonal block: the four row groups in a fixed order
    if (diag) {
        red[sr][sc] = colsum;
        __syncthreads();
        if (t < MOM_T && f0 + t < F) {
            const double v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
            if (DIRECT) s1[f0 + t] += v;
            else ws1[((int64_t)blockIdx.y * t1 + ti) * MOM_T + t] = v;
        }
    }

    // the wave's output starts at row (feature f) f0 + wi*32, column (feature g) g0 + wj*32 (element map: common.h)
    if (DIRECT) {
        double* const tile = reinterpret_cast<double*>(lds_raw);                // the K loop's last barrier is behind every read of `stage`
        if (work) {
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int r = wi * 32 + a * 16 + lk + 4 * e, c = wj * 32 + b * 16 + lc;
                        const bool in = f0 + r < F && g0 + c < F;
                        const double old = in ? s2[(int64_t)(f0 + r) * F + g0 + c] : 0.0;
                        tile[r * MOM_TLD + c] = old + acc[a][b][e];
                    }
        }
        __syncthreads();
        mom_store_tile(tile, s2, F, f0, g0, diag);
    } else if (work) {
        double* const dst = ws2 + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (MOM_T * MOM_T);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int e = 0; e < 4; e++) dst[(wi * 32 + a * 16 + lk + 4 * e) * MOM_T + wj * 32 + b * 16 + lc] = acc[a][b][e];
    }
}

__global__ __launch_bounds__(MOM_THREADS) void mom_merge_kernel(const double* __restrict__ ws2, const double* __restrict__ ws1, int runs, int F, int t1,
                                                                double* __restrict__ s1, double* __restrict__ s2) {
    __shared__ double tile[MOM_T * MOM_TLD];
    const int t = threadIdx.x;
    int ti, tj;
    mom_tile_of((int)blockIdx.x, t1, ti, tj);
    const bool diag = ti == tj;
    const int f0 = ti * MOM_T, g0 = tj * MOM_T;
    for (int idx = t; idx < MOM_T * MOM_T; idx += MOM_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        if (f0 + r < F && g0 + c < F && (!diag || (r >> 5) <= (c >> 5))) {      // a diagonal block's wave below the diagonal wrote nothing
            double v = s2[(int64_t)(f0 + r) * F + g0 + c];
            for (int s = 0; s < runs; s++) v += ws2[((int64_t)s * gridDim.x + blockIdx.x) * (MOM_T * MOM_T) + idx];
            tile[r * MOM_TLD + c] = v;
        }
    }
    if (diag && t < MOM_T && f0 + t < F) {
        double v = s1[f0 + t];
        for (int s = 0; s < runs; s++) v += ws1[((int64_t)s * t1 + ti) * MOM_T + t];
        s1[f0 + t] = v;
    }
    __syncthreads();
    mom_store_tile(tile, s2, F, f0, g0, diag);
}

}  // namespace

TDGP_API int64_t tdgp_moments_workspace_bytes(int64_t n, int F) {
    if (!mom_shape_ok(n, F)) return -1;
    const MomPlan p = mom_plan(n, F);
    if (p.runs == 1) return 16;                                                 // one run adds in place: the workspace is not touched
    return p.runs * (p.tiles * MOM_T * MOM_T + (int64_t)p.t1 * MOM_T) * 8;
}

TDGP_API int tdgp_moments_add(const float* rows, int64_t n, int F, double* s1, double* s2, void* workspace, int64_t workspace_bytes,
                              tdgp_stream_t stream) {
    TDGP_CHECK(mom_shape_ok(n, F), TDGP_EINVAL, "moments_add: n = %lld, F = %d outside 0 <= n < 2^31, 1 <= F <= %d", (long long)n, F, MOM_MAX_F);
    if (n == 0) return TDGP_OK;                                                  // nothing to add, whatever the pointers
    TDGP_CHECK(rows && s1 && s2 && workspace, TDGP_EINVAL, "moments_add: null pointer");
    TDGP_CHECK(((uintptr_t)rows & 3) == 0 && (((uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)workspace) & 7) == 0, TDGP_EINVAL,
               "moments_add: rows must be 4-byte aligned, s1 / s2 / workspace 8-byte aligned");
    const int64_t need = tdgp_moments_workspace_bytes(n, F);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EINVAL, "moments_add: workspace of %lld bytes, %lld needed (workspace too small)", (long long)workspace_bytes,
               (long long)need);
    const MomPlan p = mom_plan(n, F);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.runs);
    if (p.runs == 1) {
        double* none = nullptr;
        TDGP_LAUNCH("mom_tile_kernel_direct", mom_tile_kernel<true>, grid, dim3(MOM_THREADS), 0, st, rows, n, F, p.t1, p.run_rows, s1, s2, none, none);
        TDGP_LAUNCH_CHECK();
        return TDGP_OK;
    }
    double* ws2 = (double*)workspace;
    double* ws1 = ws2 + p.runs * p.tiles * MOM_T * MOM_T;
    TDGP_LAUNCH("mom_tile_kernel_runs", mom_tile_kernel<false>, grid, dim3(MOM_THREADS), 0, st, rows, n, F, p.t1, p.run_rows, s1, s2, ws2, ws1);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("mom_merge_kernel", mom_merge_kernel, dim3((unsigned)p.tiles), dim3(MOM_THREADS), 0, st, (const double*)ws2, (const double*)ws1, (int)p.runs,
                F, p.t1, s1, s2);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// sampling.hip -- per-ray stages of the volumetric renderer: stratified samples, ray marchers,
// hierarchical importance resampling, depth merge + alpha compositing.
//
// Replaces ~40 eager PyTorch ops per chunk of src/training/tri_plane_renderer.py:
//   :208-235 sample_stratified      :353-405 ClassicalRayMarcher     :300-348 MipRayMarcher2
//   :237-255 sample_importance      :257-295 sample_pdf              :196-206 unify_samples
//
// Mapping: ONE 64-lane wavefront per ray (4 rays per 256-thread block), samples across lanes, per-wave LDS
// scratch, no block-level synchronisation.
// Arithmetic (r02): the marchers are the reference's own fp32 chain -- delta, softplus = log1p(exp(x)), alpha = 1 - exp(-delta*sigma),
// transmittance = cumprod, weights, weighted sums -- on fp32 OCML transcendentals (<= 1 ulp), fp32 DPP wave scans and fp32 wave
// sums.  r01 evaluated the transcendentals, scans and sums in fp64 to be bit-identical to the CPU oracle (which rounds the exact
// value once); that cost 2-3x the instructions (fp64 exp / log1p, two-register DPP moves, half-rate adds) for an agreement that
// is not the reference's either (torch's expf is Sleef's 1-ulp routine, its sums fp32 cascades).  What has to be EXACT is kept
// exact: sample_pdf's normaliser follows torch's summation order, the cdf is torch's sequential-double cumsum rounded per prefix,
// so for given weights the searchsorted indices and the fine samples equal the reference's bit for bit (the stage-level tests).
//
// Written once, fence-free functions (or statements) of one ray's LDS pointers and per-lane state, for the one-ray kernels (stage, wave_sync(),
// next stage) and the 64 + 64 pair kernels (stage for ray A, for ray B, wave_sync()) alike:
//   TDGP_CLASSICAL_ALPHA / TDGP_MIP_ALPHA   alpha and transmittance factor of a sample (both marchers, every branch; both pair marches)
//   TDGP_MARCH_PASS / TDGP_MARCH_PASS2      the fp64-scan pass of a march and its two-chunk side-by-side form
//   smooth_read / smooth_write / offset_weights / pdf_cdf / cdf_search / cdf_sample   the importance stages (importance_lds = all of them)
//   wave_bitonic_sort_n<NS>                 the (key, index) network, NS = 1, 2, 4, 8 slots per lane
//   stable_ranks<NR> over stable_ranks_n    the brute-force stable rank and its one dispatcher (short and long lists)
//   TDGP_LAUNCH_RAYS                        the launch of every per-ray kernel family; an entry point selects an instantiation once
// The first two are statement macros: as functions they change the instruction text of all ten one-ray kernels that hold a marcher, as text none.
// Specialised copies in the pair section, each restating the one-ray text it names at 64 / 128 (profiles/ray_tail_refactor_ab.json):
//   torch_order_sum_62      torch_order_sum_lds, branch n >= 8 at nv = 7, for the pair kernel's pdf row (pdf_cdf<true>)
//   imp_count / imp_gather  the counting rank of importance_from_coarse_kernel's N <= 64 / N <= 128 blocks: behind one count_rank<NS> for all
//                           three, importance_from_coarse_kernel<128> / <256> go from 57 / 97 to 65 / 104 VGPRs (7 instead of 8 waves per SIMD at <128>)
//   mrg_search / _scatter_last / _ranks / mrg_scatter / mrg_composite   merge_composite_kernel's merge ranks, scatter and composite: as shared
//                           stage functions merge_composite_pair_kernel goes from 572 to 606 us (parent spread 6) and merge_composite_kernel<512>
//                           at 256 + 256 from 550 to 566 us (spread 2)
#include "common.h"

namespace {

constexpr int MAXS = 256;          // capacity of the short-ray kernels: samples per ray in one pass (2*S for the merged pass)
constexpr int RAYS_PER_BLOCK = 4;
// Long rays: the same one-wave-per-ray kernels instantiated at larger capacities, launched only above
// the short kernels' thresholds.  A pass (coarse S, fine N, a pdf row of S - 2 <= 510 entries) holds at most MAXS_PASS samples: beyond 512
// the pdf normaliser would reach a level of torch's cascade sum that torch_order_sum_lds does not restate.  A merged list holds at most
// MAXS_LONG = 2 * MAXS_PASS.
constexpr int MAXS_PASS = 512;
constexpr int MAXS_LONG = 1024;

// Per-wave LDS scratch.  MS = capacity in samples; the fused kernels pick 128 when the ray fits (4.1 KB per wave -> 8 waves
// per SIMD instead of 4: these kernels are chains of dependent LDS / cross-lane steps, occupancy is what hides them).
template <int MS>
struct alignas(16) WaveScratchT {
    float z[MS];        // depths (s- or t-space)
    float sig[MS];      // densities
    float w[MS + 4];    // weights / pdf scratch
    float cdf[MS];
    float bins[MS];
    float col[3][MS];   // colours (merged pass)
};
using WaveScratch = WaveScratchT<MAXS>;

// The plain marcher reads only z / sig / w: its long form (MS = MAXS_LONG) keeps only those (12.3 KB per wave instead of 32.8 KB).
template <int MS> struct alignas(16) MarchScratchT { float z[MS]; float sig[MS]; float w[MS + 4]; };
template <> struct alignas(16) MarchScratchT<MAXS> : WaveScratch {};      // the short form keeps its layout
// unify_samples ranks the depths only.
template <int MS> struct alignas(16) UnifyScratchT { float z[MS]; };
template <> struct alignas(16) UnifyScratchT<MAXS> : WaveScratch {};

__device__ __forceinline__ void wave_sync() {
    // all LDS traffic of a wave is issued in order; this only stops the compiler from reordering across it
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float s2t(float s, float t_near, float t_far) { return s * t_far + (1.0f - s) * t_near; }

// ------------------------------------------------------------------------------------------------
// classical marcher on LDS-resident depths/densities: writes weights w[0..S), returns (final_T, sum w).
// tri_plane_renderer.py:355-387.
// flags: bit0 use_inf_depth, bit1 last_back, bit3 relu clamp
// ------------------------------------------------------------------------------------------------
// LONGX: a list longer than MAXS (the long-ray kernels only).  alpha = 1 - exp(-delta sigma) cancels: with delta ~ 1 / S its relative
// error is exp's ulp over delta sigma, and at 768 samples a 1-ulp expf left the image 2.6x further (mean) from the reference's float64
// run than the reference's own fp32 run.  The long form rounds exp once from fp64 (the exactly rounded expf but for ~2^-29 of inputs).
template <bool LONGX>
__device__ __forceinline__ float exp_neg(float x) { return LONGX ? (float)exp(-(double)x) : expf(-x); }

// alpha_i and the transmittance factor (1 - alpha_i) + 1e-10 of sample i < S (classical; tri_plane_renderer.py:362-372) or of mid-point sample
// i < M (mip; :313-330) of an LDS-resident list of S samples, (0, 1) past the end: the only place these expressions are written.  Statements, not functions:
// behind a call (inlined or not) the compiler folds the marchers' `M = (flags & 1) ? S : S - 1` differently and every kernel with a marcher
// changes; as text the one-ray kernels keep their code to the instruction.
#define TDGP_CLASSICAL_ALPHA(LONGX, z, sig, i, S, flags, cut_thr, alpha, fac)                                        \
    do {                                                                                                            \
        alpha = 0.f; fac = 1.0f;                                                                                    \
        if ((i) < (S)) {                                                                                            \
            const float delta = ((i) < (S) - 1) ? (z[(i) + 1] - z[i]) : (((flags) & 1) ? 1e10f : 1e-3f);            \
            float sp = ((flags) & 8) ? (sig[i] > 0.f ? sig[i] : 0.f) : softplus20f(sig[i]);                         \
            if (sp < cut_thr) sp = 0.f; /* cut_quantile (:366-368); cut_thr = 0 never cuts (sp >= 0) */             \
            alpha = 1.0f - exp_neg<LONGX>(delta * sp);                                                              \
            fac = (1.0f - alpha) + 1e-10f;                                                                          \
        }                                                                                                           \
    } while (0)

#define TDGP_MIP_ALPHA(LONGX, z, sig, i, S, M, density_bias, cut_thr, alpha, fac)                                    \
    do {                                                                                                            \
        alpha = 0.f; fac = 1.0f;                                                                                    \
        if ((i) < (M)) {                                                                                            \
            float delta, smid;                                                                                      \
            if ((i) < (S) - 1) { delta = z[(i) + 1] - z[i]; smid = (sig[i] + sig[(i) + 1]) / 2.f; }                 \
            else { delta = 1e10f; smid = sig[(S) - 1]; }                                                            \
            float sp = softplus20f(smid + density_bias);                                                            \
            if (sp < cut_thr) sp = 0.f; /* cut_quantile (:324-326) */                                               \
            float dd = sp * delta;                                                                                  \
            alpha = 1.0f - exp_neg<LONGX>(dd);                                                                      \
            fac = (1.0f - alpha) + 1e-10f;                                                                          \
        }                                                                                                           \
    } while (0)

// One 64-sample pass of a march: lane l's weight `wi` = alpha * (exclusive prefix product of the factors), `carry` = the product so far,
// `incl64` = the pass's fp64 prefixes (their last lane is the next carry).  Statements for the same reason.  DECLARATIONS in the caller's
// scope, so never the body of an unbraced if / for, once per scope: `wi`, `incl64` (named at the call) and `incl`, `excl` (not named there).
// transmittance = torch.cumprod on the CPU: prefixes accumulated in fp64, each rounded to fp32.  The fp64 DPP
// scan (6 steps of 2 moves + 1 v_mul_f64) rounds to the same fp32 prefix as the sequential fp64 product except with probability
// ~2^-29 per element.  Round 5: the fp32 scan used since round 2 left the composited depth 2.4e-7 (2 ulp) from the reference's
// float64 image on average where the reference's own fp32 run sits at 0.9e-7 (e2e_full_c3) -- with this it is level.
#define TDGP_MARCH_PASS(wi, incl64, alpha, fac, carry)                   \
    const double incl64 = wave_scan_f64<true>((double)(fac)) * (carry);  \
    const float incl = (float)incl64;                                    \
    const float excl = wave_shr1_f32(incl, (float)(carry));              \
    const float wi = (alpha) * excl;
// Two passes (a list of 65..128 samples) SIDE BY SIDE: both chunks' prefix products are two independent dependency chains the scheduler
// interleaves, joined by the one multiplication that couples them, where two TDGP_MARCH_PASS run one after the other -- and these kernels
// are bound by the length of a wave's dependent chain at the SIMD's 8-wave occupancy.  Same operations on the same values
// (the first chunk's `* carry` is `* 1.0`): same bits.  `i1` = the second chunk's fp64 prefixes.  `alpha` and `fac` are float[2].  Declares `wi0`,
// `wi1`, `i1` (named at the call) and `s0`, `s1`, `c1`, `incl0`, `incl1` (not named there) in the caller's scope, under the same rules.
#define TDGP_MARCH_PASS2(wi0, wi1, i1, alpha, fac)                                                                          \
    const double s0 = wave_scan_f64<true>((double)fac[0]), s1 = wave_scan_f64<true>((double)fac[1]);                        \
    const double c1 = wave_last_f64(s0);                                                                                    \
    const double i1 = s1 * c1;                                                                                              \
    const float incl0 = (float)s0, incl1 = (float)i1;                                                                       \
    const float wi0 = alpha[0] * wave_shr1_f32(incl0, 1.0f), wi1 = alpha[1] * wave_shr1_f32(incl1, (float)c1);

template <bool LONGX = false>
__device__ void march_classical_lds(const float* z, const float* sig, float* w, int S, int flags, float cut_thr, float& final_T, float& wagg) {
    const int l = lane_id();
    double carry = 1.0;
    float wsum = 0.0f;
    if (S > 64 && S <= 128) {
        // two chunks of 64 samples (the merged 64 + 64 list): their softplus / exp / prefix products side by side (TDGP_MARCH_PASS2)
        float alpha[2], fac[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int i = 64 * c + l;
            TDGP_CLASSICAL_ALPHA(LONGX, z, sig, i, S, flags, cut_thr, alpha[c], fac[c]);
        }
        TDGP_MARCH_PASS2(wi0, wi1, i1, alpha, fac)
        w[l] = wi0; wsum += wi0;
        if (64 + l < S) { w[64 + l] = wi1; wsum += wi1; }
        carry = wave_last_f64(i1);
    } else
    for (int base = 0; base < S; base += 64) {
        const int i = base + l;
        float alpha, fac;
        TDGP_CLASSICAL_ALPHA(LONGX, z, sig, i, S, flags, cut_thr, alpha, fac);
        TDGP_MARCH_PASS(wi, incl64, alpha, fac, carry)
        if (i < S) { w[i] = wi; wsum += wi; }
        carry = wave_last_f64(incl64);
    }
    wagg = wave_sum_f32(wsum);
    final_T = (float)carry;
    wave_sync();
    if ((flags & 2) && l == 0) w[S - 1] += (1.0f - wagg);
    wave_sync();
}

// mip marcher weights on LDS-resident data: M = S (inf depth) or S-1 mid-point samples.
// tri_plane_renderer.py:305-334.
template <bool LONGX = false>
__device__ void march_mip_lds(const float* z, const float* sig, float* w, int S, int flags, float density_bias, float cut_thr, float& final_T,
                              float& wagg) {
    const int l = lane_id();
    const int M = (flags & 1) ? S : S - 1;
    double carry = 1.0;
    float wsum = 0.0f;
    for (int base = 0; base < M; base += 64) {
        const int i = base + l;
        float alpha, fac;
        TDGP_MIP_ALPHA(LONGX, z, sig, i, S, M, density_bias, cut_thr, alpha, fac);
        TDGP_MARCH_PASS(wi, incl64, alpha, fac, carry)
        if (i < M) { w[i] = wi; wsum += wi; }
        carry = wave_last_f64(incl64);
    }
    wagg = wave_sum_f32(wsum);
    final_T = (float)carry;
    wave_sync();
}

// ------------------------------------------------------------------------------------------------
// torch.sum(x, -1) of the reference's CPU path over x[i] = w1[i] + eps, i < n, IN TORCH'S OWN ORDER: the value is
// sample_pdf's normaliser (tri_plane_renderer.py:272) and its last bit decides which cdf knot a draw falls behind,
// i.e. the searchsorted indices.  ATen's sum kernel (cpu/SumKernel.cpp, AVX2 dispatch: 8 fp32 lanes) cuts the row
// into nv = n/8 vectors, adds them into 4 interleaved vector accumulators (acc[k] += V[4i+k]), the nv%4 left-over
// vectors into accumulator 0, then acc0 += acc1, acc2, acc3, and finally a scalar takes the n%8 tail elements in
// order followed by the 8 lanes of acc0 in order (ATen's cascade_sum folds its accumulators every 16 groups of 4 x 8 lanes: the order
// first changes at 18 groups = 576 elements; n <= MAXS_PASS - 2 = 510 here, checked on the host).
// Rows shorter than 8 run the same scheme on scalars.  Lane (a = (l>>3)&3, col = l&7) plays lane col of accumulator a;
// every lane returns the result.
// ------------------------------------------------------------------------------------------------
__device__ float torch_order_sum_lds(const float* w1, int n, float eps) {
    const int l = lane_id();
    if (n >= 8) {
        const int nv = n >> 3, nilp = nv >> 2;
        const int col = l & 7, a = (l >> 3) & 3;
        float acc = 0.f;
        for (int i = 0; i < nilp; i++) acc = __fadd_rn(acc, __fadd_rn(w1[(4 * i + a) * 8 + col], eps));
        for (int j = 4 * nilp; j < nv; j++) {
            const float v = __fadd_rn(w1[j * 8 + col], eps);
            if (a == 0) acc = __fadd_rn(acc, v);
        }
        float p = __shfl(acc, col, 64);
        p = __fadd_rn(p, __shfl(acc, col + 8, 64));
        p = __fadd_rn(p, __shfl(acc, col + 16, 64));
        p = __fadd_rn(p, __shfl(acc, col + 24, 64));
        float fin = 0.f;
        for (int k = nv * 8; k < n; k++) fin = __fadd_rn(fin, __fadd_rn(w1[k], eps));
#pragma unroll
        for (int c = 0; c < 8; c++) fin = __fadd_rn(fin, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), c)));      // lanes 0..7: scalar reads, no LDS permute
        return fin;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int nilp = n >> 2;                       // 0 or 1
    if (nilp)
        for (int k = 0; k < 4; k++) acc[k] = __fadd_rn(acc[k], __fadd_rn(w1[k], eps));
    for (int r = 4 * nilp; r < n; r++) acc[0] = __fadd_rn(acc[0], __fadd_rn(w1[r], eps));
    for (int k = 1; k < 4; k++) acc[0] = __fadd_rn(acc[0], acc[k]);
    return acc[0];
}

// torch_order_sum_lds for 56 <= n <= 62 (a pdf row of 61 or 62 entries): nv = 7 vectors, one interleaved group, vectors 4..6 into accumulator 0, n - 56 tail elements
__device__ __forceinline__ float torch_order_sum_62(const float* w1, int n, float eps) {
    const int l = lane_id();
    const int col = l & 7, a = (l >> 3) & 3;
    float acc = 0.f;
    acc = __fadd_rn(acc, __fadd_rn(w1[a * 8 + col], eps));
#pragma unroll
    for (int j = 4; j < 7; j++) {
        const float v = __fadd_rn(w1[j * 8 + col], eps);
        if (a == 0) acc = __fadd_rn(acc, v);
    }
    float p = __shfl(acc, col, 64);
    p = __fadd_rn(p, __shfl(acc, col + 8, 64));
    p = __fadd_rn(p, __shfl(acc, col + 16, 64));
    p = __fadd_rn(p, __shfl(acc, col + 24, 64));
    float fin = 0.f;
#pragma unroll
    for (int k = 56; k < 62; k++) {
        const float t = __fadd_rn(fin, __fadd_rn(w1[k], eps));
        fin = k < n ? t : fin;
    }
#pragma unroll
    for (int c = 0; c < 8; c++) fin = __fadd_rn(fin, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), c)));
    return fin;
}

// ------------------------------------------------------------------------------------------------
// sample_importance + sample_pdf (tri_plane_renderer.py:237-295) on one ray's LDS-resident z[S] (s-space)
// and weights w[Wn], as fence-free stages: the caller puts a wave_sync() between them (importance_lds below; the pair kernel for two rays).
// ------------------------------------------------------------------------------------------------
// mip smoothing of the weights, in two stages through registers (slot c of lane l = weight l + 64 c):
// max_pool1d(2,1,pad 1) -> Wn+1, avg_pool1d(2,1) -> Wn, + 0.01
template <int NV>
__device__ __forceinline__ void smooth_read(const float* w, int Wn, float (&nv)[NV]) {
    const int l = lane_id();
#pragma unroll
    for (int c = 0; c < NV; c++) {
        const int i = l + 64 * c;
        if (i < Wn) {
            float a = (i - 1 >= 0) ? w[i - 1] : -INFINITY, b = w[i], d = (i + 1 < Wn) ? w[i + 1] : -INFINITY;
            float t0 = a > b ? a : b;      // tmp[i]   = max(w[i-1], w[i])
            float t1 = b > d ? b : d;      // tmp[i+1] = max(w[i], w[i+1])
            nv[c] = (t0 + t1) / 2.f + 0.01f;
        }
    }
}
template <int NV>
__device__ __forceinline__ void smooth_write(float* w, int Wn, const float (&nv)[NV]) {
    const int l = lane_id();
#pragma unroll
    for (int c = 0; c < NV; c++) {
        const int i = l + 64 * c;
        if (i < Wn) w[i] = nv[c];
    }
}
// the classical marcher's weights + 1e-5
__device__ __forceinline__ void offset_weights(float* w, int Wn) {
    for (int i = lane_id(); i < Wn; i += 64) w[i] = w[i] + 1e-5f;
}
// bins, the pdf normaliser in torch's fp32 accumulation order (not the exactly rounded sum: the integer rows depend on it), cdf = [0, cumsum(pdf)]
// as the fp64 scan rounded per prefix.  ROW62: the row has 56..62 entries (S = 64) and the normaliser is torch_order_sum_62.
template <bool ROW62>
__device__ __forceinline__ void pdf_cdf(const float* z, const float* w, float* bins, float* cdf, int S, int Wn) {
    const int l = lane_id();
    const float eps = 1e-5f;
    const int nb = S - 1, ns = Wn - 2;
    for (int i = l; i < nb; i += 64) bins[i] = 0.5f * (z[i] + z[i + 1]);
    const float totf = ROW62 ? torch_order_sum_62(w + 1, ns, eps) : torch_order_sum_lds(w + 1, ns, eps);
    double carry = 0.0;
    if (l == 0) cdf[0] = 0.f;
    for (int base = 0; base < ns; base += 64) {
        const int i = base + l;
        float pdf = (i < ns) ? (w[1 + i] + eps) / totf : 0.f;
        double incl = wave_scan_f64<false>((double)pdf) + carry;
        if (i < ns) cdf[i + 1] = (float)incl;
        carry = wave_last_f64(incl);
    }
}
// searchsorted(right=True): the first of the nc knots with cdf > u
__device__ __forceinline__ int cdf_search(const float* cdf, int nc, float uu) {
    int lo = 0, hi = nc;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (cdf[mid] <= uu) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the sample of draw u behind knot `ind`: linear in its bin
__device__ __forceinline__ float cdf_sample(const float* cdf, const float* bins, int nb, int ns, int ind, float uu, int& below, int& above) {
    const float eps = 1e-5f;
    below = ind - 1 < 0 ? 0 : ind - 1;
    above = ind > ns ? ns : ind;
    const float cb = cdf[below], ca = cdf[above];
    const float bb = bins[below < nb ? below : nb - 1], ba = bins[above < nb ? above : nb - 1];
    float denom = ca - cb;
    if (denom < eps) denom = 1.f;
    return bb + (uu - cb) / denom * (ba - bb);
}

// All stages on one ray.  Clobbers sc.w / sc.cdf / sc.bins.  Lane j produces sample j (strided by 64).  `emit(j, sample, ind, below, above)`
// consumes the results.
template <typename SC, typename GetU, typename Emit>
__device__ void importance_lds(SC& sc, int S, int Wn, GetU getu, int N, int mip, Emit emit) {
    const int l = lane_id();
    float* w = sc.w;
    constexpr int CAP = sizeof(sc.z) / sizeof(float), NV = (CAP > MAXS ? CAP : MAXS) / 64;
    if (mip) {
        float nv[NV];
        smooth_read<NV>(w, Wn, nv);
        wave_sync();
        smooth_write<NV>(w, Wn, nv);
    } else {
        offset_weights(w, Wn);
    }
    wave_sync();
    const int nb = S - 1, ns = Wn - 2, nc = ns + 1;
    pdf_cdf<false>(sc.z, w, sc.bins, sc.cdf, S, Wn);
    wave_sync();
    for (int j = l; j < N; j += 64) {
        const float uu = getu(j);
        const int ind = cdf_search(sc.cdf, nc, uu);
        int below, above;
        const float smp = cdf_sample(sc.cdf, sc.bins, nb, ns, ind, uu, below, above);
        emit(j, smp, ind, below, above);
    }
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// One stratified sample (tri_plane_renderer.py:225-233): lin = torch.linspace(0, 1, S) on the CPU, one fused multiply-add per element
// (camera_rays.hip:linspace_f).
__device__ __forceinline__ float strat_one(float u, int k, int S, float step, int marcher) {
    auto lin = [&](int q) { return (S == 1) ? 0.f : ((q < S / 2) ? __fmaf_rn(step, (float)q, 0.f) : __fmaf_rn(-step, (float)(S - 1 - q), 1.f)); };
    if (marcher == 0) {
        const float lower = (k == 0) ? lin(0) : 0.5f * (lin(k) + lin(k - 1));
        const float upper = (k == S - 1) ? lin(S - 1) : 0.5f * (lin(k + 1) + lin(k));
        return lower + (upper - lower) * u;
    }
    const float delta = (float)((1.0 - 0.0) / (double)(S - 1));
    return lin(k) + u * delta;
}

__global__ __launch_bounds__(256) void stratified_kernel(const float* __restrict__ u, float* __restrict__ sdist, float* __restrict__ tdist,
                                                        int64_t n, int S, int marcher, float t_near, float t_far) {
    const float step = (1.f - 0.f) / (float)(S - 1);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float s = strat_one(u[i], (int)(i % S), S, step, marcher);
        sdist[i] = s;
        if (tdist) tdist[i] = s2t(s, t_near, t_far);
    }
}

// The same, four consecutive samples of a ray per thread as 16-byte loads / stores (S % 4 == 0, 16-byte aligned pointers: the generator's shapes).
// Round 5: the scalar form moved 4 bytes per lane and instruction and spent a 64-bit modulo per sample -- 4.3 of the 6.3 TB/s a copy reaches.
__global__ __launch_bounds__(256) void stratified4_kernel(const float4* __restrict__ u, float4* __restrict__ sdist, float4* __restrict__ tdist,
                                                         int64_t n4, int S, int marcher, float t_near, float t_far) {
    const float step = (1.f - 0.f) / (float)(S - 1);
    const int S4 = S >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % S4) * 4;
        const float4 uu = u[i];
        const float4 s = make_float4(strat_one(uu.x, k, S, step, marcher), strat_one(uu.y, k + 1, S, step, marcher), strat_one(uu.z, k + 2, S, step, marcher),
                                     strat_one(uu.w, k + 3, S, step, marcher));
        sdist[i] = s;
        if (tdist) tdist[i] = make_float4(s2t(s.x, t_near, t_far), s2t(s.y, t_near, t_far), s2t(s.z, t_near, t_far), s2t(s.w, t_near, t_far));
    }
}

__global__ __launch_bounds__(256) void density_activation_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int relu, float bias) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = relu ? (x[i] > 0.f ? x[i] : 0.f) : softplus20f(x[i] + bias);
}

// generic marcher: colours [rays,S,C], densities [rays,S], depths [rays,S].  MS = MAXS, or MAXS_LONG for S > MAXS.
template <int MS>
__global__ __launch_bounds__(256) void ray_march_kernel(const float* __restrict__ colors, const float* __restrict__ dens,
                                                       const float* __restrict__ depths, float* __restrict__ rgb, float* __restrict__ depth_o,
                                                       float* __restrict__ weights, float* __restrict__ final_T, int64_t rays, int S, int C,
                                                       int marcher, int flags, float density_bias, float cut_thr) {
    __shared__ MarchScratchT<MS> scratch[RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6, l = lane_id();
    const int64_t r = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (r >= rays) return;
    MarchScratchT<MS>& sc = scratch[wv];
    for (int i = l; i < S; i += 64) { sc.z[i] = depths[r * S + i]; sc.sig[i] = dens[r * S + i]; }
    wave_sync();
    float fT, wagg;
    const int M = (marcher == 0) ? S : ((flags & 1) ? S : S - 1);
    if (MS > MAXS && S > MAXS) {
        if (marcher == 0) march_classical_lds<(MS > MAXS)>(sc.z, sc.sig, sc.w, S, flags, cut_thr, fT, wagg);
        else march_mip_lds<(MS > MAXS)>(sc.z, sc.sig, sc.w, S, flags, density_bias, cut_thr, fT, wagg);
    } else
    if (marcher == 0) march_classical_lds(sc.z, sc.sig, sc.w, S, flags, cut_thr, fT, wagg);
    else march_mip_lds(sc.z, sc.sig, sc.w, S, flags, density_bias, cut_thr, fT, wagg);
    if (weights) for (int i = l; i < M; i += 64) weights[r * M + i] = sc.w[i];
    // composite: sum_i w_i * c_i
    for (int c = 0; c <= C; c++) {          // c == C: depth
        float acc = 0.0f;
        for (int i = l; i < M; i += 64) {
            float v;
            if (c < C) {
                v = colors[(r * S + i) * C + c];
                if (marcher == 1 && i < S - 1) v = (v + colors[(r * S + i + 1) * C + c]) / 2.f;
            } else {
                v = sc.z[i];
                if (marcher == 1 && i < S - 1) v = (v + sc.z[i + 1]) / 2.f;
            }
            acc += sc.w[i] * v;
        }
        float out = wave_sum_f32(acc);
        if (marcher == 1 && c < C) {
            if (flags & 4) out = out + 1.0f - wagg;
            out = out * 2.0f - 1.0f;
        }
        if (l == 0) { if (c < C) rgb[r * C + c] = out; else depth_o[r] = out; }
    }
    if (l == 0) final_T[r] = fT;
}

template <int MS>
__global__ __launch_bounds__(256) void sample_importance_kernel(const float* __restrict__ z, const float* __restrict__ weights,
                                                               const float* __restrict__ u, float* __restrict__ samples, int32_t* __restrict__ inds,
                                                               int32_t* __restrict__ below, int32_t* __restrict__ above, float* __restrict__ cdf_o,
                                                               int64_t rays, int S, int Wn, int N, int mip) {
    __shared__ WaveScratchT<MS> scratch[RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6, l = lane_id();
    const int64_t r = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (r >= rays) return;
    WaveScratchT<MS>& sc = scratch[wv];
    for (int i = l; i < S; i += 64) sc.z[i] = z[r * S + i];
    for (int i = l; i < Wn; i += 64) sc.w[i] = weights[r * Wn + i];
    wave_sync();
    importance_lds(sc, S, Wn, [&](int j) { return u[r * N + j]; }, N, mip, [&](int j, float smp, int ind, int bl, int ab) {
        samples[r * N + j] = smp;
        if (inds) { inds[r * N + j] = ind; below[r * N + j] = bl; above[r * N + j] = ab; }
    });
    if (cdf_o) for (int i = l; i < Wn - 1; i += 64) cdf_o[r * (Wn - 1) + i] = sc.cdf[i];
}

// stable rank of every element of key[0..M) under (key, index) order -> rank[]; brute force from LDS broadcasts.
// NS = ceil(M / 64) value slots per lane actually in use (compile time, so no work is spent on empty slots).
template <int NS>
__device__ __forceinline__ void stable_ranks_n(const float* key, int M, int* rank) {
    const int l = lane_id();
    float k[NS];
#pragma unroll
    for (int c = 0; c < NS; c++) { const int i = l + 64 * c; k[c] = i < M ? key[i] : 0.f; rank[c] = 0; }
#pragma unroll 4
    for (int m = 0; m < M; m++) {
        const float km = key[m];                   // same address on every lane: LDS broadcast
#pragma unroll
        for (int c = 0; c < NS; c++) {
            const int i = l + 64 * c;
            rank[c] += (km < k[c] || (km == k[c] && m < i)) ? 1 : 0;
        }
    }
}
// The dispatcher over NS for a lane's NR rank slots: NR = MAXS / 64 (the short kernels: 1..4 slots in use), or 8 / 16 for the long lists
// (M <= MAXS_LONG).  O(M^2 / 64) per lane -- the fallback for lists that are not ascending, and unify_samples' rank (not on the
// renderer's forward).
template <int NR>
__device__ __forceinline__ void stable_ranks(const float* key, int M, int (&rank)[NR]) {
    static_assert(NR == MAXS / 64 || NR == MAXS_PASS / 64 || NR == MAXS_LONG / 64, "stable_ranks: 4, 8 or 16 slots");
#pragma unroll
    for (int c = 0; c < NR; c++) rank[c] = 0;
    if constexpr (NR == MAXS / 64) {
        if (M <= 64) stable_ranks_n<1>(key, M, rank);
        else if (M <= 128) stable_ranks_n<2>(key, M, rank);
        else if (M <= 192) stable_ranks_n<3>(key, M, rank);
        else stable_ranks_n<4>(key, M, rank);
    } else {
        if (M <= MAXS_PASS) stable_ranks_n<MAXS_PASS / 64>(key, M, rank);
        else stable_ranks_n<NR>(key, M, rank);
    }
}

// Bitonic sort of 64 * NS (key, index) pairs, NS per lane (element e = 64 c + lane), ascending by (key, index), for any power-of-two NS.
// Stages with j >= 64 are compare-exchanges between two slots of the same lane, the others one pair of cross-lane permutes (ds_bpermute,
// LDS pipe) + ~5 VALU per slot.  Indices are unique, so the order is total and the result is the stable sort.
//   NS = 1: 21 stages -- a third of the vector work of the brute-force rank above for 64 keys;
//   NS = 2: 28 stages, for 64 < N <= 128 fine samples (BASELINE configs[4]: 96) instead of N broadcasts x 2 slots;
//   NS = 4, 8: 128 < N <= 512 fine samples (long rays): 45 stages at NS = 8, against 512 broadcasts x 8 slots of the brute-force rank.
template <int NS, int CAP>
__device__ __forceinline__ void wave_bitonic_sort_n(float (&key)[CAP], int (&idx)[CAP]) {
    static_assert(NS <= CAP && (NS & (NS - 1)) == 0, "wave_bitonic_sort_n: NS a power of two within the arrays");
    const int l = lane_id();
#pragma unroll
    for (int k = 2; k <= 64 * NS; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
                const int js = j >> 6;
#pragma unroll
                for (int c = 0; c < NS; c++) {
                    if (c & js) continue;
                    const int c2 = c | js;
                    const bool asc = ((64 * c) & k) == 0;           // bits of e at or above 64 are the slot's; c and c2 agree on bit k
                    const bool less2 = key[c2] < key[c] || (key[c2] == key[c] && idx[c2] < idx[c]);
                    if (less2 == asc) { const float tk = key[c]; key[c] = key[c2]; key[c2] = tk; const int ti = idx[c]; idx[c] = idx[c2]; idx[c2] = ti; }
                }
            } else {
#pragma unroll
                for (int c = 0; c < NS; c++) {
                    const float pk = __shfl_xor(key[c], j, 64);
                    const int pi = __shfl_xor(idx[c], j, 64);
                    const bool asc = ((64 * c + l) & k) == 0;
                    const bool keep_min = ((l & j) == 0) == asc;
                    const bool partner_less = pk < key[c] || (pk == key[c] && pi < idx[c]);
                    if (partner_less == keep_min) { key[c] = pk; idx[c] = pi; }
                }
            }
        }
    }
}

// fused: coarse march (s-space) -> importance sampling -> fine depths (t-space), WRITTEN IN ASCENDING DEPTH ORDER.
// The reference leaves the fine samples in draw order and sorts coarse+fine together later (unify_samples); sorting the
// fine list here (stable, by (t, draw index)) changes nothing in that final order but makes the j-th fine sample of
// neighbouring rays neighbours in space (texture locality of the second field pass) and turns the later merge into a
// merge of two sorted lists.  fine_perm[pos] = draw index of the sample stored at pos.
template <int MS>
__global__ __launch_bounds__(256) void importance_from_coarse_kernel(const float* __restrict__ rgbs, const float* __restrict__ sdist,
                                                                    const float* __restrict__ u_fine, float* __restrict__ tfine,
                                                                    float* __restrict__ sfine, int32_t* __restrict__ inds,
                                                                    int32_t* __restrict__ fine_perm, int64_t rays, int S, int N,
                                                                    int marcher, int flags, float density_bias, float cut_thr, float t_near, float t_far) {
    __shared__ WaveScratchT<MS> scratch[RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6, l = lane_id();
    const int64_t r = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (r >= rays) return;
    WaveScratchT<MS>& sc = scratch[wv];
    for (int i = l; i < S; i += 64) { sc.z[i] = sdist[r * S + i]; sc.sig[i] = rgbs[(r * S + i) * 4 + 3]; }
    // the draws are not needed before the cdf exists: their loads go out now and land during the march
    float upre[MS / 64];
    if constexpr (MS > MAXS) {      // long rays: the draws wait in LDS (sc.col[1]) -- a register array behind the non-inlined importance_lds would live in scratch
        for (int i = l; i < N; i += 64) sc.col[1][i] = u_fine[r * N + i];
    } else {
#pragma unroll
    for (int c = 0; c < MS / 64; c++) upre[c] = (l + 64 * c < N) ? u_fine[r * N + l + 64 * c] : 0.f;
    }
    wave_sync();
    float fT, wagg;
    int Wn = S;
    if (MS > MAXS && S > MAXS) {    // the coarse list marched as tdgp_ray_march marches a list of that length
        if (marcher == 0) march_classical_lds<(MS > MAXS)>(sc.z, sc.sig, sc.w, S, flags, cut_thr, fT, wagg);
        else { march_mip_lds<(MS > MAXS)>(sc.z, sc.sig, sc.w, S, flags, density_bias, cut_thr, fT, wagg); Wn = (flags & 1) ? S : S - 1; }
    } else
    if (marcher == 0) march_classical_lds(sc.z, sc.sig, sc.w, S, flags, cut_thr, fT, wagg);
    else { march_mip_lds(sc.z, sc.sig, sc.w, S, flags, density_bias, cut_thr, fT, wagg); Wn = (flags & 1) ? S : S - 1; }
    float* tkey = sc.col[0];
    if constexpr (MS > MAXS)
        // inlined here (the short forms inline it on their own): a call would pass the lambdas' captures through private scratch
        [[clang::always_inline]] importance_lds(sc, S, Wn, [&](int j) { return sc.col[1][j]; }, N, marcher, [&](int j, float smp, int ind, int, int) {
            tkey[j] = s2t(smp, t_near, t_far);
            if (sfine) sfine[r * N + j] = smp;
            if (inds) inds[r * N + j] = ind;
        });
    else
    importance_lds(sc, S, Wn, [&](int j) { float v = upre[0];
#pragma unroll
                                          for (int c = 1; c < MS / 64; c++) v = (j >> 6) == c ? upre[c] : v;
                                          return v; }, N, marcher, [&](int j, float smp, int ind, int, int) {
        tkey[j] = s2t(smp, t_near, t_far);
        if (sfine) sfine[r * N + j] = smp;
        if (inds) inds[r * N + j] = ind;
    });
    wave_sync();
    if (N <= 64) {                  // one sample per lane: sort across the lanes, store coalesced
        float key = l < N ? tkey[l] : INFINITY;
        // Distinct keys (all but measure-zero rays): the sorted slot of a key is the number of smaller keys -- 16 broadcast LDS reads
        // and 128 compare / add-carry instructions with no dependent chain, where the network below is 21 stages of two dependent
        // cross-lane permutes each (it was 30 % of this kernel's time).  Equal keys collide on a slot, which the read-back sees: those
        // rays take the network, whose (key, draw index) order is the stable sort.
        {
            if (l >= N) tkey[l] = INFINITY;
            wave_sync();
            int cnt = 0;
#pragma unroll
            for (int jj = 0; jj < 16; jj++) {
                const float4 k4 = *(const float4*)&tkey[4 * jj];
                cnt += (k4.x < key ? 1 : 0) + (k4.y < key ? 1 : 0) + (k4.z < key ? 1 : 0) + (k4.w < key ? 1 : 0);
            }
            int* slot = (int*)sc.bins;                      // free since importance_lds returned
            if (l < N) slot[cnt] = l;
            wave_sync();
            const bool mine = l >= N || slot[cnt] == l;
            if (__all(mine)) {
                if (l < N) {
                    const int src = slot[l];
                    tfine[r * N + l] = tkey[src];
                    if (fine_perm) fine_perm[r * N + l] = src;
                }
                return;
            }
        }
        float k1[1] = {key};
        int idx[1] = {l};
        wave_bitonic_sort_n<1>(k1, idx);
        if (l < N) {
            tfine[r * N + l] = k1[0];
            if (fine_perm) fine_perm[r * N + l] = idx[0];
        }
        return;
    }
    if (N <= 128) {                 // two samples per lane
        float key[2] = {tkey[l], l + 64 < N ? tkey[l + 64] : INFINITY};
        {                           // distinct keys: slot = number of smaller keys, as above (MS >= 128 entries behind tkey)
            if (l + 64 >= N) tkey[l + 64] = INFINITY;
            wave_sync();
            int cnt[2] = {0, 0};
#pragma unroll 8
            for (int jj = 0; jj < 32; jj++) {
                const float4 k4 = *(const float4*)&tkey[4 * jj];
#pragma unroll
                for (int c = 0; c < 2; c++)
                    cnt[c] += (k4.x < key[c] ? 1 : 0) + (k4.y < key[c] ? 1 : 0) + (k4.z < key[c] ? 1 : 0) + (k4.w < key[c] ? 1 : 0);
            }
            int* slot = (int*)sc.bins;
            slot[cnt[0]] = l;
            if (l + 64 < N) slot[cnt[1]] = l + 64;
            wave_sync();
            const bool mine = slot[cnt[0]] == l && (l + 64 >= N || slot[cnt[1]] == l + 64);
            if (__all(mine)) {
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const int pos = l + 64 * c;
                    if (pos < N) {
                        const int src = slot[pos];
                        tfine[r * N + pos] = tkey[src];
                        if (fine_perm) fine_perm[r * N + pos] = src;
                    }
                }
                return;
            }
        }
        int idx[2] = {l, l + 64};
        wave_bitonic_sort_n<2>(key, idx);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int pos = l + 64 * c;
            if (pos < N) {
                tfine[r * N + pos] = key[c];
                if (fine_perm) fine_perm[r * N + pos] = idx[c];
            }
        }
        return;
    }
    if constexpr (MS > MAXS) {      // long rays, 128 < N <= MS: the bitonic network over 256 or 512 (t, draw index) pairs, NS per lane
        constexpr int NSL = MS / 64;
        float key[NSL];
        int idx[NSL];
#pragma unroll
        for (int c = 0; c < NSL; c++) { const int e = l + 64 * c; key[c] = e < N ? tkey[e] : INFINITY; idx[c] = e; }    // padding sorts last (index >= N)
        if (N <= 256) wave_bitonic_sort_n<4>(key, idx);
        else wave_bitonic_sort_n<NSL>(key, idx);
#pragma unroll
        for (int c = 0; c < NSL; c++) {
            const int pos = l + 64 * c;
            if (pos < N) {
                tfine[r * N + pos] = key[c];
                if (fine_perm) fine_perm[r * N + pos] = idx[c];
            }
        }
        return;
    } else {
    int rank[MAXS / 64];
    stable_ranks(tkey, N, rank);
#pragma unroll
    for (int c = 0; c < MAXS / 64; c++) {
        const int j = l + 64 * c;
        if (j < N) {
            tfine[r * N + rank[c]] = tkey[j];
            if (fine_perm) fine_perm[r * N + rank[c]] = j;
        }
    }
    }
}

// MS = MAXS, or MAXS_LONG for S1 + S2 > MAXS (brute-force stable rank over 8 / 16 slots per lane: the staged path, not the renderer's forward).
template <int MS>
__global__ __launch_bounds__(256) void unify_kernel(const float* __restrict__ d1, const float* __restrict__ c1, const float* __restrict__ s1, int S1,
                                                   const float* __restrict__ d2, const float* __restrict__ c2, const float* __restrict__ s2, int S2,
                                                   float* __restrict__ d, float* __restrict__ c, float* __restrict__ s, int32_t* __restrict__ perm,
                                                   int64_t rays, int C) {
    __shared__ UnifyScratchT<MS> scratch[RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6, l = lane_id();
    const int64_t r = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (r >= rays) return;
    UnifyScratchT<MS>& sc = scratch[wv];
    const int M = S1 + S2;
    for (int i = l; i < M; i += 64) sc.z[i] = i < S1 ? d1[r * S1 + i] : d2[r * S2 + (i - S1)];
    wave_sync();
    int rank[MS / 64];
    stable_ranks(sc.z, M, rank);
#pragma unroll
    for (int cc = 0; cc < MS / 64; cc++) {
        const int i = l + 64 * cc;
        if (i >= M) continue;
        const int pos = rank[cc];
        d[r * M + pos] = sc.z[i];
        s[r * M + pos] = i < S1 ? s1[r * S1 + i] : s2[r * S2 + (i - S1)];
        for (int k = 0; k < C; k++) c[(r * M + pos) * C + k] = i < S1 ? c1[(r * S1 + i) * C + k] : c2[(r * S2 + (i - S1)) * C + k];
        if (perm) perm[r * M + pos] = i;
    }
}

// fused: merge coarse + fine by depth (stable), march in t-space, composite.
template <int MS>
__global__ __launch_bounds__(256) void merge_composite_kernel(const float* __restrict__ rgbs1, const float* __restrict__ t1, int S1,
                                                             const float* __restrict__ rgbs2, const float* __restrict__ t2, int S2,
                                                             float* __restrict__ rgb, float* __restrict__ depth_o, float* __restrict__ wsum_o,
                                                             float* __restrict__ final_T, int32_t* __restrict__ perm, const int32_t* __restrict__ perm2, int64_t rays,
                                                             int marcher, int flags, float density_bias, float cut_thr) {
    __shared__ WaveScratchT<MS> scratch[RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6, l = lane_id();
    const int64_t r = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (r >= rays) return;
    WaveScratchT<MS>& sc = scratch[wv];
    const int M = S1 + S2;
    // keys -> sc.cdf (scratch), ranks, scatter into sorted sc.z / sc.sig / sc.col.  The colours do not depend on the ranks: their
    // loads go out with the keys' and land while the ranks are searched.
    float4 cval[MS / 64];
#pragma unroll
    for (int cc = 0; cc < MS / 64; cc++) {
        const int i = l + 64 * cc;
        if (i < M) {
            sc.cdf[i] = i < S1 ? t1[r * S1 + i] : t2[r * S2 + (i - S1)];
            cval[cc] = i < S1 ? ((const float4*)rgbs1)[r * S1 + i] : ((const float4*)rgbs2)[r * S2 + (i - S1)];
        }
    }
    wave_sync();
    // both lists already ascending (stratified coarse samples; fine samples sorted by importance_from_coarse)?  Then the
    // stable merge position is the element's own index plus a binary search in the OTHER list; otherwise (arbitrary caller
    // data, or the ~1e-10-probability ulp inversion of s -> t) fall back to the brute-force stable rank.
    bool bad = false;
    for (int i = l; i < M; i += 64)
        if (i + 1 < M && i + 1 != S1 && sc.cdf[i + 1] < sc.cdf[i]) bad = true;
    constexpr int RK = (MS > MAXS ? MS : MAXS) / 64;
    int rank[RK];
    if (__any(bad)) {
        stable_ranks(sc.cdf, M, rank);
    } else {
        // Ranks of a stable merge of two ascending lists (coarse wins ties).
        //   fine element j:    its own index + #coarse <= f_j  =: j + cnt_j     -- a binary search in the coarse list;
        //   coarse element i:  its own index + #fine < c_i.  No second search: c_i <= f_j  <=>  cnt_j >= i + 1, so #fine < c_i = #{j : cnt_j <= i}, and
        //                      cnt_j does not decrease with j, so that count is (the largest j with cnt_j <= i) + 1 = a PREFIX MAXIMUM over
        //                      last[c] = max{j + 1 : cnt_j = c} -- one LDS max-scatter by the fine elements and one wave scan.
        // (Round 5.  Before, every element searched the other list: 7 lock-step rounds of ~14 vector instructions on both slots of a lane, a third of
        //  this kernel's instructions; now the slots that hold only coarse elements skip the search.)  The searches of a lane's slots still advance
        //  together, a fixed number of branch-free steps: one chain of dependent LDS reads instead of one per slot.
        constexpr int NSL = MS / 64;
        float v[NSL];
        int lo[NSL], hi[NSL];
        bool fine[NSL];
        int* const last = (int*)sc.bins;                 // [S1 + 1] (S1 + 1 <= MS: the list lengths are checked on the host)
        for (int c = l; c <= S1 && c < MS; c += 64) last[c] = 0;        // (c == MS only when there is no fine list at all)
#pragma unroll
        for (int cc = 0; cc < NSL; cc++) {
            const int i = l + 64 * cc;
            v[cc] = i < M ? sc.cdf[i] : 0.f;
            fine[cc] = i >= S1 && i < M;
            lo[cc] = 0;
            hi[cc] = fine[cc] ? S1 : 0;                  // coarse elements (and slots past the end) never open a search
        }
        const int steps = 32 - __clz(S1);
        for (int it = 0; it < steps; it++) {
#pragma unroll
            for (int cc = 0; cc < NSL; cc++) {           // #coarse <= v (coarse wins ties)
                if (64 * cc + 64 <= S1) continue;        // a slot of coarse elements only (wave-uniform)
                const bool open = lo[cc] < hi[cc];
                const int mid = (lo[cc] + hi[cc]) >> 1;
                const float o = sc.cdf[open ? mid : 0];
                const bool right = o <= v[cc];
                lo[cc] = (open && right) ? mid + 1 : lo[cc];
                hi[cc] = (open && !right) ? mid : hi[cc];
            }
        }
        wave_sync();                                     // last[] is zeroed before the scatter below
#pragma unroll
        for (int cc = 0; cc < NSL; cc++) {
            const int i = l + 64 * cc;
            if (fine[cc]) atomicMax(&last[lo[cc]], i - S1 + 1);
        }
        wave_sync();
#pragma unroll
        for (int cc = 0; cc < RK; cc++) rank[cc] = 0;
        int carry = 0;
#pragma unroll
        for (int cc = 0; cc < NSL; cc++) {
            const int i = l + 64 * cc;
            if (64 * cc < S1) {                          // this slot holds coarse elements: F(i) = max over c <= i of last[c]
                const int incl = max(wave_scan_max_i32((i <= S1 && i < MS) ? last[i] : 0), carry);
                carry = wave_last_i32(incl);
                rank[cc] = fine[cc] ? (i - S1) + lo[cc] : i + incl;
            } else {
                rank[cc] = (i - S1) + lo[cc];
            }
        }
    }
#pragma unroll
    for (int cc = 0; cc < MS / 64; cc++) {
        const int i = l + 64 * cc;
        if (i >= M) continue;
        const int pos = rank[cc];
        const float4 v = cval[cc];
        sc.z[pos] = sc.cdf[i];
        sc.col[0][pos] = v.x; sc.col[1][pos] = v.y; sc.col[2][pos] = v.z; sc.sig[pos] = v.w;
        if (perm) perm[r * M + pos] = i < S1 ? i : S1 + (perm2 ? perm2[r * S2 + (i - S1)] : i - S1);
    }
    wave_sync();
    float fT, wagg;
    const int Mm = (marcher == 0) ? M : ((flags & 1) ? M : M - 1);
    if (MS > MAXS && M > MAXS) {
        if (marcher == 0) march_classical_lds<(MS > MAXS)>(sc.z, sc.sig, sc.w, M, flags, cut_thr, fT, wagg);
        else march_mip_lds<(MS > MAXS)>(sc.z, sc.sig, sc.w, M, flags, density_bias, cut_thr, fT, wagg);
    } else
    if (marcher == 0) march_classical_lds(sc.z, sc.sig, sc.w, M, flags, cut_thr, fT, wagg);
    else march_mip_lds(sc.z, sc.sig, sc.w, M, flags, density_bias, cut_thr, fT, wagg);
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, wacc = 0.f;
    for (int i = l; i < Mm; i += 64) {
        const float wi = sc.w[i];
        wacc += wi;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float v = c < 3 ? sc.col[c][i] : sc.z[i];
            if (marcher == 1 && i < M - 1) v = (v + (c < 3 ? sc.col[c][i + 1] : sc.z[i + 1])) / 2.f;
            acc[c] += wi * v;
        }
    }
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = wave_sum_f32(acc[c]);
    const float wtot = wave_sum_f32(wacc);            // weights.sum(2): final weights incl. last_back
    if (marcher == 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (flags & 4) out[c] = out[c] + 1.0f - wagg;
            out[c] = out[c] * 2.0f - 1.0f;
        }
    }
    if (l == 0) {
        rgb[r * 3 + 0] = out[0]; rgb[r * 3 + 1] = out[1]; rgb[r * 3 + 2] = out[2];
        depth_o[r] = out[3];
        if (wsum_o) wsum_o[r] = wtot;
        if (final_T) final_T[r] = fT;
    }
}

// ------------------------------------------------------------------------------------------------
// 64 + 64 pair forms: a wave owns rays 2w and 2w + 1, 8 rays per 256-thread block.  The kernels above sit at the
// hardware's 8 waves per SIMD with half the register file empty, and what bounds them is the length of one ray's chain of dependent
// LDS / cross-lane steps; here every phase is a function of ONE ray's state, fence-free inside, called for ray A and then for ray B
// with the wave fence after both, so the scheduler has two independent chains to interleave and the global loads of both rays are
// out before anything waits.  The importance phases and the marches are the one-ray kernels' stage functions / statements at S = N = 64 and
// M = 128; the file header names the specialised copies that remain and why.  Per ray the same operations in the same order: the same bits.
// The slow paths (the
// bitonic network after a key collision, the brute-force rank of a list that is not ascending) are wave-uniform branches per ray.
// An odd last ray: its wave computes it twice (B = A) and B stores nothing.
// ------------------------------------------------------------------------------------------------
constexpr int PAIR_RAYS_PER_BLOCK = 8;

// Importance form.  Scratch: z, sig, w, cdf, bins and the key column at 64 entries = 1552 B per ray, 12.4 KB per block; 8 blocks per CU
// (99 KB of LDS) = 8 waves = 16 rays per SIMD, twice the one-ray form's.
struct alignas(16) ImpPairScratch { float z[64]; float sig[64]; float w[64 + 4]; float cdf[64]; float bins[64]; float key[64]; };

struct ImpRay {
    ImpPairScratch* sc;
    int64_t r;          // the ray (B of an odd last pair: A's ray again)
    bool live;          // this ray stores its results
    float zl, sg, u;    // lane l's coarse depth, density and draw
    float nv[1];        // mip: the smoothed weight between its read and its write
    float key[1];       // lane l's fine sample in t-space (draw order), then the sample sorted to position l
    int cnt, idx[1];    // the number of smaller keys; the draw index sorted to position l (key, idx: the one slot of wave_bitonic_sort_n<1>)
};

__device__ __forceinline__ void imp_load(ImpRay& R, const float* __restrict__ rgbs, const float* __restrict__ sdist, const float* __restrict__ u_fine) {
    const int l = lane_id();
    R.zl = sdist[R.r * 64 + l]; R.sg = rgbs[(R.r * 64 + l) * 4 + 3]; R.u = u_fine[R.r * 64 + l];
}
__device__ __forceinline__ void imp_park(ImpRay& R) { const int l = lane_id(); R.sc->z[l] = R.zl; R.sc->sig[l] = R.sg; }
// coarse march of 64 samples: the single pass of march_classical_lds' / march_mip_lds' loop (carry = 1); returns sum w
__device__ __forceinline__ float imp_march(ImpRay& R, int marcher, int flags, float density_bias, float cut_thr) {
    const int l = lane_id();
    const int M = (marcher == 0 || (flags & 1)) ? 64 : 63;
    float alpha, fac;
    const float *z = R.sc->z, *sig = R.sc->sig;
    if (marcher == 0) { TDGP_CLASSICAL_ALPHA(false, z, sig, l, 64, flags, cut_thr, alpha, fac); }
    else { TDGP_MIP_ALPHA(false, z, sig, l, 64, M, density_bias, cut_thr, alpha, fac); }
    const double carry = 1.0;
    TDGP_MARCH_PASS(wi, incl64, alpha, fac, carry)
    float wsum = 0.0f;
    if (l < M) { R.sc->w[l] = wi; wsum += wi; }
    return wave_sum_f32(wsum);
}
__device__ __forceinline__ void imp_last_back(ImpRay& R, float wagg) { if (lane_id() == 0) R.sc->w[63] += (1.0f - wagg); }
// cdf_search of lane l's draw, the sample, its t-space key into the key column
__device__ __forceinline__ void imp_search(ImpRay& R, int Wn, float t_near, float t_far, float* __restrict__ sfine, int32_t* __restrict__ inds) {
    const int l = lane_id();
    ImpPairScratch& sc = *R.sc;
    const int ns = Wn - 2, nc = ns + 1;
    const float uu = R.u;
    const int ind = cdf_search(sc.cdf, nc, uu);
    int below, above;
    const float smp = cdf_sample(sc.cdf, sc.bins, 63, ns, ind, uu, below, above);
    R.key[0] = s2t(smp, t_near, t_far);
    sc.key[l] = R.key[0];
    if (R.live) {
        if (sfine) sfine[R.r * 64 + l] = smp;
        if (inds) inds[R.r * 64 + l] = ind;
    }
}
// the sorted slot of a key is the number of smaller keys; equal keys collide on a slot
__device__ __forceinline__ void imp_count(ImpRay& R) {
    const int l = lane_id();
    int cnt = 0;
#pragma unroll
    for (int jj = 0; jj < 16; jj++) {
        const float4 k4 = *(const float4*)&R.sc->key[4 * jj];
        cnt += (k4.x < R.key[0] ? 1 : 0) + (k4.y < R.key[0] ? 1 : 0) + (k4.z < R.key[0] ? 1 : 0) + (k4.w < R.key[0] ? 1 : 0);
    }
    R.cnt = cnt;
    ((int*)R.sc->bins)[cnt] = l;            // bins is free since imp_search
}
// read back: without a collision position l takes the key whose slot it is; with one the ray keeps (key, l) for the network.  Returns "no collision".
__device__ __forceinline__ bool imp_gather(ImpRay& R) {
    const int l = lane_id();
    const int* slot = (const int*)R.sc->bins;
    const bool ok = __all(slot[R.cnt] == l);
    const int src = ok ? slot[l] : l;
    R.key[0] = R.sc->key[src];
    R.idx[0] = src;
    return ok;
}
__device__ __forceinline__ void imp_store(const ImpRay& R, float* __restrict__ tfine, int32_t* __restrict__ fine_perm) {
    const int l = lane_id();
    if (R.live) {
        tfine[R.r * 64 + l] = R.key[0];
        if (fine_perm) fine_perm[R.r * 64 + l] = R.idx[0];
    }
}

// importance_from_coarse_kernel<128> at S = N = 64, two rays per wave.  gfx950: see DESIGN.md 5.5 for the register count (at most 64, no scratch).
__global__ __launch_bounds__(256, 8) void importance_from_coarse_pair_kernel(const float* __restrict__ rgbs, const float* __restrict__ sdist,
                                                                            const float* __restrict__ u_fine, float* __restrict__ tfine,
                                                                            float* __restrict__ sfine, int32_t* __restrict__ inds,
                                                                            int32_t* __restrict__ fine_perm, int64_t rays, int marcher, int flags,
                                                                            float density_bias, float cut_thr, float t_near, float t_far) {
    __shared__ ImpPairScratch scratch[PAIR_RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6;
    const int64_t r0 = ((int64_t)blockIdx.x * (PAIR_RAYS_PER_BLOCK / 2) + wv) * 2;
    if (r0 >= rays) return;
    ImpRay A, B;
    A.sc = &scratch[2 * wv]; A.r = r0; A.live = true;
    B.sc = &scratch[2 * wv + 1]; B.live = r0 + 1 < rays; B.r = B.live ? r0 + 1 : r0;
    imp_load(A, rgbs, sdist, u_fine); imp_load(B, rgbs, sdist, u_fine);
    imp_park(A); imp_park(B);
    wave_sync();
    const float waA = imp_march(A, marcher, flags, density_bias, cut_thr), waB = imp_march(B, marcher, flags, density_bias, cut_thr);
    wave_sync();
    int Wn = 64;
    if (marcher == 0) {
        if (flags & 2) { imp_last_back(A, waA); imp_last_back(B, waB); }
        wave_sync();
        offset_weights(A.sc->w, Wn); offset_weights(B.sc->w, Wn);
    } else {
        Wn = (flags & 1) ? 64 : 63;
        smooth_read<1>(A.sc->w, Wn, A.nv); smooth_read<1>(B.sc->w, Wn, B.nv);
        wave_sync();
        smooth_write<1>(A.sc->w, Wn, A.nv); smooth_write<1>(B.sc->w, Wn, B.nv);
    }
    wave_sync();
    pdf_cdf<true>(A.sc->z, A.sc->w, A.sc->bins, A.sc->cdf, 64, Wn); pdf_cdf<true>(B.sc->z, B.sc->w, B.sc->bins, B.sc->cdf, 64, Wn);
    wave_sync();
    imp_search(A, Wn, t_near, t_far, sfine, inds); imp_search(B, Wn, t_near, t_far, sfine, inds);
    wave_sync();
    imp_count(A); imp_count(B);
    wave_sync();
    const bool okA = imp_gather(A), okB = imp_gather(B);
    if (!okA) wave_bitonic_sort_n<1>(A.key, A.idx);      // per ray: the other one is done
    if (!okB) wave_bitonic_sort_n<1>(B.key, B.idx);
    imp_store(A, tfine, fine_perm); imp_store(B, tfine, fine_perm);
}

// Merge form.  Scratch: six arrays of 128 entries = 3072 B per ray (the one-ray form's eight: the unsorted keys are dead once the scatter has run
// and the weights take their place; last[] is dead before the scatter writes z and lives there), 24.6 KB per block; 6 blocks per CU
// (147 KB of LDS) = 6 waves = 12 rays per SIMD against the one-ray form's 8.
struct alignas(16) MergePairScratch {
    float key[128];     // unsorted depths (coarse 0..63, fine 64..127); from the march on: the weights
    float z[128];       // last[0..64] of the rank computation, then the sorted depths
    float sig[128];
    float col[3][128];
};

struct MergeRay {
    MergePairScratch* sc;
    int64_t r;
    bool live;
    float k[2];         // lane l's coarse and fine depth
    float4 c[2];        // and their colours + density
    int p2;             // draw index of fine element l
    int lo;             // fine element l: #coarse <= its depth
    int rank[2];
    bool bad;
};

__device__ __forceinline__ void mrg_load(MergeRay& R, const float* __restrict__ rgbs1, const float* __restrict__ t1, const float* __restrict__ rgbs2,
                                         const float* __restrict__ t2, const int32_t* __restrict__ perm2, bool want_perm) {
    const int l = lane_id();
    R.k[0] = t1[R.r * 64 + l]; R.k[1] = t2[R.r * 64 + l];
    R.c[0] = ((const float4*)rgbs1)[R.r * 64 + l]; R.c[1] = ((const float4*)rgbs2)[R.r * 64 + l];
    R.p2 = (want_perm && perm2) ? perm2[R.r * 64 + l] : l;
}
__device__ __forceinline__ void mrg_park(MergeRay& R) { const int l = lane_id(); R.sc->key[l] = R.k[0]; R.sc->key[64 + l] = R.k[1]; }
// ascending check, last[] zeroed, the fine elements' binary search in the coarse list (7 lock-step halvings of [0, 64))
__device__ __forceinline__ void mrg_search(MergeRay& R) {
    const int l = lane_id();
    const float* key = R.sc->key;
    R.bad = l < 63 && (key[l + 1] < key[l] || key[64 + l + 1] < key[64 + l]);
    int* const last = (int*)R.sc->z;
    last[l] = 0;
    if (l == 0) last[64] = 0;
    const float v = R.k[1];
    int lo = 0, hi = 64;
#pragma unroll
    for (int it = 0; it < 7; it++) {
        const bool open = lo < hi;
        const int mid = (lo + hi) >> 1;
        const bool right = key[open ? mid : 0] <= v;
        lo = (open && right) ? mid + 1 : lo;
        hi = (open && !right) ? mid : hi;
    }
    R.lo = lo;
}
__device__ __forceinline__ void mrg_scatter_last(MergeRay& R) { atomicMax(&((int*)R.sc->z)[R.lo], lane_id() + 1); }
// coarse ranks = own index + prefix maximum of last[]; fine ranks = own index + lo.  Returns "not ascending" (the ray needs the brute-force rank).
__device__ __forceinline__ bool mrg_ranks(MergeRay& R) {
    const int l = lane_id();
    const int incl = max(wave_scan_max_i32(((const int*)R.sc->z)[l]), 0);
    R.rank[0] = l + incl;
    R.rank[1] = l + R.lo;
    return __any(R.bad);
}
__device__ __forceinline__ void mrg_scatter(MergeRay& R, int32_t* __restrict__ perm) {
    const int l = lane_id();
    MergePairScratch& sc = *R.sc;
#pragma unroll
    for (int cc = 0; cc < 2; cc++) {
        const int pos = R.rank[cc];
        const float4 v = R.c[cc];
        sc.z[pos] = R.k[cc];
        sc.col[0][pos] = v.x; sc.col[1][pos] = v.y; sc.col[2][pos] = v.z; sc.sig[pos] = v.w;
        if (perm && R.live) perm[R.r * 128 + pos] = cc == 0 ? l : 64 + R.p2;
    }
}
// march of the merged 128 samples: march_classical_lds' two side-by-side chunks / the two passes of march_mip_lds' loop
__device__ __forceinline__ void mrg_march(MergeRay& R, int marcher, int flags, float density_bias, float cut_thr, float& final_T, float& wagg) {
    const int l = lane_id();
    MergePairScratch& sc = *R.sc;
    float* w = sc.key;
    double carry = 1.0;
    float wsum = 0.0f;
    if (marcher == 0) {
        float alpha[2], fac[2];
#pragma unroll
        for (int c = 0; c < 2; c++) { const int i = 64 * c + l; TDGP_CLASSICAL_ALPHA(false, sc.z, sc.sig, i, 128, flags, cut_thr, alpha[c], fac[c]); }
        TDGP_MARCH_PASS2(wi0, wi1, i1, alpha, fac)
        w[l] = wi0; wsum += wi0;
        w[64 + l] = wi1; wsum += wi1;
        carry = wave_last_f64(i1);
    } else {
        const int M = (flags & 1) ? 128 : 127;
#pragma unroll
        for (int base = 0; base < 128; base += 64) {
            const int i = base + l;
            float alpha, fac;
            TDGP_MIP_ALPHA(false, sc.z, sc.sig, i, 128, M, density_bias, cut_thr, alpha, fac);
            TDGP_MARCH_PASS(wi, incl64, alpha, fac, carry)
            if (i < M) { w[i] = wi; wsum += wi; }
            carry = wave_last_f64(incl64);
        }
    }
    wagg = wave_sum_f32(wsum);
    final_T = (float)carry;
}
__device__ __forceinline__ void mrg_last_back(MergeRay& R, float wagg) { if (lane_id() == 0) R.sc->key[127] += (1.0f - wagg); }
__device__ __forceinline__ void mrg_composite(MergeRay& R, int marcher, int flags, float wagg, float fT, float* __restrict__ rgb, float* __restrict__ depth_o,
                                              float* __restrict__ wsum_o, float* __restrict__ final_T) {
    const int l = lane_id();
    const MergePairScratch& sc = *R.sc;
    const float* w = sc.key;
    const int Mm = (marcher == 0 || (flags & 1)) ? 128 : 127;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, wacc = 0.f;
#pragma unroll
    for (int i = l; i < 128; i += 64) {
        if (i < Mm) {
            const float wi = w[i];
            wacc += wi;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                float v = c < 3 ? sc.col[c][i] : sc.z[i];
                if (marcher == 1 && i < 127) v = (v + (c < 3 ? sc.col[c][i + 1] : sc.z[i + 1])) / 2.f;
                acc[c] += wi * v;
            }
        }
    }
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = wave_sum_f32(acc[c]);
    const float wtot = wave_sum_f32(wacc);
    if (marcher == 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (flags & 4) out[c] = out[c] + 1.0f - wagg;
            out[c] = out[c] * 2.0f - 1.0f;
        }
    }
    if (l == 0 && R.live) {
        rgb[R.r * 3 + 0] = out[0]; rgb[R.r * 3 + 1] = out[1]; rgb[R.r * 3 + 2] = out[2];
        depth_o[R.r] = out[3];
        if (wsum_o) wsum_o[R.r] = wtot;
        if (final_T) final_T[R.r] = fT;
    }
}

// merge_composite_kernel<128> at S1 = S2 = 64, two rays per wave.  gfx950: see DESIGN.md 5.5 for the register count (at most 64, no scratch).
__global__ __launch_bounds__(256, 8) void merge_composite_pair_kernel(const float* __restrict__ rgbs1, const float* __restrict__ t1,
                                                                     const float* __restrict__ rgbs2, const float* __restrict__ t2,
                                                                     float* __restrict__ rgb, float* __restrict__ depth_o, float* __restrict__ wsum_o,
                                                                     float* __restrict__ final_T, int32_t* __restrict__ perm, const int32_t* __restrict__ perm2,
                                                                     int64_t rays, int marcher, int flags, float density_bias, float cut_thr) {
    __shared__ MergePairScratch scratch[PAIR_RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6;
    const int64_t r0 = ((int64_t)blockIdx.x * (PAIR_RAYS_PER_BLOCK / 2) + wv) * 2;
    if (r0 >= rays) return;
    MergeRay A, B;
    A.sc = &scratch[2 * wv]; A.r = r0; A.live = true;
    B.sc = &scratch[2 * wv + 1]; B.live = r0 + 1 < rays; B.r = B.live ? r0 + 1 : r0;
    mrg_load(A, rgbs1, t1, rgbs2, t2, perm2, perm != nullptr); mrg_load(B, rgbs1, t1, rgbs2, t2, perm2, perm != nullptr);
    mrg_park(A); mrg_park(B);
    wave_sync();
    mrg_search(A); mrg_search(B);
    wave_sync();                                    // last[] is zeroed before the max-scatter
    mrg_scatter_last(A); mrg_scatter_last(B);
    wave_sync();
    const bool slowA = mrg_ranks(A), slowB = mrg_ranks(B);
    if (slowA) stable_ranks_n<2>(A.sc->key, 128, A.rank);      // per ray: the other one keeps its merge ranks
    if (slowB) stable_ranks_n<2>(B.sc->key, 128, B.rank);
    wave_sync();                                    // last[] is read before z is written over it
    mrg_scatter(A, perm); mrg_scatter(B, perm);
    wave_sync();                                    // the keys are read before the weights are written over them
    float fTA, waA, fTB, waB;
    mrg_march(A, marcher, flags, density_bias, cut_thr, fTA, waA); mrg_march(B, marcher, flags, density_bias, cut_thr, fTB, waB);
    wave_sync();
    if (marcher == 0 && (flags & 2)) { mrg_last_back(A, waA); mrg_last_back(B, waB); }
    wave_sync();
    mrg_composite(A, marcher, flags, waA, fTA, rgb, depth_o, wsum_o, final_T); mrg_composite(B, marcher, flags, waB, fTB, rgb, depth_o, wsum_o, final_T);
}

// The launch of every per-ray kernel family: `kernel` is the instantiation the entry point selected (all instantiations of a family share
// one signature), one wave per ray and RAYS_PER_BLOCK rays per block; the pair forms pass their own rays per block.  A statement of
// the entry point: it reads its `rays` and `stream`, and like TDGP_LAUNCH_CHECK returns from it only on a launch error.
#define TDGP_LAUNCH_RAYS(NAME, KERNEL, PER_BLOCK, ...)                                                                                   \
    do {                                                                                                                                 \
        TDGP_LAUNCH(NAME, KERNEL, dim3((int)cdiv64(rays, PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                   \
        TDGP_LAUNCH_CHECK();                                                                                                             \
    } while (0)

}  // namespace

TDGP_API int tdgp_sample_stratified(const float* u, float* sdist, float* tdist, int64_t rays, int S, int marcher, float t_near,
                                    float t_far, tdgp_stream_t stream) {
    TDGP_CHECK(u && sdist, TDGP_EINVAL, "sample_stratified: null pointer");
    TDGP_CHECK(S >= 2 && rays >= 0, TDGP_EINVAL, "sample_stratified: need S >= 2");
    TDGP_CHECK(marcher == 0 || marcher == 1, TDGP_EINVAL, "sample_stratified: unknown ray marcher %d", marcher);
    const int64_t n = rays * S;
    if (n == 0) return TDGP_OK;
    if ((S & 3) == 0 && (((uintptr_t)u | (uintptr_t)sdist | (uintptr_t)tdist) & 15) == 0) {
        TDGP_LAUNCH("stratified_kernel", stratified4_kernel, dim3((int)min((int64_t)8192, cdiv64(n / 4, 256))), dim3(256), 0, (hipStream_t)stream, (const float4*)u,
                    (float4*)sdist, (float4*)tdist, n / 4, S, marcher, t_near, t_far);
        TDGP_LAUNCH_CHECK();
        return TDGP_OK;
    }
    TDGP_LAUNCH("stratified_kernel", stratified_kernel, dim3((int)min((int64_t)8192, cdiv64(n, 256))), dim3(256), 0, (hipStream_t)stream, u, sdist, tdist, n, S,
                       marcher, t_near, t_far);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_density_activation(const float* sigma, float* out, int64_t n, int flags, float density_bias, tdgp_stream_t stream) {
    TDGP_CHECK(sigma && out, TDGP_EINVAL, "density_activation: null pointer");
    TDGP_CHECK(n >= 0, TDGP_EINVAL, "density_activation: negative length");
    if (n == 0) return TDGP_OK;
    TDGP_LAUNCH("density_activation_kernel", density_activation_kernel, dim3((int)min((int64_t)8192, cdiv64(n, 256))), dim3(256), 0, (hipStream_t)stream, sigma, out, n,
                (flags & 8) ? 1 : 0, density_bias);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_ray_march(const float* colors, const float* densities, const float* depths, float* rgb, float* depth, float* weights,
                            float* final_T, int64_t rays, int S, int C, int marcher, int flags, float density_bias, float cut_threshold, tdgp_stream_t stream) {
    TDGP_CHECK(colors && densities && depths && rgb && depth && final_T, TDGP_EINVAL, "ray_march: null pointer");
    TDGP_CHECK(S >= 2 && S <= MAXS_LONG, TDGP_EUNSUPPORTED, "ray_march: S=%d outside [2,%d] (a merged list of at most %d + %d samples)", S, MAXS_LONG,
               MAXS_PASS, MAXS_PASS);
    TDGP_CHECK(C >= 1 && C <= 8, TDGP_EUNSUPPORTED, "ray_march: C=%d outside [1,8]", C);
    TDGP_CHECK(marcher == 0 || marcher == 1, TDGP_EINVAL, "ray_march: unknown ray marcher %d", marcher);
    TDGP_FAULT_CHECK("ray_march");
    if (rays == 0) return TDGP_OK;
    TDGP_LAUNCH_RAYS("ray_march_kernel", S <= MAXS ? ray_march_kernel<MAXS> : ray_march_kernel<MAXS_LONG>, RAYS_PER_BLOCK, colors, densities, depths, rgb, depth,
                     weights, final_T, rays, S, C, marcher, flags, density_bias, cut_threshold);
    return TDGP_OK;
}

TDGP_API int tdgp_sample_importance(const float* z, const float* weights, const float* u, float* samples, int32_t* inds, int32_t* below,
                                    int32_t* above, float* cdf, int64_t rays, int S, int Wn, int N, int marcher, tdgp_stream_t stream) {
    TDGP_CHECK(z && weights && u && samples, TDGP_EINVAL, "sample_importance: null pointer");
    TDGP_CHECK(!inds || (below && above), TDGP_EINVAL, "sample_importance: inds/below/above come together");
    TDGP_CHECK(S >= 4 && S <= MAXS_PASS && Wn >= 3 && Wn <= S && N >= 1, TDGP_EUNSUPPORTED,
               "sample_importance: bad S=%d Wn=%d N=%d (S at most %d: beyond it torch's sum order is not restated)", S, Wn, N, MAXS_PASS);
    if (rays == 0) return TDGP_OK;
    TDGP_LAUNCH_RAYS("sample_importance_kernel", S <= MAXS ? sample_importance_kernel<MAXS> : sample_importance_kernel<MAXS_PASS>, RAYS_PER_BLOCK, z, weights, u,
                     samples, inds, below, above, cdf, rays, S, Wn, N, marcher);
    return TDGP_OK;
}

TDGP_API int tdgp_unify_samples(const float* d1, const float* c1, const float* s1, int S1, const float* d2, const float* c2, const float* s2,
                                int S2, float* d, float* c, float* s, int32_t* perm, int64_t rays, int C, tdgp_stream_t stream) {
    TDGP_CHECK(d1 && c1 && s1 && d2 && c2 && s2 && d && c && s, TDGP_EINVAL, "unify_samples: null pointer");
    TDGP_CHECK(S1 >= 1 && S2 >= 1 && S1 + S2 <= MAXS_LONG, TDGP_EUNSUPPORTED, "unify_samples: S1+S2=%d > %d", S1 + S2, MAXS_LONG);
    if (rays == 0) return TDGP_OK;
    TDGP_LAUNCH_RAYS("unify_kernel", S1 + S2 <= MAXS ? unify_kernel<MAXS> : unify_kernel<MAXS_LONG>, RAYS_PER_BLOCK, d1, c1, s1, S1, d2, c2, s2, S2, d, c, s, perm,
                     rays, C);
    return TDGP_OK;
}

TDGP_API int tdgp_importance_from_coarse(const float* rgbs_coarse, const float* sdist, const float* u_fine, float* tdist_fine,
                                         float* sdist_fine, int32_t* inds, int32_t* fine_perm, int64_t rays, int S, int N, int marcher, int flags,
                                         float density_bias, float cut_threshold, float t_near, float t_far, tdgp_stream_t stream) {
    TDGP_CHECK(rgbs_coarse && sdist && u_fine && tdist_fine, TDGP_EINVAL, "importance_from_coarse: null pointer");
    TDGP_CHECK(S >= 4 && S <= MAXS_PASS && N >= 1 && N <= MAXS_PASS, TDGP_EUNSUPPORTED, "importance_from_coarse: bad S=%d N=%d (both at most %d)", S, N, MAXS_PASS);
    TDGP_CHECK(marcher == 0 || marcher == 1, TDGP_EINVAL, "importance_from_coarse: unknown ray marcher %d", marcher);
    TDGP_FAULT_CHECK("importance_from_coarse");
    if (rays == 0) return TDGP_OK;
    if (S == 64 && N == 64) {       // the generator's 64 + 64: two rays per wave (the sizes are the kernel's own)
        TDGP_LAUNCH_RAYS("importance_from_coarse_kernel", importance_from_coarse_pair_kernel, PAIR_RAYS_PER_BLOCK, rgbs_coarse, sdist, u_fine, tdist_fine, sdist_fine,
                         inds, fine_perm, rays, marcher, flags, density_bias, cut_threshold, t_near, t_far);
        return TDGP_OK;
    }
    const bool fits = S <= MAXS && N <= MAXS;       // else long rays: 16.4 KB of scratch per wave
    const auto kernel = (S <= 128 && N <= 128) ? importance_from_coarse_kernel<128> : fits ? importance_from_coarse_kernel<MAXS> : importance_from_coarse_kernel<MAXS_PASS>;
    TDGP_LAUNCH_RAYS("importance_from_coarse_kernel", kernel, RAYS_PER_BLOCK, rgbs_coarse, sdist, u_fine, tdist_fine, sdist_fine, inds, fine_perm, rays, S, N, marcher,
                     flags, density_bias, cut_threshold, t_near, t_far);
    return TDGP_OK;
}

TDGP_API int tdgp_merge_composite(const float* rgbs_coarse, const float* t_coarse, int S1, const float* rgbs_fine, const float* t_fine, int S2,
                                  float* rgb, float* depth, float* wsum, float* final_T, int32_t* perm, const int32_t* fine_perm, int64_t rays,
                                  int marcher, int flags, float density_bias, float cut_threshold, tdgp_stream_t stream) {
    TDGP_CHECK(rgbs_coarse && t_coarse && rgbs_fine && t_fine && rgb && depth, TDGP_EINVAL, "merge_composite: null pointer");
    TDGP_CHECK(S1 >= 1 && S2 >= 1 && S1 + S2 <= MAXS_LONG, TDGP_EUNSUPPORTED, "merge_composite: S1+S2=%d > %d", S1 + S2, MAXS_LONG);
    TDGP_CHECK(marcher == 0 || marcher == 1, TDGP_EINVAL, "merge_composite: unknown ray marcher %d", marcher);
    TDGP_FAULT_CHECK("merge_composite");
    if (rays == 0) return TDGP_OK;
    if (S1 == 64 && S2 == 64) {     // the generator's 64 + 64: two rays per wave (the sizes are the kernel's own)
        TDGP_LAUNCH_RAYS("merge_composite_kernel", merge_composite_pair_kernel, PAIR_RAYS_PER_BLOCK, rgbs_coarse, t_coarse, rgbs_fine, t_fine, rgb, depth, wsum, final_T,
                         perm, fine_perm, rays, marcher, flags, density_bias, cut_threshold);
        return TDGP_OK;
    }
    // 192: BASELINE configs[4], 96 + 96 samples -- three lane slots and 6.2 KB of scratch per wave instead of four and 8.2 KB.  Long rays: up to 256 + 256
    // in 16.4 KB per wave, twice the occupancy of the last form's 32.8 KB (last[] holds S1 + 1 <= MAXS_LONG entries)
    const int M = S1 + S2;
    const auto kernel = M <= 128 ? merge_composite_kernel<128> : M <= 192 ? merge_composite_kernel<192> : M <= MAXS ? merge_composite_kernel<MAXS>
                      : M <= MAXS_PASS ? merge_composite_kernel<MAXS_PASS> : merge_composite_kernel<MAXS_LONG>;
    TDGP_LAUNCH_RAYS("merge_composite_kernel", kernel, RAYS_PER_BLOCK, rgbs_coarse, t_coarse, S1, rgbs_fine, t_fine, S2, rgb, depth, wsum, final_T, perm, fine_perm,
                     rays, marcher, flags, density_bias, cut_threshold);
    return TDGP_OK;
}

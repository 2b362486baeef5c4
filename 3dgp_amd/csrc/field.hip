// field.hip -- fused tri-plane feature lookup + tiny MLP (the renderer's hot kernel).
//
// Replaces, per point, the reference's eager chain (src/training/tri_plane_renderer.py:560-588
// simple_tri_plane_renderer -> F.grid_sample(bilinear, align_corners=True, zeros) on 3 planes,
// networks_epigraf.py:46-68 TriPlaneMLP.forward: mean over planes, FC(F->hid, lrelu)*sqrt2, FC(hid->4)).
// The reference materialises a [3,F,P] gather result and a [P,hid] hidden tensor per 1M-point chunk
// (403 MB + 268 MB); here neither ever leaves registers.
//
// Layout / mapping (CDNA4, wave64):
//   * planes are plane-major channel-LAST [B,3,H,W,F]: one bilinear tap = one contiguous F*4-byte line
//     (128 B for F=32) instead of F strided 4-byte reads in NCHW;
//   * a wave processes tiles of 16 points; lane l = (pt = l & 15, q = l >> 4).  The 4 lanes that share a
//     point each gather a contiguous quarter of the channels (FQ = F/4 floats, 16/32-B vector loads) of the
//     12 taps, blend them, and hold FQ features of the plane-mean g[pt][q*FQ + s];
//   * layer 1 runs on the matrix cores as h^T[hid x 16pts] = W0s[hid x F] * g^T[F x 16pts] with
//     v_mfma_f32_16x16x4_f32: B operand = g (exactly the per-lane data the gather produced: k-slot = q),
//     A operand = W0s pre-arranged in registers; FQ k-steps per 16-row tile of hid, exact fp32;
//   * the accumulator layout then gives each lane 4*MT hidden units of ITS point, so lrelu is lane-local (the bias is
//     the accumulator's initial value), and layer 2 (hid -> 4) is 4*MT 16-block v_mfma_f32_4x4x1 steps + two cross-lane adds;
//   * ray walk: a wave marches the S samples of a 4x4-pixel quad; the taps of sample k+1 are in flight while sample k runs
//     its MLP, and results are parked in LDS and flushed as 128-B runs per ray (8 samples x 16 B).
// Where the code is: the body of the kernels is field_body<FQ, MT, NH, TAPS, WALK> in field_body.inc, shared with field_deep.hip (NH = hidden ->
// hidden layers; the kernels of this file are its NH = 0 instantiations), with the host code both forward entry points use; the producer /
// consumer walk is field_walk2.inc.  This file keeps FieldParams, the three kernels, the walk dispatch and the entry points.
// Roofline: 2*(F*hid + 4*hid) = 4608 MLP flop + 768 blend flop and 12 taps * F * 4 = 1536 B of L1/L2-served gathers per
// point; the tri-plane of one image (100.7 MB at 512^2 x 96) is read from HBM once and then lives in
// L2 / Infinity Cache.  Output traffic 16 B per point.
// Measured (r02, tools/dev/ubench_overlap2.hip): fp32 MFMA and every vector-ALU instruction of ANY wave of a SIMD issue through one
// port (5-7 cycles of matrix time per VALU instruction, 5.4 for a packed one), LDS and vector-memory instructions overlap.  Per
// 16-point tile this kernel issues 64 MFMAs (1152 cycles) and ~142 vector instructions (316 in r01) and takes ~2900 cycles per
// SIMD; 4.95 ms per 67 M points, matrix pipe 43 % busy.  DESIGN.md (e) lists what was tried on top and measured slower.
#include "common.h"

constexpr int WALK_WAVES = 2;  // waves per SIMD the table walk is compiled for (3: 168 registers, 24 spilled -- measured slower)

namespace {

struct FieldParams {
    const float* planes;   // [B,3,H,W,F]
    const float* coords;   // [B,P,3] or null
    const float* ray_o;    // [B*R,3]
    const float* ray_d;    // [B*R,3]
    const float* t;        // [B*R*S]
    const float* w0; const float* b0; const float* w1; const float* b1;
    float* rgbs;           // [B*P,4]
    const float* snoise;   // [B*P] standard-normal draws or null: sigma += snoise * snoise_std (tri_plane_renderer.py:185-186)
    float snoise_std;
    int32_t* tap_idx;      // [B*P,3,2] or null
    int64_t total;         // B*P
    int64_t P;
    int S, H, W;
    float scale, inv_scale, g0, g1;
    int scale_is_pow2;     // scale is a power of two: x * (1/scale) == x / scale exactly
    int marcher;
    int ray_h, ray_w;      // > 0: rays form a [B, ray_h, ray_w] image -> waves walk 4x4-pixel tiles (cache locality); 0: linear point order
    int64_t R;             // rays per sample
    uint32_t planes_bytes; // B*3*H*W*F*4 when it fits a buffer descriptor (< 4 GiB), else 0
    int* fault;            // the library's device-fault word (pinned host memory) or null
    // what field_body.inc asks of a parameter struct: layer i = 0 (first) or 1 (output)
    __device__ const float* weight(int i) const { return i == 0 ? w0 : w1; }
    __device__ const float* bias(int i) const { return i == 0 ? b0 : b1; }
    __device__ float out_gain() const { return g1; }
};

template <int N>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float* v) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; i++) {
            float4 t = ((const float4*)p)[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    } else if constexpr (N % 2 == 0) {
#pragma unroll
        for (int i = 0; i < N / 2; i++) {
            float2 t = ((const float2*)p)[i];
            v[2 * i] = t.x; v[2 * i + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = p[i];
    }
}

// field_body<FQ, MT, NH, TAPS, WALK>: the forward body (shared with field_deep.hip, whose kernel is its NH = 1, 2 instantiation), the
// texel / channel helpers and the host code of the forward entry points
#include "field_body.inc"

template <int FQ, int MT, bool TAPS>
__global__ __launch_bounds__(256, 2) void triplane_field_kernel(FieldParams p) { field_body<FQ, MT, 0, TAPS, false>(p); }

template <int FQ, int MT, bool TAPS>
__global__ __launch_bounds__(256, WALK_WAVES) void triplane_walk_kernel(FieldParams p) { field_body<FQ, MT, 0, TAPS, true>(p); }

#include "field_walk2.inc"

// NCHW planes [B,3F,H,W] -> [B,3,H,W,F] through an LDS tile of 64 pixels x F channels.
// The lookup alone: mean over the three planes of the bilinear samples, feats [B,P,F] -- simple_tri_plane_renderer's input to TriPlaneMLP
// (tri_plane_renderer.py:575-586, networks_epigraf.py:55).  The path of the decoders the fused kernels do not cover (tri_plane.mlp.n_layers != 2,
// has_view_cond, widths outside its table; round 6): their MLP then runs as eager tensor ops on this output, exactly as the reference's.  Built for
// correctness, not speed -- thread = (point, 4 channels) -- and written in torch's own evaluation order: per plane nw * a, + ne * b, + sw * c, + se * d
// (separate multiplies and adds), ((f0 + f1) + f2) / 3.
__global__ __launch_bounds__(256) void triplane_features_kernel(const float* __restrict__ planes, const float* __restrict__ coords, float* __restrict__ feats,
                                                                int64_t total, int64_t P, int F, int H, int W, float scale) {
    const int fq = F >> 2;
    const float sx = (float)(W - 1) / 2.f, sy = (float)(H - 1) / 2.f;
    const int64_t plane_elems = (int64_t)H * W * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total * fq; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gp = i / fq;
        const int c4 = (int)(i - gp * fq) * 4;
        const int64_t b = gp / P;
        const float* cp = coords + gp * 3;
        const float qc[3] = {cp[0] / scale, cp[1] / scale, cp[2] / scale};
        float4 acc[3];
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const float u = qc[pl == 2 ? 1 : 0], v = qc[pl == 0 ? 1 : 2];
            const float ix = (u + 1.0f) * sx, iy = (v + 1.0f) * sy;
            const float fx = floorf(ix), fy = floorf(iy);
            const float tw = ix - fx, te = 1.0f - tw, tn = iy - fy, ts = 1.0f - tn;
            const float cfx = fx < -2.f ? -2.f : (fx > (float)W ? (float)W : fx), cfy = fy < -2.f ? -2.f : (fy > (float)H ? (float)H : fy);
            const int x0 = (int)cfx, y0 = (int)cfy;
            const float w4[4] = {ts * te, ts * tw, tn * te, tn * tw};
            const float* base = planes + (b * 3 + pl) * plane_elems + c4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int x = x0 + (k & 1), y = y0 + (k >> 1);
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);                      // zero padding: the tap VALUE is 0, its weight stays (torch's order)
                if (x >= 0 && x < W && y >= 0 && y < H) t = *(const float4*)(base + ((int64_t)y * W + x) * F);
                if (k == 0) a = make_float4(t.x * w4[0], t.y * w4[0], t.z * w4[0], t.w * w4[0]);
                else a = make_float4(a.x + t.x * w4[k], a.y + t.y * w4[k], a.z + t.z * w4[k], a.w + t.w * w4[k]);
            }
            acc[pl] = a;
        }
        *(float4*)(feats + gp * F + c4) = make_float4(((acc[0].x + acc[1].x) + acc[2].x) / 3.0f, ((acc[0].y + acc[1].y) + acc[2].y) / 3.0f,
                                                      ((acc[0].z + acc[1].z) + acc[2].z) / 3.0f, ((acc[0].w + acc[1].w) + acc[2].w) / 3.0f);
    }
}

__global__ __launch_bounds__(256) void planes_to_hwc_kernel(const float* __restrict__ src, float* __restrict__ dst, int F, int HW, int64_t ntiles,
                                                           int tiles_per_plane) {
    extern __shared__ float tile[];      // [F][65]
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t plane = t / tiles_per_plane;       // b*3 + pl
        const int p0 = (int)(t % tiles_per_plane) * 64;
        const int np = min(64, HW - p0);
        for (int i = threadIdx.x; i < F * 64; i += blockDim.x) {
            int c = i >> 6, px = i & 63;
            if (px < np) tile[c * 65 + px] = src[(plane * F + c) * (int64_t)HW + p0 + px];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < F * 64; i += blockDim.x) {
            int px = i / F, c = i % F;
            if (px < np) dst[(plane * (int64_t)HW + p0 + px) * F + c] = tile[c * 65 + px];
        }
        __syncthreads();
    }
}

template <int FQ, int MT, bool TAPS>
void launch_field_t(const FieldParams& p, hipStream_t s) {
    const bool walk = FQ % 4 == 0 && p.ray_w > 0 && p.planes_bytes != 0;
    // hid_dim 16 (MT = 1) is not built as a producer / consumer walk.  In those instantiations the compiler runs out of scalar registers (24-28 SGPRs
    // spilled, the plane bases of the walk held in vector registers), and the `v_readfirstlane_b32` that brings a plane base back stands 1-4 wait states
    // in front of the hand-issued `buffer_load_dwordx4` that reads it as its scalar offset.  CDNA wants 5 between a vector instruction that writes an
    // SGPR and a vector-memory instruction that reads it; the compiler pads its own memory instructions and cannot see into the asm statement, so the
    // load goes out with whatever the register held before: a memory fault.  (32,16) also needs 48-56 B of scratch there.  Both pairs take the table
    // walk below, which gives the same bytes; how much slower that is than a working walk2 would be for (32,16) and (16,16) image walks with
    // S % 4 == 0 and S >= 16 has not been measured.  isa_check refuses any walk2 instantiation with that hazard or with scratch.
    if constexpr (FQ % 4 == 0 && FQ <= 8 && MT > 1) {
        // producer / consumer walk (field_walk2.inc): whole groups of four samples, a ring that is shorter than a patch's march
        // (the walk addresses ray_o / ray_d / t through scalar base + 32-bit byte offset)
        if (walk && (p.S & 3) == 0 && p.S >= 16 && p.total * 4 < ((int64_t)1 << 32) && (p.total / p.S) * 12 < ((int64_t)1 << 32)) {
            using L = Walk2Lds<FQ, MT>;
            const int cus = tdgp_cu_count();
            TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)triplane_walk2_kernel<FQ, MT, TAPS>, hipFuncAttributeMaxDynamicSharedMemorySize, L::total));
            const int ps = 8;                                            // patch side (field_walk2.inc)
            const int64_t npatch = (p.total / p.P) * cdiv(p.ray_w, ps) * cdiv(p.ray_h, ps);
            int blocks = (int)min((int64_t)cus, npatch);                // one 512-thread block per CU, each striding over the patches
            if (blocks > 8) blocks -= blocks % 8;
            TDGP_LAUNCH("triplane_field_kernel", (triplane_walk2_kernel<FQ, MT, TAPS>), dim3(blocks), dim3(512), L::total, s, p);
            return;
        }
    }
    static std::atomic<int> resident_pc[2];                  // persistent_blocks' cache: generic kernel, table walk
    if constexpr (FQ % 4 == 0) {
        if (walk) {
            const int blocks = persistent_blocks(triplane_walk_kernel<FQ, MT, TAPS>, resident_pc[1], field_work_blocks(p));
            TDGP_LAUNCH("triplane_field_kernel", (triplane_walk_kernel<FQ, MT, TAPS>), dim3(blocks), dim3(256), 0, s, p);
            return;
        }
    }
    const int blocks = persistent_blocks(triplane_field_kernel<FQ, MT, TAPS>, resident_pc[0], field_work_blocks(p));
    TDGP_LAUNCH("triplane_field_kernel", (triplane_field_kernel<FQ, MT, TAPS>), dim3(blocks), dim3(256), 0, s, p);
}

template <int FQ, int MT>
void launch_field(const FieldParams& p, hipStream_t s) {
    if (p.tap_idx) { launch_field_t<FQ, MT, true>(p, s); return; }
    launch_field_t<FQ, MT, false>(p, s);
}

}  // namespace

TDGP_API int tdgp_planes_to_hwc(const float* planes_nchw, float* planes_hwc, int B, int F, int H, int W, tdgp_stream_t stream) {
    TDGP_CHECK(planes_nchw && planes_hwc, TDGP_EINVAL, "planes_to_hwc: null pointer");
    TDGP_CHECK(B >= 0 && F >= 1 && F <= 256 && H >= 1 && W >= 1, TDGP_EINVAL, "planes_to_hwc: bad shape");
    if (B == 0) return TDGP_OK;
    const int HW = H * W;
    const int tpp = cdiv(HW, 64);
    const int64_t ntiles = (int64_t)B * 3 * tpp;
    TDGP_LAUNCH("planes_to_hwc_kernel", planes_to_hwc_kernel, dim3((int)min((int64_t)65535, ntiles)), dim3(256), F * 65 * sizeof(float), (hipStream_t)stream,
                       planes_nchw, planes_hwc, F, HW, ntiles, tpp);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_triplane_features(const float* planes_hwc, const float* coords, float* feats, int B, int64_t P, int F, int H, int W, float scale,
                                    tdgp_stream_t stream) {
    TDGP_CHECK(planes_hwc && coords && feats, TDGP_EINVAL, "triplane_features: null pointer");
    TDGP_CHECK(B >= 0 && P >= 0 && H >= 2 && W >= 2 && F >= 4 && (F & 3) == 0, TDGP_EINVAL, "triplane_features: bad shape (feat_dim must be a multiple of 4)");
    TDGP_CHECK((int64_t)B * P <= INT32_MAX / 4, TDGP_EINVAL, "triplane_features: tensor too large");
    if (B == 0 || P == 0) return TDGP_OK;
    const int64_t work = (int64_t)B * P * (F >> 2);
    TDGP_LAUNCH("triplane_features_kernel", triplane_features_kernel, dim3((unsigned)std::min<int64_t>(65535 * 4, cdiv64(work, 256))), dim3(256), 0, (hipStream_t)stream,
                planes_hwc, coords, feats, (int64_t)B * P, P, F, H, W, scale);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_triplane_field(const float* planes_hwc, const float* coords, const float* ray_o, const float* ray_d, const float* t,
                                 const float* w0, const float* b0, const float* w1, const float* b1, const float* sigma_noise, float density_noise,
                                 float* rgbs, int32_t* tap_idx, int B, int64_t P, int S, int ray_w, int F, int H, int W, int hid, float scale,
                                 int marcher, tdgp_stream_t stream) {
    TDGP_CHECK(planes_hwc && w0 && b0 && w1 && b1 && rgbs, TDGP_EINVAL, "triplane_field: null pointer");
    FieldParams p;
    bool empty;
    const int rc = field_common_params(p, "triplane_field", &empty, planes_hwc, coords, ray_o, ray_d, t, sigma_noise, density_noise, rgbs, tap_idx, B, P, S,
                                       ray_w, F, H, W, scale, marcher);
    if (rc != TDGP_OK || empty) return rc;
    p.w0 = w0; p.b0 = b0; p.w1 = w1; p.b1 = b1;
    p.g1 = (float)(1.0 / sqrt((double)hid));
    { const int64_t pb = (int64_t)B * 3 * H * W * F * 4; p.planes_bytes = (pb < ((int64_t)1 << 32) - 65536 && (int64_t)W * F * 4 < (1 << 24)) ? (uint32_t)pb : 0u; }
    p.fault = tdgp_fault_word();
    hipStream_t s = (hipStream_t)stream;
    bool ok = true;
#define FIELD_CASE(FF, HH) else if (F == FF && hid == HH) launch_field<FF / 4, HH / 16>(p, s);
    if (false) {}
    FIELD_CASE(32, 64) FIELD_CASE(32, 32) FIELD_CASE(32, 128) FIELD_CASE(32, 16)
    FIELD_CASE(16, 64) FIELD_CASE(16, 32) FIELD_CASE(16, 16)
    FIELD_CASE(8, 64) FIELD_CASE(8, 32) FIELD_CASE(8, 16)
    FIELD_CASE(64, 64) FIELD_CASE(64, 128)
    else ok = false;
#undef FIELD_CASE
    TDGP_CHECK(ok, TDGP_EUNSUPPORTED, "triplane_field: no kernel for feat_dim=%d, hid_dim=%d (the pairs of the table: feat 8 / 16 with hid 16, 32, 64; feat 32 with hid 16, 32, 64, 128; feat 64 with hid 64, 128)", F, hid);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// field_deep.hip -- the tri-plane field for 3- and 4-layer decoders (tri_plane.mlp.n_layers = 3, 4): forward and gradient.
//
// Reference: the same eager chain as field.hip (tri_plane_renderer.py:560-588 simple_tri_plane_renderer, networks_epigraf.py:46-68
// TriPlaneMLP.forward) with dims = [feat] + [hid] * (n_layers - 1) + [4]: FC(feat -> hid, lrelu), n_layers - 2 x FC(hid -> hid, lrelu), FC(hid -> 4).
//
// What is shared, and where:
//   field_body.inc  the forward body field_body<FQ, MT, NH, TAPS, WALK> -- geometry, tap addressing, zero padding, blend, layer-1 passes, output
//                   layer, generic image walk with its flush, linear tile loop -- of which triplane_field_deep_kernel is the NH = 1, 2
//                   instantiation (field.hip's kernels are NH = 0), load_texel / feat_of, the persistent-grid launcher and the argument checks
//                   common to tdgp_triplane_field and tdgp_triplane_field_deep.  The hidden -> hidden staging and layer loop live there too,
//                   behind `if constexpr (NH > 0)`.  So the tap rows written here equal the two-layer kernels' because they are the same statements;
//   field_grad.inc  the gradient kernels' stage 1 (geometry + gather), stage 6a (d_coords) and stage 6 (tap table + atomic scatter), the panel
//                   pitch, the accumulator row map and the wave-level sync, shared with render_grad.hip's triplane_field_grad_kernel.
// What is this file's own: DeepParams and the dispatch table of the forward; the gradient kernel's MLP middle (stages 2-5: every layer's panel
// kept, bias gradients summed from the A operands), its block reduction (one slot, waves adding in turn -- the two-layer kernel has a slot per
// wave, a different summation order, so the "zero slot, write slot, sum waves" skeleton stays duplicated) and its fp64 grid reduce kernel; and
// the five lines that transpose dg through LDS before stage 6, which need one more sync here than in render_grad.hip.
// The two-layer kernels' mangled names and ISA are pinned (tests/test_abi.py, isa_check.py, every benchmark line): tools/compare_device_asm.py
// --compile --allow-added OLD NEW <file> is how a change to a shared file is shown to leave them alone.
//
// Forward, what the NH > 0 branches of the body add: after layer 1 lane (q, pt) of the 16-point tile holds hidden units 16 mt + 4 q + r of ITS point (accumulator layout of
// v_mfma_f32_16x16x4_f32).  That is a B operand of the same instruction (k-slot = lane >> 4) for k-step (mt, r) when the A operand is arranged
// as A[m][q] = W[16 mo + m][16 mt + 4 q + r]: a hidden -> hidden layer needs no cross-lane traffic and no LDS round trip for activations.  lrelu is
// lane-local (its sqrt 2 gain lives in the NEXT layer's weights), the bias is the initial accumulator, the 4x4x1 output layer follows unchanged.
// Per 16-point tile (F 32 / hid 64): 32 + 64 (n_layers - 2) MFMAs 16x16x4 + 16 MFMAs 4x4x1, i.e. 112 / 176 matrix instructions against the
// two-layer kernel's 48, and per hidden layer 16 LDS bias reads (b128) + 64 A-operand reads + 8 packed multiplies + 16 v_med3 on top of its
// ~142 vector instructions.  A operands of one hidden layer take hid * hid * 4 bytes of LDS (16 KiB at hid 64), which is why hid 128 is refused.
// Plain loads only (no hand-issued loads, no producer / consumer walk): nothing here needs an ISA checker.
//
// Gradient: render_grad.hip's 32-point tiles on v_mfma_f32_32x32x2_f32, with one more [HP][33] activation panel per wave and one more weight-
// gradient accumulator set per hidden layer; the d(pre-activation) panel is reused layer by layer on the way back.  Occupancy as built:
//   hid 33..64 (HP 64), NW = 2 waves per block: 86,784 B of LDS at n_layers 3, 120,576 B at 4 -- one block per CU, one wave on two of its four SIMDs,
//       each with the whole 512-register file (256 VGPR + 170 / 256 AGPR; the 4-layer kernel spills 204 B per lane, the others nothing);
//   hid <= 32 (HP 32), NW = 4: 78,848 B (two blocks per CU) / 100,096 B (one block per CU), one wave per SIMD, no spills.
#include "common.h"

namespace {

constexpr int DEEP_MAX_LAYERS = 4;

struct DeepParams {
    const float* planes;   // [B,3,H,W,F]
    const float* coords;   // [B,P,3] or null
    const float* ray_o;    // [B*R,3]
    const float* ray_d;    // [B*R,3]
    const float* t;        // [B*R*S]
    const float* w[DEEP_MAX_LAYERS]; const float* b[DEEP_MAX_LAYERS];     // raw module parameters, layer 0 .. n_layers - 1
    float* rgbs;           // [B*P,4]
    const float* snoise;   // [B*P] standard-normal draws or null
    float snoise_std;
    int32_t* tap_idx;      // [B*P,3,2] or null
    int64_t total;         // B*P
    int64_t P;
    int S, H, W;
    float scale, inv_scale, g0, gh;       // gh = 1 / sqrt(hid): gain of every layer behind the first
    int scale_is_pow2;
    int marcher;
    int ray_h, ray_w;
    int64_t R;
    // what field_body.inc asks of a parameter struct: layer i = 0 .. n_layers - 1
    __device__ const float* weight(int i) const { return w[i]; }
    __device__ const float* bias(int i) const { return b[i]; }
    __device__ float out_gain() const { return gh; }
};

#include "field_body.inc"

// NH = hidden -> hidden layers (n_layers - 2): 1 or 2
template <int FQ, int MT, int NH, bool TAPS>
__global__ __launch_bounds__(256, 2) void triplane_field_deep_kernel(DeepParams p) { field_body<FQ, MT, NH, TAPS, false>(p); }

template <int FQ, int MT, int NH, bool TAPS>
void launch_deep_t(const DeepParams& p, hipStream_t s) {
    static std::atomic<int> resident_pc;                     // persistent_blocks' cache for this instantiation
    const int blocks = persistent_blocks(triplane_field_deep_kernel<FQ, MT, NH, TAPS>, resident_pc, field_work_blocks(p));
    TDGP_LAUNCH("triplane_field_deep_kernel", (triplane_field_deep_kernel<FQ, MT, NH, TAPS>), dim3(blocks), dim3(256), 0, s, p);
}

template <int FQ, int MT>
void launch_deep(const DeepParams& p, int nh, hipStream_t s) {
    if (nh == 1) { if (p.tap_idx) launch_deep_t<FQ, MT, 1, true>(p, s); else launch_deep_t<FQ, MT, 1, false>(p, s); }
    else { if (p.tap_idx) launch_deep_t<FQ, MT, 2, true>(p, s); else launch_deep_t<FQ, MT, 2, false>(p, s); }
}

}  // namespace

TDGP_API int tdgp_triplane_field_deep(const float* planes_hwc, const float* coords, const float* ray_o, const float* ray_d, const float* t,
                                      const float* const* w, const float* const* b, int n_layers, const float* sigma_noise, float density_noise,
                                      float* rgbs, int32_t* tap_idx, int B, int64_t P, int S, int ray_w, int F, int H, int W, int hid, float scale,
                                      int marcher, tdgp_stream_t stream) {
    TDGP_CHECK(planes_hwc && w && b && rgbs, TDGP_EINVAL, "triplane_field_deep: null pointer");
    TDGP_CHECK(n_layers == 3 || n_layers == 4, TDGP_EUNSUPPORTED,
               "triplane_field_deep: n_layers=%d (3 or 4; two-layer decoders go through tdgp_triplane_field)", n_layers);
    const bool pair_ok = ((F == 32 || F == 16 || F == 8) && (hid == 64 || hid == 32 || hid == 16)) || (F == 64 && hid == 64);
    TDGP_CHECK(pair_ok, TDGP_EUNSUPPORTED,
               "triplane_field_deep: no kernel for feat_dim=%d, hid_dim=%d (need feat in {8,16,32} with hid in {16,32,64}, or 64/64)", F, hid);
    for (int i = 0; i < n_layers; i++) TDGP_CHECK(w[i] && b[i], TDGP_EINVAL, "triplane_field_deep: null layer %d", i);
    DeepParams p;
    bool empty;
    const int rc = field_common_params(p, "triplane_field_deep", &empty, planes_hwc, coords, ray_o, ray_d, t, sigma_noise, density_noise, rgbs, tap_idx, B, P,
                                       S, ray_w, F, H, W, scale, marcher);
    if (rc != TDGP_OK || empty) return rc;
    for (int i = 0; i < DEEP_MAX_LAYERS; i++) { p.w[i] = i < n_layers ? w[i] : nullptr; p.b[i] = i < n_layers ? b[i] : nullptr; }
    p.gh = (float)(1.0 / sqrt((double)hid));
    hipStream_t s = (hipStream_t)stream;
    const int nh = n_layers - 2;
#define DEEP_CASE(FF, HH) else if (F == FF && hid == HH) launch_deep<FF / 4, HH / 16>(p, nh, s);
    if (false) {}
    DEEP_CASE(32, 64) DEEP_CASE(32, 32) DEEP_CASE(32, 16)
    DEEP_CASE(16, 64) DEEP_CASE(16, 32) DEEP_CASE(16, 16)
    DEEP_CASE(8, 64) DEEP_CASE(8, 32) DEEP_CASE(8, 16)
    DEEP_CASE(64, 64)
#undef DEEP_CASE
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// =================================================================================================================================
// Gradient.  One wave = tiles of 32 points; lane = (point l32, half); v_mfma_f32_32x32x2_f32 throughout.  With L = n_layers, h_0 = g (the
// plane-mean features), Ws_j = w_j / sqrt(fan_in), h_j = lrelu(Ws_{j-1} h_{j-1} + b_{j-1}) sqrt2 for j = 1 .. L-1 and o = Ws_{L-1} h_{L-1} + b_{L-1}:
//     forward : h_j [hid x 32] panels kept in LDS (one per layer), o on the vector ALU
//     do = d_out (mip: through sigmoid * 1.002 - 0.001);   d_{L-1} = Ws_{L-1}^T do . lrelu'(h_{L-1}) sqrt2       -> the dh_pre panel
//     dWs_{L-1}^T [hid x 4] += h_{L-1} . do^T                                                                      K = the 32 points
//     for j = L-2 .. 1:  dWs_j [hid x hid] += d_{j+1} . h_j^T  (K = points);   d_j = Ws_j^T d_{j+1} . lrelu'(h_j) sqrt2  (K = hid; the
//                        product sits in accumulators while the panel is overwritten)
//     dWs_0 [hid x F] += d_1 . g^T;   dg = Ws_0^T d_1;   dg / 3 -> the 12 taps with fp32 atomics, d_coords as in render_grad.hip.
// Weight and bias gradients stay in registers over all tiles of a wave and are reduced wave -> block -> grid in a fixed order.
// Bias gradients: each lane sums the A operands it feeds to the weight-gradient GEMMs (one register per layer and tile).  Occupancy: the file header.
// =================================================================================================================================
namespace {

#include "field_grad.inc"      // fg_f32x16, FG_PITCH, fg_row_of, fg_wave_sync; included again in the tile loop for stages 1 and 6

struct DeepGradParams {
    const float* planes;       // [B,3,H,W,F]
    const float* coords;       // [B,P,3]
    const float* w[DEEP_MAX_LAYERS]; const float* b[DEEP_MAX_LAYERS];
    const float* d_out;        // [B,P,4]
    float* d_planes;           // accumulated into (caller zeroes) or null
    float* d_coords;           // [B,P,3] written, or null
    float* partial;            // [gridDim.x][npart]
    int64_t total, P;
    int F, hid, H, W, marcher, npart;
    float scale, g0, gh;
};

__host__ __device__ inline int deep_npart(int F, int hid, int nh) { return hid * F + hid + nh * (hid * hid + hid) + 4 * hid + 4; }

template <int MT, int NW, int NH>
__global__ __launch_bounds__(64 * NW) void triplane_field_deep_grad_kernel(DeepGradParams p) {
    constexpr int NT = 64 * NW;
    constexpr int HP = 32 * MT;                               // hid padded to whole MFMA tiles
    constexpr int HPP = HP + 1;                               // pitch of the hidden weight panels (odd: rows and columns both conflict-free)
    extern __shared__ __attribute__((aligned(16))) float dg_smem[];
    float* W0s = dg_smem;                                     // [HP][33]        w0 * g0, zero padded
    float* Whs = W0s + HP * FG_PITCH;                         // [NH][HP][HPP]   w_j * gh
    float* Wls = Whs + NH * HP * HPP;                         // [4][HP]         w_last * gh
    float* Bs = Wls + 4 * HP;                                 // [NH + 1][HP]
    float* wave_mem = Bs + (NH + 1) * HP;
    const int tid = threadIdx.x, l = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), l32 = l & 31, half = l >> 5;
    constexpr int PANEL = HP * FG_PITCH;
    constexpr int WAVE_FLOATS = 32 * FG_PITCH + (NH + 2) * PANEL + 4 * 32;
    float* gl = wave_mem + wv * WAVE_FLOATS;                  // [32 pts][33]          features
    float* hl = gl + 32 * FG_PITCH;                           // [NH + 1][HP][33]      h_1 .. h_{NH+1}
    float* dl = hl + (NH + 1) * PANEL;                        // [HP][33]              dh_pre of the layer being walked back
    float* dol = dl + PANEL;                                  // [4][32]               do

    for (int i = tid; i < HP * FG_PITCH; i += NT) {
        const int m = i / FG_PITCH, f = i % FG_PITCH;
        W0s[i] = (m < p.hid && f < p.F) ? p.w[0][m * p.F + f] * p.g0 : 0.f;
    }
    for (int i = tid; i < NH * HP * HPP; i += NT) {
        const int j = i / (HP * HPP), m = (i / HPP) % HP, k = i % HPP;
        Whs[i] = (m < p.hid && k < p.hid) ? p.w[1 + j][m * p.hid + k] * p.gh : 0.f;
    }
    for (int i = tid; i < 4 * HP; i += NT) { const int j = i / HP, m = i % HP; Wls[i] = m < p.hid ? p.w[NH + 1][j * p.hid + m] * p.gh : 0.f; }
    for (int i = tid; i < (NH + 1) * HP; i += NT) { const int j = i / HP, m = i % HP; Bs[i] = m < p.hid ? p.b[j][m] : 0.f; }
    __syncthreads();

    fg_f32x16 dW0a[MT], dWha[NH][MT][MT], dWla[MT];
    // bias gradients db_j[m] = sum over points of d_j[m][pt]: the weight-gradient GEMMs read d_j[m = mt*32 + l32][pt = 2 ks + half] as their A operand
    // anyway, so each lane sums what it reads -- ONE register per (layer, tile) instead of the 16 of the accumulator layout
    float dba[NH + 1][MT], dbla[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            dW0a[mt][r] = 0.f; dWla[mt][r] = 0.f;
#pragma unroll
            for (int j = 0; j < NH + 1; j++) dba[j][mt] = 0.f;
#pragma unroll
            for (int j = 0; j < NH; j++)
#pragma unroll
                for (int mi = 0; mi < MT; mi++) dWha[j][mt][mi][r] = 0.f;
        }
    const float* blp = p.b[NH + 1];
    const float blv[4] = {blp[0], blp[1], blp[2], blp[3]};
    const float sx = (float)(p.W - 1) / 2.f, sy = (float)(p.H - 1) / 2.f;
    const int fh = p.F / 2;                                   // channels of this lane in the gather: [half * fh, half * fh + fh)
    const float sqrt2 = 1.41421356237309515f;

    auto row_of = [&](int mt, int r) { return fg_row_of(mt, r, half); };      // (a lambda of its own: with fg_row_of called directly the listing moves)

    const int64_t ntiles = (p.total + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * NW + wv; tile < ntiles; tile += (int64_t)gridDim.x * NW) {
        const int64_t gp = tile * 32 + l32;
        const bool valid = gp < p.total;
        const int64_t gpc = valid ? gp : 0;
        const int b = (int)(gpc / p.P);
#define FIELD_GRAD_STAGE 1
#include "field_grad.inc"

        // ---- 2. forward: h_1 = act(W0s g + b0), h_{j+1} = act(Whs_j h_j + b_j), every panel kept ------------------------------
        fg_f32x16 hacc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) hacc[mt][r] = Bs[row_of(mt, r)];
#pragma unroll
        for (int ks = 0; ks < 16; ks++) {
            const float bf = gl[l32 * FG_PITCH + 2 * ks + half];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) hacc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(W0s[(mt * 32 + l32) * FG_PITCH + 2 * ks + half], bf, hacc[mt], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j <= NH; j++) {
            float* hj = hl + j * PANEL;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float hp = hacc[mt][r];
                    const float h = (hp > 0.f ? hp : hp * 0.2f) * sqrt2;
                    hacc[mt][r] = h;
                    hj[row_of(mt, r) * FG_PITCH + l32] = h;
                }
            if (j == NH) break;
            fg_wave_sync();
            const float* Wj = Whs + j * HP * HPP;
            fg_f32x16 nxt[MT];
#pragma unroll
            for (int mo = 0; mo < MT; mo++)
#pragma unroll
                for (int r = 0; r < 16; r++) nxt[mo][r] = Bs[(j + 1) * HP + row_of(mo, r)];
#pragma unroll 4
            for (int ks = 0; ks < HP / 2; ks++) {
                const int k = 2 * ks + half;                                      // input unit of this K step
                const float bf = hj[k * FG_PITCH + l32];                          // B[k][n = pt]
#pragma unroll
                for (int mo = 0; mo < MT; mo++) nxt[mo] = __builtin_amdgcn_mfma_f32_32x32x2f32(Wj[(mo * 32 + l32) * HPP + k], bf, nxt[mo], 0, 0, 0);
            }
#pragma unroll
            for (int mo = 0; mo < MT; mo++) hacc[mo] = nxt[mo];
        }
        // ---- 3. outputs, incoming gradient (hacc = h of the last hidden layer) -------------------------------------------------
        float oj[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = row_of(mt, r);
#pragma unroll
                for (int j = 0; j < 4; j++) oj[j] = fmaf_(Wls[j * HP + m], hacc[mt][r], oj[j]);
            }
        float dj[4] = {dout4.x, dout4.y, dout4.z, dout4.w};
#pragma unroll
        for (int j = 0; j < 4; j++) oj[j] = (oj[j] + __shfl_xor(oj[j], 32, 64)) + blv[j];
        if (p.marcher == 1) {
#pragma unroll
            for (int j = 0; j < 3; j++) { const float sg = 1.0f / (1.0f + expf(-oj[j])); dj[j] = dj[j] * 1.002f * sg * (1.0f - sg); }
        }
        if (half == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) { dbla[j] += dj[j]; dol[j * 32 + l32] = dj[j]; }
        }
        // ---- 4. dh_pre of the last hidden layer -> panel -------------------------------------------------------------------------
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = row_of(mt, r);
                float dh = 0.f;
#pragma unroll
                for (int j = 0; j < 4; j++) dh = fmaf_(Wls[j * HP + m], dj[j], dh);
                const float dhp = dh * sqrt2 * (hacc[mt][r] > 0.f ? 1.0f : 0.2f);
                dl[m * FG_PITCH + l32] = dhp;
            }
        fg_wave_sync();
        // ---- 5. weight-gradient GEMMs over the 32 points, walking the layers back ------------------------------------------------
        {
            const float* hlast = hl + NH * PANEL;
#pragma unroll
            for (int ks = 0; ks < 16; ks++) {
                const int k = 2 * ks + half;                                          // point index of this K step
                const float bd = l32 < 4 ? dol[l32 * 32 + k] : 0.f;                   // B[k = pt][n = j]
#pragma unroll
                for (int mt = 0; mt < MT; mt++) dWla[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(hlast[(mt * 32 + l32) * FG_PITCH + k], bd, dWla[mt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = NH - 1; j >= 0; j--) {
            const float* hj = hl + j * PANEL;                                         // h_{j+1}: the input of hidden layer j
            const float* Wj = Whs + j * HP * HPP;
#pragma unroll
            for (int ks = 0; ks < 16; ks++) {
                const int k = 2 * ks + half;                                          // point
                float bh[MT];
#pragma unroll
                for (int mi = 0; mi < MT; mi++) bh[mi] = hj[(mi * 32 + l32) * FG_PITCH + k];        // B[k = pt][n = input unit]
#pragma unroll
                for (int mo = 0; mo < MT; mo++) {
                    const float ad = dl[(mo * 32 + l32) * FG_PITCH + k];                            // A[m = output unit][k = pt]
                    dba[j + 1][mo] += ad;
#pragma unroll
                    for (int mi = 0; mi < MT; mi++) dWha[j][mo][mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(ad, bh[mi], dWha[j][mo][mi], 0, 0, 0);
                }
            }
            fg_f32x16 dh[MT];
#pragma unroll
            for (int mi = 0; mi < MT; mi++)
#pragma unroll
                for (int r = 0; r < 16; r++) dh[mi][r] = 0.f;
#pragma unroll 4
            for (int ks = 0; ks < HP / 2; ks++) {
                const int k = 2 * ks + half;                                          // output unit of this K step
                const float bd = dl[k * FG_PITCH + l32];                              // B[k][n = pt]
#pragma unroll
                for (int mi = 0; mi < MT; mi++) dh[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(Wj[k * HPP + mi * 32 + l32], bd, dh[mi], 0, 0, 0);   // A[m = input unit][k]
            }
            fg_wave_sync();                                                              // every lane has read the panel it is about to overwrite
#pragma unroll
            for (int mi = 0; mi < MT; mi++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int m = row_of(mi, r);
                    const float dhp = dh[mi][r] * sqrt2 * (hj[m * FG_PITCH + l32] > 0.f ? 1.0f : 0.2f);
                    dl[m * FG_PITCH + l32] = dhp;
                }
            fg_wave_sync();
        }
#pragma unroll
        for (int ks = 0; ks < 16; ks++) {
            const int k = 2 * ks + half;
            const float bg = gl[k * FG_PITCH + l32];                                  // B[k = pt][n = f]
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const float ad = dl[(mt * 32 + l32) * FG_PITCH + k];
                dba[0][mt] += ad;
                dW0a[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ad, bg, dW0a[mt], 0, 0, 0);
            }
        }
        fg_f32x16 dg;
#pragma unroll
        for (int r = 0; r < 16; r++) dg[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < HP / 2; ks++) {
            const int k = 2 * ks + half;
            dg = __builtin_amdgcn_mfma_f32_32x32x2f32(W0s[k * FG_PITCH + l32], dl[k * FG_PITCH + l32], dg, 0, 0, 0);   // A[m = f][k], B[k][n = pt]
        }
        // ---- 6. dg transposed through LDS (lane = point -> lane = channel), then d_coords and the scatter (field_grad.inc) ---------
        if (p.d_planes || p.d_coords) {
            fg_wave_sync();
#pragma unroll
            for (int r = 0; r < 16; r++) gl[l32 * FG_PITCH + row_of(0, r)] = dg[r];
            fg_wave_sync();
        }
#define FIELD_GRAD_STAGE 6
#include "field_grad.inc"
    }

    // ---- reduction of the weight gradients: the waves of a block add into ONE slot in wave order (the whole LDS is free now), then
    // partial[blockIdx].  Layout of the slot / of `partial`: dW0 [hid][F] | db0 [hid] | (dW_j [hid][hid] | db_j [hid]) x NH | dWl [4][hid] | dbl [4]
    __syncthreads();
    float* slot = dg_smem;                                       // >= npart floats (host check)
    auto sum32 = [&](float s) {
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 16, 64);
        return s;
    };
    for (int w = 0; w < NW; w++) {
        if (wv == w) {
            auto put = [&](int idx, float v) { if (w == 0) slot[idx] = v; else slot[idx] += v; };
            const int o_db0 = p.hid * p.F;
            int o_h = o_db0 + p.hid;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int m = row_of(mt, r);
                    if (m < p.hid && l32 < p.F) put(m * p.F + l32, dW0a[mt][r]);                      // C[m][n = f]
                }
            auto put_bias = [&](int off, int mt, float v) {                                        // lane (l32, half) summed the points of parity `half` of row mt*32 + l32
                const float s = v + __shfl_xor(v, 32, 64);
                if (half == 0 && mt * 32 + l32 < p.hid) put(off + mt * 32 + l32, s);
            };
#pragma unroll
            for (int mt = 0; mt < MT; mt++) put_bias(o_db0, mt, dba[0][mt]);
#pragma unroll
            for (int j = 0; j < NH; j++) {
#pragma unroll
                for (int mo = 0; mo < MT; mo++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int m = row_of(mo, r);
#pragma unroll
                        for (int mi = 0; mi < MT; mi++) {
                            const int n = mi * 32 + l32;
                            if (m < p.hid && n < p.hid) put(o_h + m * p.hid + n, dWha[j][mo][mi][r]);    // C[m = output unit][n = input unit]
                        }
                    }
#pragma unroll
                for (int mo = 0; mo < MT; mo++) put_bias(o_h + p.hid * p.hid, mo, dba[j + 1][mo]);
                o_h += p.hid * p.hid + p.hid;
            }
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int m = row_of(mt, r);
                    if (m < p.hid && l32 < 4) put(o_h + l32 * p.hid + m, dWla[mt][r]);                // C[m][n = j]
                }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float s = sum32(dbla[j]);
                if (l == 0) put(o_h + 4 * p.hid + j, s);
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < p.npart; i += NT) p.partial[(int64_t)blockIdx.x * p.npart + i] = slot[i];
}

struct DeepReduceSegs {
    int n;
    int end[2 * DEEP_MAX_LAYERS];          // exclusive end of segment i in a partial row
    float gain[2 * DEEP_MAX_LAYERS];
    float* out[2 * DEEP_MAX_LAYERS];
};

// d_w_j = gain_j * sum over blocks, d_b_j = sum over blocks: blocks summed in block order, in fp64 and rounded once -- up to 1536 partials per element
// summed one after the other in fp32 put the bias gradients 6e-7 of their maximum from the float64 result at 521 blocks, past twice the fp32 reference's own error
__global__ __launch_bounds__(256) void field_deep_grad_reduce_kernel(const float* __restrict__ partial, int nblocks, int npart, DeepReduceSegs sg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npart) return;
    double acc = 0.0;
    for (int k = 0; k < nblocks; k++) acc += (double)partial[(int64_t)k * npart + i];
    const float s = (float)acc;
    int begin = 0;
    for (int g = 0; g < sg.n; g++) {
        if (i < sg.end[g]) { sg.out[g][i - begin] = s * sg.gain[g]; return; }
        begin = sg.end[g];
    }
}

int deep_grad_blocks(int64_t total) { return (int)min((int64_t)1536, max((int64_t)1, cdiv64(total, 128))); }

template <int MT, int NW, int NH>
hipError_t launch_deep_grad(const DeepGradParams& p, int nb, size_t lds, hipStream_t s) {
    // 78.8 - 120.6 KB of dynamic LDS: above the 64 KB a kernel gets without asking.  Once per device, and marked done only when it succeeded: a refused
    // opt-in is reported by every call, not left to the launch error of the calls after the first
    static std::atomic<uint64_t> done[4];
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    std::atomic<uint64_t>& w = done[(dev >> 6) & 3];
    if (!(w.load(std::memory_order_acquire) & bit)) {
        const hipError_t e = hipFuncSetAttribute((const void*)triplane_field_deep_grad_kernel<MT, NW, NH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        w.fetch_or(bit, std::memory_order_release);
    }
    TDGP_LAUNCH("triplane_field_deep_grad_kernel", (triplane_field_deep_grad_kernel<MT, NW, NH>), dim3(nb), dim3(64 * NW), lds, s, p);
    return hipSuccess;
}

}  // namespace

TDGP_API int64_t tdgp_triplane_field_deep_grad_workspace_bytes(int B, int64_t P, int F, int hid, int n_layers) {
    if (n_layers != 3 && n_layers != 4) return -1;
    return (int64_t)deep_grad_blocks((int64_t)B * P) * deep_npart(F, hid, n_layers - 2) * (int64_t)sizeof(float);
}

TDGP_API int tdgp_triplane_field_deep_grad(const float* planes_hwc, const float* coords, const float* const* w, const float* const* b, int n_layers,
                                           const float* d_out, float* d_planes_hwc, float* const* d_w, float* const* d_b, float* d_coords,
                                           void* workspace, int64_t workspace_bytes, int B, int64_t P, int F, int H, int W, int hid, float scale,
                                           int marcher, tdgp_stream_t stream) {
    TDGP_CHECK(planes_hwc && coords && w && b && d_out && d_w && d_b, TDGP_EINVAL, "triplane_field_deep_grad: null pointer");
    TDGP_CHECK(n_layers == 3 || n_layers == 4, TDGP_EUNSUPPORTED,
               "triplane_field_deep_grad: n_layers=%d (3 or 4; two-layer decoders go through tdgp_triplane_field_grad)", n_layers);
    for (int i = 0; i < n_layers; i++) TDGP_CHECK(w[i] && b[i] && d_w[i] && d_b[i], TDGP_EINVAL, "triplane_field_deep_grad: null layer %d", i);
    TDGP_CHECK(B >= 1 && P >= 1 && H >= 2 && W >= 2, TDGP_EINVAL, "triplane_field_deep_grad: bad shape");
    TDGP_CHECK(F % 8 == 0 && F >= 8 && F <= 32, TDGP_EUNSUPPORTED, "triplane_field_deep_grad: feat_dim=%d (8, 16, 24 or 32)", F);
    TDGP_CHECK(hid >= 1 && hid <= 64, TDGP_EUNSUPPORTED, "triplane_field_deep_grad: hid_dim=%d > 64", hid);
    TDGP_CHECK(marcher == 0 || marcher == 1, TDGP_EINVAL, "triplane_field_deep_grad: unknown ray marcher %d", marcher);
    TDGP_CHECK((int64_t)B * 3 * H * W * F <= INT32_MAX, TDGP_EINVAL, "triplane_field_deep_grad: plane tensor too large");
    const int64_t need = tdgp_triplane_field_deep_grad_workspace_bytes(B, P, F, hid, n_layers);
    TDGP_CHECK(workspace && workspace_bytes >= need, TDGP_EINVAL, "triplane_field_deep_grad: workspace of %lld bytes needed", (long long)need);
    const int nh = n_layers - 2;
    DeepGradParams p;
    p.planes = planes_hwc; p.coords = coords; p.d_out = d_out; p.d_planes = d_planes_hwc; p.d_coords = d_coords;
    for (int i = 0; i < DEEP_MAX_LAYERS; i++) { p.w[i] = i < n_layers ? w[i] : nullptr; p.b[i] = i < n_layers ? b[i] : nullptr; }
    p.partial = (float*)workspace; p.total = (int64_t)B * P; p.P = P; p.F = F; p.hid = hid; p.H = H; p.W = W; p.marcher = marcher;
    p.npart = deep_npart(F, hid, nh);
    p.scale = scale; p.g0 = (float)(1.0 / sqrt((double)F)); p.gh = (float)(1.0 / sqrt((double)hid));
    const int nb = deep_grad_blocks(p.total);
    const int MT = hid <= 32 ? 1 : 2, HP = 32 * MT, NW = MT == 1 ? 4 : 2;
    const int wave_floats = 32 * FG_PITCH + (nh + 2) * HP * FG_PITCH + 4 * 32;
    const int lds_floats = HP * FG_PITCH + nh * HP * (HP + 1) + 4 * HP + (nh + 1) * HP + NW * wave_floats;
    TDGP_CHECK(p.npart <= lds_floats, TDGP_EUNSUPPORTED, "triplane_field_deep_grad: reduction slot too small");
    const size_t lds = (size_t)lds_floats * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    hipError_t le;
    if (MT == 1 && nh == 1) le = launch_deep_grad<1, 4, 1>(p, nb, lds, s);
    else if (MT == 1) le = launch_deep_grad<1, 4, 2>(p, nb, lds, s);
    else if (nh == 1) le = launch_deep_grad<2, 2, 1>(p, nb, lds, s);
    else le = launch_deep_grad<2, 2, 2>(p, nb, lds, s);
    TDGP_CHECK(le == hipSuccess, TDGP_ELAUNCH, "triplane_field_deep_grad: %zu bytes of dynamic LDS refused: %s", lds, hipGetErrorString(le));
    DeepReduceSegs sg;
    sg.n = 2 * n_layers;
    int end = 0;
    for (int i = 0; i < n_layers; i++) {
        const int fan_in = i == 0 ? F : hid, rows = i == n_layers - 1 ? 4 : hid;
        end += rows * fan_in; sg.end[2 * i] = end; sg.gain[2 * i] = i == 0 ? p.g0 : p.gh; sg.out[2 * i] = d_w[i];
        end += rows; sg.end[2 * i + 1] = end; sg.gain[2 * i + 1] = 1.0f; sg.out[2 * i + 1] = d_b[i];
    }
    TDGP_LAUNCH("field_deep_grad_reduce_kernel", field_deep_grad_reduce_kernel, dim3(cdiv(p.npart, 256)), dim3(256), 0, s, (const float*)workspace, nb,
                p.npart, sg);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

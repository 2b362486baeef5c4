// field_deep.hip -- the tri-plane field for 3- and 4-layer decoders (tri_plane.mlp.n_layers = 3, 4): forward and gradient.
//
// Reference: the same eager chain as field.hip (tri_plane_renderer.py:560-588 simple_tri_plane_renderer, networks_epigraf.py:46-68
// TriPlaneMLP.forward) with dims = [feat] + [hid] * (n_layers - 1) + [4]: FC(feat -> hid, lrelu), n_layers - 2 x FC(hid -> hid, lrelu), FC(hid -> 4).
//
// The geometry, tap addressing, zero padding and blend lambdas of the forward kernel (issue_taps, blend_pass, mlp_begin, mlp_pass and the
// generic image walk / linear tile loop) are COPIES of field.hip's field_body<.., WALK = false>, and the gather / scatter / coordinate-gradient
// stages of the gradient kernel are copies of render_grad.hip's triplane_field_grad_kernel.  That duplication is deliberate: the two-layer
// kernels' mangled names and ISA are pinned (tests/test_abi.py, isa_check.py, every benchmark line), so they are not touched, and the tap rows
// written here equal theirs bit for bit because the arithmetic is theirs statement for statement.  A change to the geometry goes into both files.
//
// Forward, what is new: after layer 1 lane (q, pt) of the 16-point tile holds hidden units 16 mt + 4 q + r of ITS point (accumulator layout of
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

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

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
};

template <int FQ>
__device__ __forceinline__ void load_texel(const float* __restrict__ texel, int c4, f32x2* v) {
    static_assert(FQ % 2 == 0, "feat_dim must be a multiple of 8");
    if constexpr (FQ % 4 == 0) {
#pragma unroll
        for (int j = 0; j < FQ / 4; j++) {
            const float4 t = *(const float4*)(texel + 16 * j + 4 * c4);
            v[2 * j] = (f32x2){t.x, t.y}; v[2 * j + 1] = (f32x2){t.z, t.w};
        }
    } else {
#pragma unroll
        for (int j = 0; j < FQ / 2; j++) {
            const float2 t = *(const float2*)(texel + c4 * FQ + 2 * j);
            v[j] = (f32x2){t.x, t.y};
        }
    }
}

// channel held in value slot s of the lane that serves k-slot q (field.hip: feat_of)
__host__ __device__ __forceinline__ int feat_of(int s, int q, int FQ) { return FQ % 4 == 0 ? 16 * (s >> 2) + 4 * q + (s & 3) : q * FQ + s; }

// NH = hidden -> hidden layers (n_layers - 2): 1 or 2
template <int FQ, int MT, int NH, bool TAPS>
__device__ __forceinline__ void field_deep_body(const DeepParams& p) {
    constexpr int F = FQ * 4;
    constexpr int HID = MT * 16;
    // MFMA A operands, one float per lane per k-step, stored [step][lane]:
    //   layer 1: a0s[mt*FQ + s][lane]                    = W0[mt*16 + (lane&15)][feat_of(s, lane>>4)] / sqrt(F) / 3
    //   hidden : ahs[((j*MT + mo)*MT + mt)*4 + r][lane]  = Wj[mo*16 + (lane&15)][mt*16 + 4*(lane>>4) + r] * sqrt(2)/sqrt(HID)
    //   output : a1s[mt*4 + r][lane]                     = Wl[lane&3][mt*16 + 4*(lane>>4) + r] * sqrt(2)/sqrt(HID)
    __shared__ float a0s[MT * FQ * 64];
    __shared__ float ahs[NH * MT * MT * 4 * 64];
    __shared__ float a1s[MT * 4 * 64];
    __shared__ __attribute__((aligned(16))) float bs[(NH + 1) * HID];      // biases of layer 1 and of the hidden layers
    constexpr int NW = 4;
    constexpr int PW = 8;
    __shared__ float4 obuf_all[NW * 16 * 9];
    const float sqrt2 = 1.41421353816986083984375f;
    for (int i = threadIdx.x; i < MT * FQ * 64; i += blockDim.x) {
        const int ln = i & 63, ms = i >> 6, mt = ms / FQ, sidx = ms % FQ;
        a0s[i] = (p.w[0][(mt * 16 + (ln & 15)) * F + feat_of(sidx, ln >> 4, FQ)] * p.g0) / 3.0f;
    }
    for (int i = threadIdx.x; i < NH * MT * MT * 4 * 64; i += blockDim.x) {
        const int ln = i & 63, ms = i >> 6, r = ms & 3, mt = (ms >> 2) % MT, mo = ((ms >> 2) / MT) % MT, j = (ms >> 2) / (MT * MT);
        ahs[i] = (p.w[1 + j][(mo * 16 + (ln & 15)) * HID + mt * 16 + 4 * (ln >> 4) + r] * p.gh) * sqrt2;
    }
    for (int i = threadIdx.x; i < MT * 4 * 64; i += blockDim.x) {
        const int ln = i & 63, ms = i >> 6, mt = ms >> 2, r = ms & 3;
        a1s[i] = (p.w[NH + 1][(ln & 3) * HID + mt * 16 + 4 * (ln >> 4) + r] * p.gh) * sqrt2;
    }
    for (int i = threadIdx.x; i < (NH + 1) * HID; i += blockDim.x) bs[i] = p.b[i / HID][i % HID];
    __syncthreads();

    const int l = lane_id();
    const int pt = l & 15, q = l >> 4;
    const float sx = (float)(p.W - 1) / 2.f, sy = (float)(p.H - 1) / 2.f;
    const float* bl = p.b[NH + 1];
    const f32x4 o4init = (l >> 4) == 0 ? (f32x4){bl[0], bl[1], bl[2], bl[3]} : (f32x4){0.f, 0.f, 0.f, 0.f};
    const int plane_elems = p.H * p.W * F;
    const int gpt = (FQ % 4 == 0) ? (l >> 2) : pt, gc4 = (FQ % 4 == 0) ? (l & 3) : q;

    f32x2 tap[3][4][FQ / 2];
    float wgt[3][4];
    auto issue_taps = [&](float cx, float cy, float cz, const float* __restrict__ bplanes, int64_t ggp, bool gvalid) {
        float qc[3];
        if (p.scale_is_pow2) { qc[0] = cx * p.inv_scale; qc[1] = cy * p.inv_scale; qc[2] = cz * p.inv_scale; }   // exact == cx / scale
        else { qc[0] = cx / p.scale; qc[1] = cy / p.scale; qc[2] = cz / p.scale; }                                 // :576 true division
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const float u = qc[pl == 2 ? 1 : 0];          // planes (x,y), (x,z), (y,z): width <- first coordinate (:577-581)
            const float v = qc[pl == 0 ? 1 : 2];
            const float ix = (u + 1.0f) * sx, iy = (v + 1.0f) * sy;   // align_corners=True unnormalisation
            const float fx = floorf(ix), fy = floorf(iy);
            const float tw = ix - fx, te = 1.0f - tw, tn = iy - fy, ts = 1.0f - tn;
            const float cfx = fx < -2.f ? -2.f : (fx > (float)p.W ? (float)p.W : fx);
            const float cfy = fy < -2.f ? -2.f : (fy > (float)p.H ? (float)p.H : fy);
            const int x0 = (int)cfx, y0 = (int)cfy;
            if (TAPS) {
                if (p.tap_idx && gc4 == 0 && gvalid) {
                    p.tap_idx[(ggp * 3 + pl) * 2 + 0] = x0;
                    p.tap_idx[(ggp * 3 + pl) * 2 + 1] = y0;
                }
            }
            const bool vx0 = x0 >= 0 && x0 < p.W, vx1 = x0 + 1 >= 0 && x0 + 1 < p.W;
            const bool vy0 = y0 >= 0 && y0 < p.H, vy1 = y0 + 1 >= 0 && y0 + 1 < p.H;
            // zero padding: an out-of-range tap keeps a clamped (in-bounds) address and gets weight 0
            wgt[pl][0] = (vx0 && vy0) ? ts * te : 0.f;    // nw
            wgt[pl][1] = (vx1 && vy0) ? ts * tw : 0.f;    // ne
            wgt[pl][2] = (vx0 && vy1) ? tn * te : 0.f;    // sw
            wgt[pl][3] = (vx1 && vy1) ? tn * tw : 0.f;    // se
            const float* base = bplanes + pl * plane_elems;
            const int xa = min(max(x0, 0), p.W - 1), xb = min(max(x0 + 1, 0), p.W - 1);
            const int ya = min(max(y0, 0), p.H - 1), yb = min(max(y0 + 1, 0), p.H - 1);
            const int ra = ya * p.W, rb = yb * p.W;         // 32-bit element offsets inside one plane (< 2^31)
            load_texel<FQ>(base + (ra + xa) * F, gc4, tap[pl][0]);
            load_texel<FQ>(base + (ra + xb) * F, gc4, tap[pl][1]);
            load_texel<FQ>(base + (rb + xa) * F, gc4, tap[pl][2]);
            load_texel<FQ>(base + (rb + xb) * F, gc4, tap[pl][3]);
        }
    };
    constexpr int NP = (FQ % 4 == 0) ? FQ / 4 : 1;          // passes per tile
    constexpr int PP = (FQ % 4 == 0) ? 2 : FQ / 2;          // channel pairs per lane and pass
    auto blend_pass = [&](auto& T, int base, float* gp) {
#pragma unroll
        for (int s = 0; s < PP; s++) {
            f32x2 a = T[0][0][base + s] * (f32x2){wgt[0][0], wgt[0][0]};
#pragma unroll
            for (int j = 1; j < 12; j++) a = __builtin_elementwise_fma(T[j >> 2][j & 3][base + s], (f32x2){wgt[j >> 2][j & 3], wgt[j >> 2][j & 3]}, a);
            gp[2 * s] = a.x; gp[2 * s + 1] = a.y;
        }
        if (FQ % 4 == 0) {                                 // gather layout -> MFMA layout: lane (q, pt) takes from lane 4*pt + q
            const int src = (pt * 4 + q) * 4;
#pragma unroll
            for (int s = 0; s < 2 * PP; s++) gp[s] = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(gp[s])));
        }
    };
    auto mlp_begin = [&](f32x4* acc) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) acc[mt] = *(const f32x4*)(bs + mt * 16 + 4 * q);
    };
    auto mlp_pass = [&](f32x4* acc, int ps, const float* gp) {     // layer 1: h^T[hid x 16 pts] += W0s[:, pass] * g^T[pass]
#pragma unroll
        for (int i = 0; i < 2 * PP; i++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0s[(mt * FQ + ps * 2 * PP + i) * 64 + l], gp[i], acc[mt], 0, 0, 0);
    };
    // leaky_relu(v, 0.2) = max(v, 0.2 v) of the 4 hidden units a lane holds of tile mt: one packed multiply per pair + one v_med3 per value
    // (field.hip: mlp_finish has the reasons for the third operand and for not writing this in assembly)
    auto lrelu4 = [&](const f32x4 a, float* h) {
        const f32x2 c02 = {0.2f, 0.2f};
        const f32x2 lo = (f32x2){a[0], a[1]} * c02, hi = (f32x2){a[2], a[3]} * c02;
        const float sc[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
        for (int r = 0; r < 4; r++) h[r] = __builtin_amdgcn_fmed3f(a[r], sc[r], 3.4028234663852886e38f);
    };
    auto mlp_finish = [&](f32x4* acc) -> float4 {
        // hidden -> hidden layers: the lane's own 4 units of input tile mt are the B operand of k-step (mt, r); the accumulators of the MT output
        // tiles start at the bias and end in the same layout, so the layers chain in registers.  (The layer loop is NOT unrolled: unrolled, the
        // compiler hoists the second layer's A-operand reads over the first layer's MFMAs and spills 0.4 KB per lane at F 32 / hid 64.)
#pragma unroll 1
        for (int j = 0; j < NH; j++) {
            __builtin_amdgcn_sched_barrier(0);             // (same reason, for the single hidden layer of n_layers = 3: its reads stay behind layer 1)
            f32x4 nxt[MT];
#pragma unroll
            for (int mo = 0; mo < MT; mo++) nxt[mo] = *(const f32x4*)(bs + (j + 1) * HID + mo * 16 + 4 * q);
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                float h[4];
                lrelu4(acc[mt], h);
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int mo = 0; mo < MT; mo++)
                        nxt[mo] = __builtin_amdgcn_mfma_f32_16x16x4f32(ahs[(((j * MT + mo) * MT + mt) * 4 + r) * 64 + l], h[r], nxt[mo], 0, 0, 0);
            }
#pragma unroll
            for (int mo = 0; mo < MT; mo++) acc[mo] = nxt[mo];
        }
        // output layer (hid -> 4) as sixteen-block 4x4x1 MFMAs, exactly field.hip's
        f32x4 o4[2] = {o4init, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            float h[4];
            lrelu4(acc[mt], h);
#pragma unroll
            for (int r = 0; r < 4; r++) o4[r & 1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a1s[(mt * 4 + r) * 64 + l], h[r], o4[r & 1], 0, 0, 0);
        }
        const f32x2 s01 = (f32x2){o4[0][0], o4[0][1]} + (f32x2){o4[1][0], o4[1][1]}, s23 = (f32x2){o4[0][2], o4[0][3]} + (f32x2){o4[1][2], o4[1][3]};
        float o[4] = {s01.x, s01.y, s23.x, s23.y};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            o[c] += __shfl_xor(o[c], 16, 64);
            o[c] += __shfl_xor(o[c], 32, 64);
        }
        if (p.marcher == 1) {
#pragma unroll
            for (int c = 0; c < 3; c++) o[c] = (1.0f / (1.0f + expf(-o[c]))) * (1.f + 2.f * 0.001f) - 0.001f;
        }
        return make_float4(o[0], o[1], o[2], o[3]);
    };
    // every path runs blend_pass x NP, mlp_begin, mlp_pass x NP, mlp_finish in this order: results do not depend on the walk
    auto tile_from_taps = [&]() -> float4 {
        float g[NP][2 * PP];
#pragma unroll
        for (int ps = 0; ps < NP; ps++) blend_pass(tap, ps * PP, g[ps]);
        f32x4 acc[MT];
        mlp_begin(acc);
#pragma unroll
        for (int ps = 0; ps < NP; ps++) mlp_pass(acc, ps, g[ps]);
        return mlp_finish(acc);
    };

    if (p.ray_w > 0) {
        // image-coherent walk (field.hip, generic form): block = 8x8-pixel patch, wave = 4x4 quadrant, all S samples of its rays
        const int pX = (p.ray_w + PW - 1) / PW, pY = (p.ray_h + 7) / 8;
        const int npatch = (int)(p.total / p.P) * pX * pY;
        const int nb = gridDim.x, per = nb / 8;
        const int lb = (nb % 8 == 0) ? (blockIdx.x % 8) * per + blockIdx.x / 8 : blockIdx.x;
        const int wvi = threadIdx.x >> 6;
        float4* obuf = obuf_all + wvi * (16 * 9);
        auto ray_of = [&](int b, int py, int px, int tpt, bool& ok) {
            const int y = py * 8 + ((wvi >> 1) & 1) * 4 + (tpt >> 2), x = px * PW + (wvi & 1) * 4 + (tpt & 3);
            ok = y < p.ray_h && x < p.ray_w;
            return b * (int)p.R + (ok ? y * p.ray_w + x : 0);                   // B*R*S < 2^31 (checked on the host)
        };
        for (int patch = lb; patch < npatch; patch += nb) {
            const int px = patch % pX, py = (patch / pX) % pY, b = patch / (pX * pY);       // uniform
            bool gok;
            const int gray = ray_of(b, py, px, gpt, gok);      // the ray this lane gathers for
            bool fok;
            const int fray = ray_of(b, py, px, l >> 2, fok);   // the ray whose parked results this lane flushes
            const float ox = p.ray_o[gray * 3 + 0], oy = p.ray_o[gray * 3 + 1], oz = p.ray_o[gray * 3 + 2];
            const float dxr = p.ray_d[gray * 3 + 0], dyr = p.ray_d[gray * 3 + 1], dzr = p.ray_d[gray * 3 + 2];
            const float* bplanes = p.planes + (int64_t)b * 3 * plane_elems;
            const float* tp = p.t + (int64_t)gray * p.S;
            float tt = tp[0];
            float tn = p.S > 1 ? tp[1] : 0.f;
            issue_taps(ox + tt * dxr, oy + tt * dyr, oz + tt * dzr, bplanes, (int64_t)gray * p.S, gok);          // :141 (unfused mul, add)
            for (int k = 0; k < p.S; k++) {
                float g[NP][2 * PP];
#pragma unroll
                for (int ps = 0; ps < NP; ps++) blend_pass(tap, ps * PP, g[ps]);
                if (k + 1 < p.S) {                                  // taps of sample k+1 travel while the matrix cores run sample k
                    tt = tn;
                    tn = k + 2 < p.S ? tp[k + 2] : 0.f;
                    issue_taps(ox + tt * dxr, oy + tt * dyr, oz + tt * dzr, bplanes, (int64_t)gray * p.S + k + 1, gok);
                }
                f32x4 acc[MT];
                mlp_begin(acc);
#pragma unroll
                for (int ps = 0; ps < NP; ps++) mlp_pass(acc, ps, g[ps]);
                const float4 o = mlp_finish(acc);
                if (q == 0) obuf[pt * 9 + (k & 7)] = o;             // parked per wave [16 rays][8 samples], flushed as 128-B runs per ray
                if ((k & 7) == 7 || k + 1 == p.S) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const int k0 = k & ~7, nk = (k & 7) + 1;
                    const int fr = l >> 2, j = (l & 3) * 2;
                    float4 v0 = obuf[fr * 9 + j], v1 = obuf[fr * 9 + j + 1];
                    float4* dst = (float4*)p.rgbs + (int64_t)fray * p.S + k0 + j;
                    if (p.snoise && fok) {
                        const float* np = p.snoise + (int64_t)fray * p.S + k0 + j;
                        if (j < nk) v0.w = __fadd_rn(v0.w, __fmul_rn(np[0], p.snoise_std));
                        if (j + 1 < nk) v1.w = __fadd_rn(v1.w, __fmul_rn(np[1], p.snoise_std));
                    }
                    if (fok) {
                        if (j < nk) dst[0] = v0;
                        if (j + 1 < nk) dst[1] = v1;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        return;
    }
    const int64_t ntiles = (p.total + 15) / 16;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t tile = wave0; tile < ntiles; tile += nwaves) {
        const int64_t gp = tile * 16 + pt;                 // stored by this lane (MFMA layout)
        const bool valid = gp < p.total;
        const int64_t ggp = tile * 16 + gpt;               // gathered by this lane
        const bool gvalid = ggp < p.total;
        const int64_t gpc = gvalid ? ggp : p.total - 1;
        const int b = (int)(gpc / p.P);
        float cx, cy, cz;
        if (p.coords) {
            cx = p.coords[gpc * 3 + 0]; cy = p.coords[gpc * 3 + 1]; cz = p.coords[gpc * 3 + 2];
        } else {
            const int64_t ray = gpc / p.S;
            const float tt = p.t[gpc];
            cx = p.ray_o[ray * 3 + 0] + tt * p.ray_d[ray * 3 + 0];
            cy = p.ray_o[ray * 3 + 1] + tt * p.ray_d[ray * 3 + 1];
            cz = p.ray_o[ray * 3 + 2] + tt * p.ray_d[ray * 3 + 2];
        }
        issue_taps(cx, cy, cz, p.planes + (int64_t)b * 3 * plane_elems, ggp, gvalid);
        const float4 o = tile_from_taps();
        if (q == 0 && valid) {
            float4 on = o;
            if (p.snoise) on.w = __fadd_rn(on.w, __fmul_rn(p.snoise[gp], p.snoise_std));
            ((float4*)p.rgbs)[gp] = on;
        }
    }
}

template <int FQ, int MT, int NH, bool TAPS>
__global__ __launch_bounds__(256, 2) void triplane_field_deep_kernel(DeepParams p) { field_deep_body<FQ, MT, NH, TAPS>(p); }

template <int FQ, int MT, int NH, bool TAPS>
void launch_deep_t(const DeepParams& p, hipStream_t s) {
    int64_t want;
    if (p.ray_w > 0) want = (p.total / p.P) * cdiv(p.ray_w, 8) * cdiv(p.ray_h, 8);      // one 8x8-pixel patch per block
    else want = cdiv64((p.total + 15) / 16, 4);                                          // one 16-point tile per wave
    // persistent grid = the blocks the chip holds at once (LDS-limited), each striding over the work (field.hip: launch_field_t)
    static std::atomic<int> resident_pc;
    int per_cu = resident_pc.load(std::memory_order_relaxed);
    if (per_cu == 0) {
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, triplane_field_deep_kernel<FQ, MT, NH, TAPS>, 256, 0);
        if (e != hipSuccess || per_cu < 1) per_cu = 2;
        resident_pc.store(per_cu, std::memory_order_relaxed);
    }
    int blocks = (int)min((int64_t)per_cu * tdgp_cu_count(), want);
    if (blocks > 8) blocks -= blocks % 8;                    // whole rounds of the 8 XCDs (the in-kernel XCD remap needs it)
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
    TDGP_CHECK(coords || (ray_o && ray_d && t && S >= 1), TDGP_EINVAL, "triplane_field_deep: need coords, or ray_o/ray_d/t with S >= 1");
    TDGP_CHECK(B >= 0 && P >= 0 && H >= 2 && W >= 2, TDGP_EINVAL, "triplane_field_deep: bad shape");
    TDGP_CHECK(marcher == 0 || marcher == 1, TDGP_EINVAL, "triplane_field_deep: unknown ray marcher %d", marcher);
    TDGP_CHECK(coords || (P % S) == 0, TDGP_EINVAL, "triplane_field_deep: P must be a multiple of S in ray mode");
    TDGP_CHECK(!(density_noise > 0.f) || sigma_noise, TDGP_EINVAL, "triplane_field_deep: density_noise > 0 needs the sigma_noise draws");
    TDGP_FAULT_CHECK("triplane_field_deep");
    if (B == 0 || P == 0) return TDGP_OK;
    DeepParams p;
    p.planes = planes_hwc; p.coords = coords; p.ray_o = ray_o; p.ray_d = ray_d; p.t = t;
    for (int i = 0; i < DEEP_MAX_LAYERS; i++) { p.w[i] = i < n_layers ? w[i] : nullptr; p.b[i] = i < n_layers ? b[i] : nullptr; }
    p.rgbs = rgbs; p.tap_idx = tap_idx;
    p.snoise = density_noise > 0.f ? sigma_noise : nullptr; p.snoise_std = density_noise;
    p.total = (int64_t)B * P; p.P = P; p.S = coords ? 1 : S; p.H = H; p.W = W; p.scale = scale;
    { int ex; p.scale_is_pow2 = (frexpf(scale, &ex) == 0.5f) ? 1 : 0; p.inv_scale = 1.0f / scale; }
    TDGP_CHECK((int64_t)B * P <= INT32_MAX / 4 && (int64_t)3 * H * W * F <= INT32_MAX, TDGP_EINVAL, "triplane_field_deep: tensor too large");
    p.g0 = (float)(1.0 / sqrt((double)F)); p.gh = (float)(1.0 / sqrt((double)hid));    // weight_gain, layers.py:39
    p.marcher = marcher;
    p.R = coords ? 0 : P / S; p.ray_w = 0; p.ray_h = 0;
    if (!coords && ray_w > 0) {
        TDGP_CHECK((p.R % ray_w) == 0, TDGP_EINVAL, "triplane_field_deep: ray_w=%d does not divide the %lld rays", ray_w, (long long)p.R);
        p.ray_w = ray_w; p.ray_h = (int)(p.R / ray_w);
    }
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

typedef float fg_f32x16 __attribute__((ext_vector_type(16)));
constexpr int DG_PITCH = 33;

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
    float* Whs = W0s + HP * DG_PITCH;                         // [NH][HP][HPP]   w_j * gh
    float* Wls = Whs + NH * HP * HPP;                         // [4][HP]         w_last * gh
    float* Bs = Wls + 4 * HP;                                 // [NH + 1][HP]
    float* wave_mem = Bs + (NH + 1) * HP;
    const int tid = threadIdx.x, l = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), l32 = l & 31, half = l >> 5;
    constexpr int PANEL = HP * DG_PITCH;
    constexpr int WAVE_FLOATS = 32 * DG_PITCH + (NH + 2) * PANEL + 4 * 32;
    float* gl = wave_mem + wv * WAVE_FLOATS;                  // [32 pts][33]          features
    float* hl = gl + 32 * DG_PITCH;                           // [NH + 1][HP][33]      h_1 .. h_{NH+1}
    float* dl = hl + (NH + 1) * PANEL;                        // [HP][33]              dh_pre of the layer being walked back
    float* dol = dl + PANEL;                                  // [4][32]               do

    for (int i = tid; i < HP * DG_PITCH; i += NT) {
        const int m = i / DG_PITCH, f = i % DG_PITCH;
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
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto row_of = [&](int mt, int r) { return mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half; };      // accumulator row of the 32x32 tile

    const int64_t ntiles = (p.total + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * NW + wv; tile < ntiles; tile += (int64_t)gridDim.x * NW) {
        const int64_t gp = tile * 32 + l32;
        const bool valid = gp < p.total;
        const int64_t gpc = valid ? gp : 0;
        const int b = (int)(gpc / p.P);
        // ---- 1. geometry + gather (render_grad.hip, stage 1) ----------------------------------------------------------------
        const float* cp = p.coords + gpc * 3;
        const float q[3] = {cp[0] / p.scale, cp[1] / p.scale, cp[2] / p.scale};
        float tw_[3][4];
        int to_[3][4];
        float fr_[3][2];
        int in_[3];
        float gsum[16];
        float acc3[3][16];
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const float ix = (q[pl == 2 ? 1 : 0] + 1.0f) * sx, iy = (q[pl == 0 ? 1 : 2] + 1.0f) * sy;
            const float fx = floorf(ix), fy = floorf(iy);
            const float twx = ix - fx, te = 1.0f - twx, tn = iy - fy, ts = 1.0f - tn;
            const float cfx = fminf(fmaxf(fx, -2.f), (float)p.W), cfy = fminf(fmaxf(fy, -2.f), (float)p.H);
            const int x0 = (int)cfx, y0 = (int)cfy;
            const float wgt[4] = {ts * te, ts * twx, tn * te, tn * twx};
            const float* plane = p.planes + ((int64_t)b * 3 + pl) * p.H * p.W * p.F;
            fr_[pl][0] = twx; fr_[pl][1] = tn; in_[pl] = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int x = x0 + (t & 1), y = y0 + (t >> 1);
                const bool in = valid && x >= 0 && x < p.W && y >= 0 && y < p.H;
                tw_[pl][t] = in ? wgt[t] : 0.f;
                to_[pl][t] = in ? (y * p.W + x) * p.F : 0;
                in_[pl] |= in ? (1 << t) : 0;
            }
#pragma unroll
            for (int c = 0; c < 16; c++) acc3[pl][c] = 0.f;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const float* texel = plane + to_[pl][t] + half * fh;
#pragma unroll
                for (int c4 = 0; c4 < 4; c4++) {
                    if (4 * c4 < fh) {
                        const float4 v = *(const float4*)(texel + 4 * c4);
                        acc3[pl][4 * c4 + 0] += v.x * tw_[pl][t]; acc3[pl][4 * c4 + 1] += v.y * tw_[pl][t];
                        acc3[pl][4 * c4 + 2] += v.z * tw_[pl][t]; acc3[pl][4 * c4 + 3] += v.w * tw_[pl][t];
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 16; c++) gsum[c] = ((acc3[0][c] + acc3[1][c]) + acc3[2][c]) / 3.0f;
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if (c < fh) gl[l32 * DG_PITCH + half * fh + c] = gsum[c];
        }
        for (int f = p.F + half; f < 32; f += 2) gl[l32 * DG_PITCH + f] = 0.f;
        const float4 dout4 = valid ? *(const float4*)(p.d_out + gpc * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        wave_sync();

        // ---- 2. forward: h_1 = act(W0s g + b0), h_{j+1} = act(Whs_j h_j + b_j), every panel kept ------------------------------
        fg_f32x16 hacc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) hacc[mt][r] = Bs[row_of(mt, r)];
#pragma unroll
        for (int ks = 0; ks < 16; ks++) {
            const float bf = gl[l32 * DG_PITCH + 2 * ks + half];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) hacc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(W0s[(mt * 32 + l32) * DG_PITCH + 2 * ks + half], bf, hacc[mt], 0, 0, 0);
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
                    hj[row_of(mt, r) * DG_PITCH + l32] = h;
                }
            if (j == NH) break;
            wave_sync();
            const float* Wj = Whs + j * HP * HPP;
            fg_f32x16 nxt[MT];
#pragma unroll
            for (int mo = 0; mo < MT; mo++)
#pragma unroll
                for (int r = 0; r < 16; r++) nxt[mo][r] = Bs[(j + 1) * HP + row_of(mo, r)];
#pragma unroll 4
            for (int ks = 0; ks < HP / 2; ks++) {
                const int k = 2 * ks + half;                                      // input unit of this K step
                const float bf = hj[k * DG_PITCH + l32];                          // B[k][n = pt]
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
                dl[m * DG_PITCH + l32] = dhp;
            }
        wave_sync();
        // ---- 5. weight-gradient GEMMs over the 32 points, walking the layers back ------------------------------------------------
        {
            const float* hlast = hl + NH * PANEL;
#pragma unroll
            for (int ks = 0; ks < 16; ks++) {
                const int k = 2 * ks + half;                                          // point index of this K step
                const float bd = l32 < 4 ? dol[l32 * 32 + k] : 0.f;                   // B[k = pt][n = j]
#pragma unroll
                for (int mt = 0; mt < MT; mt++) dWla[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(hlast[(mt * 32 + l32) * DG_PITCH + k], bd, dWla[mt], 0, 0, 0);
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
                for (int mi = 0; mi < MT; mi++) bh[mi] = hj[(mi * 32 + l32) * DG_PITCH + k];        // B[k = pt][n = input unit]
#pragma unroll
                for (int mo = 0; mo < MT; mo++) {
                    const float ad = dl[(mo * 32 + l32) * DG_PITCH + k];                            // A[m = output unit][k = pt]
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
                const float bd = dl[k * DG_PITCH + l32];                              // B[k][n = pt]
#pragma unroll
                for (int mi = 0; mi < MT; mi++) dh[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(Wj[k * HPP + mi * 32 + l32], bd, dh[mi], 0, 0, 0);   // A[m = input unit][k]
            }
            wave_sync();                                                              // every lane has read the panel it is about to overwrite
#pragma unroll
            for (int mi = 0; mi < MT; mi++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int m = row_of(mi, r);
                    const float dhp = dh[mi][r] * sqrt2 * (hj[m * DG_PITCH + l32] > 0.f ? 1.0f : 0.2f);
                    dl[m * DG_PITCH + l32] = dhp;
                }
            wave_sync();
        }
#pragma unroll
        for (int ks = 0; ks < 16; ks++) {
            const int k = 2 * ks + half;
            const float bg = gl[k * DG_PITCH + l32];                                  // B[k = pt][n = f]
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const float ad = dl[(mt * 32 + l32) * DG_PITCH + k];
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
            dg = __builtin_amdgcn_mfma_f32_32x32x2f32(W0s[k * DG_PITCH + l32], dl[k * DG_PITCH + l32], dg, 0, 0, 0);   // A[m = f][k], B[k][n = pt]
        }
        // ---- 6. scatter: d_plane[tap] += w_tap * dg / 3 (render_grad.hip, stage 6) --------------------------------------------
        if (p.d_planes || p.d_coords) {
            wave_sync();
#pragma unroll
            for (int r = 0; r < 16; r++) gl[l32 * DG_PITCH + (r & 3) + 8 * (r >> 2) + 4 * half] = dg[r];
            wave_sync();
        }
        if (p.d_coords) {
            float dq[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
                const float* plane = p.planes + ((int64_t)b * 3 + pl) * p.H * p.W * p.F;
                const float twx = fr_[pl][0], tn = fr_[pl][1], te = 1.0f - twx, ts = 1.0f - tn;
                float gix = 0.f, giy = 0.f;
#pragma unroll
                for (int c4 = 0; c4 < 4; c4++) {
                    if (4 * c4 < fh) {
                        float4 tv[4];
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            tv[t] = *(const float4*)(plane + to_[pl][t] + half * fh + 4 * c4);
                            if (!((in_[pl] >> t) & 1)) tv[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                        }
                        const float* gq = gl + l32 * DG_PITCH + half * fh + 4 * c4;
                        const float gv[4] = {gq[0], gq[1], gq[2], gq[3]};
                        const float nw[4] = {tv[0].x, tv[0].y, tv[0].z, tv[0].w}, ne[4] = {tv[1].x, tv[1].y, tv[1].z, tv[1].w};
                        const float sw[4] = {tv[2].x, tv[2].y, tv[2].z, tv[2].w}, se[4] = {tv[3].x, tv[3].y, tv[3].z, tv[3].w};
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            gix = fmaf_(gv[i], (ne[i] - nw[i]) * ts + (se[i] - sw[i]) * tn, gix);
                            giy = fmaf_(gv[i], (sw[i] - nw[i]) * te + (se[i] - ne[i]) * twx, giy);
                        }
                    }
                }
                gix += __shfl_xor(gix, 32, 64);
                giy += __shfl_xor(giy, 32, 64);
                dq[pl == 2 ? 1 : 0] += gix * sx;
                dq[pl == 0 ? 1 : 2] += giy * sy;
            }
            if (half == 0 && valid) {
                const float k = 1.0f / (3.0f * p.scale);
                float* dc = p.d_coords + gpc * 3;
                dc[0] = dq[0] * k; dc[1] = dq[1] * k; dc[2] = dq[2] * k;
            }
        }
        if (p.d_planes) {
            int* tab_off = (int*)hl;                             // [32 pts][12 taps] float offset into d_planes (the h panels are dead now)
            float* tab_w = hl + 32 * 12;
#pragma unroll
            for (int pl = 0; pl < 3; pl++)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (((pl * 4 + t) & 1) == half) {
                        tab_off[l32 * 12 + pl * 4 + t] = (int)((((int64_t)b * 3 + pl) * p.H * p.W) * p.F) + to_[pl][t];
                        tab_w[l32 * 12 + pl * 4 + t] = tw_[pl][t] / 3.0f;
                    }
            wave_sync();
            for (int e2 = 0; e2 < 32 * 12 / 2; e2++) {
                const int e = 2 * e2 + half;                    // (point, tap) handled by this half-wave; lane = channel
                const float wt = tab_w[e];
                if (wt != 0.f && l32 < p.F) unsafeAtomicAdd(p.d_planes + tab_off[e] + l32, wt * gl[(e / 12) * DG_PITCH + l32]);
            }
        }
        wave_sync();
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
    const int wave_floats = 32 * DG_PITCH + (nh + 2) * HP * DG_PITCH + 4 * 32;
    const int lds_floats = HP * DG_PITCH + nh * HP * (HP + 1) + 4 * HP + (nh + 1) * HP + NW * wave_floats;
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

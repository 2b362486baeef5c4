// modconv_bf16.inc -- included by modconv.hip (inside its anonymous namespace).
//
// BASELINE configs[4]: the reference's reduced-precision blocks (networks_stylegan2.py:237 `dtype = float16 if use_fp16`, :50-53,
// conv_clamp 256; networks_epigraf.py:99-108 `num_fp16_res`) with bfloat16 in the place of float16: activations live in HBM as
// bf16 NCHW, weights as bf16, products run on v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate), accumulation, demodulation,
// noise, bias, activation and clamp in fp32, outputs rounded to bf16.  The skip image / tri-planes stay fp32, as in the reference
// (:268 `y.to(float32)`).
//
// Where the rounding happens.  The reference folds style and demodulation into per-sample weights and rounds THOSE to 16 bits
// (w.to(x.dtype), :81); here, as in the fp32 kernels, the style scales the activations while they are staged and the shared weights
// are rounded once at pack time, the demodulation coefficient multiplies the fp32 accumulator:
//     reference:  y = bf16( sum  bf16(W s d) * x )                      here:  y = bf16( d * sum  bf16(W) * bf16(x s) )
// -- the same number of 8-bit-mantissa roundings per product, at different places, so the two agree to bf16 rounding noise (a few
// 1e-3 of the tensor scale), not bit for bit; the oracle (oracle/, pinned by the reference's own bf16 run) follows the reference's
// points, and the parity tests state the bf16 tolerance.  After the accumulator the reference's points are kept: conv output ->
// bf16, + noise -> bf16, bias (itself rounded) / activation / gain / clamp -> bf16.
//
// Kernels (all block = 256 threads = 4 waves, K chunk = 32 channels = two 16-channel MFMA steps, one LDS stage per chunk, two
// blocks per CU so that one block's staging runs under the other's MFMAs):
//   conv3_bf16_kernel   3x3 stride 1, W % 32 == 0: the virtual-row scheme of conv3_mfma_kernel (zero row after every sample),
//                       block tile 64 channels x (8 rows x 32 columns).  A block stages the styles of TWO samples (b_lo, b_lo + 1): its
//                       8 + 2 virtual rows reach real rows of a third sample when H + 1 <= 7, so the host takes it for H >= 8 only;
//   upconv_bf16_kernel  the x2 layers: upconv_mfma_kernel's linearised-grid transposed convolution, same parity-planar fp32 Z,
//                       followed by fir_act_kernel<.., YBF> (FIR + demod + noise + bias + lrelu + clamp -> bf16);
//   ToRGB               torgb_mfma_kernel<.., XBF> (fp32 MFMA: the layer is HBM-bound; bf16 input halves its read traffic).
// Weight pack [chunk32][tap][sub-chunk][half][CoutP][8 bf16], LDS stages [..][half][column | position][8 bf16]: a lane's MFMA
// fragment (8 consecutive channels) is one 16-byte LDS read and the 16 lanes ds_read_b128 serves per cycle read 256 contiguous
// bytes -- conflict-free (with the two halves of a column side by side, 32-byte lane stride, every read was a 2-way bank conflict
// and the LDS, not the matrix pipe, was the busiest unit).

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ float round_bf16f(float v) { return (float)(__bf16)v; }
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    const split_b2 h = __builtin_convertvector((split_f2){a, b}, split_b2);
    uint32_t u;
    __builtin_memcpy(&u, &h, 4);
    return u;
}
__device__ __forceinline__ uint32_t buf_load_h(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
}

// weight [Cout,Cin,3,3] -> [chunk32][tap][sub][half][CoutP][8 bf16] (zero beyond Cout / Cin), as u32 words of two channels
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ w, uint32_t* __restrict__ wb, int Cout, int Cin, int CoutP, int nch32) {
    const int64_t total = (int64_t)nch32 * 9 * 2 * CoutP * 8;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int jp = (int)(i % 4);
        int64_t r = i / 4;
        const int col = (int)(r % CoutP); r /= CoutP;
        const int hf = (int)(r % 2); r /= 2;
        const int sub = (int)(r % 2); r /= 2;
        const int tap = (int)(r % 9);
        const int ch = (int)(r / 9);
        float v[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int c = ch * 32 + sub * 16 + hf * 8 + 2 * jp + q;
            v[q] = (col < Cout && c < Cin) ? w[((int64_t)col * Cin + c) * 9 + tap] : 0.f;
        }
        wb[i] = pack_bf16x2(v[0], v[1]);
    }
}

// fp32 -> bf16 / bf16 -> fp32 tensor casts (x.to(dtype) at the first reduced-precision block, networks_stylegan2.py:250)
__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, int64_t n) {
    for (int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 2; i < n; i += (int64_t)gridDim.x * blockDim.x * 2) {
        if (i + 1 < n) *(uint32_t*)(y + i) = pack_bf16x2(x[i], x[i + 1]);
        else y[i] = (uint16_t)(pack_bf16x2(x[i], 0.f) & 0xffffu);
    }
}

struct ConvBfParams {
    const uint16_t* x; const void* wb; const float* styles;
    EpiParams e;                  // e.y: fp32 output (YBF = false) -- or the bf16 output reinterpreted, see `y16`
    uint16_t* y16;
    int B, Cin, Cout, CoutP, H, W;
    uint32_t x_bytes, wb_bytes;
};

// Output stage of one 32(channels) x 32(pixels) tile parked channel-major in ct (row stride CT_LD): lane = (channel row l >> 3 of the
// pass, pixel quad l & 7), 4 consecutive x per lane -> one 8-byte bf16 store (or a 16-byte fp32 store).  The reference's rounding
// points after the accumulator: conv output, + noise, bias / activation / gain / clamp.
template <bool YBF, int ACT = 0>
__device__ __forceinline__ void epilogue_tile_bf16(const EpiParams& e, const SideCache& sc, uint16_t* y16, const float* ct, int obase, int pb, int poy, int pox,
                                                   int pok) {
    const int l = lane_id();
    const int g = l & 7, cr = l >> 3;
    const int b4 = __shfl(pb, 4 * g, 64), oy4 = __shfl(poy, 4 * g, 64), ox4 = __shfl(pox, 4 * g, 64), ok4 = __shfl(pok, 4 * g, 64);
    float4 nz = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e.noise && ok4) nz = *(const float4*)(e.noise + b4 * e.noise_bstride + (int64_t)oy4 * e.Wout + ox4);
    const int cstride = e.Hout * e.Wout;
    const int pix = (b4 * e.Cout * e.Hout + oy4) * e.Wout + ox4;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int row = pass * 8 + cr, o = obase + row;
        if (ok4 && o < e.Cout) {
            const float4 a = *(const float4*)&ct[row * CT_LD + 4 * g];
            const float d = side_demod(e, sc, b4, o, true), bb = side_bias(e, sc, o, true);
            float v[4] = {a.x * d, a.y * d, a.z * d, a.w * d};
            const float nq[4] = {nz.x, nz.y, nz.z, nz.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float t = v[i];
                if (YBF) t = round_bf16f(t);                       // conv2d output in bf16
                if (e.noise) { t = t + nq[i]; if (YBF) t = round_bf16f(t); }          // x.add_(noise) on the bf16 tensor
                v[i] = finish_act<ACT>(e, t + bb);
            }
            if (YBF) *(uint2*)(y16 + pix + o * cstride) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
            else *(float4*)(e.y + pix + o * cstride) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

template <bool YBF>
__global__ __launch_bounds__(256, 2) void conv3_bf16_kernel(ConvBfParams p) {
    constexpr int R = 1, MTW = 2, NTW = 2, WN = 4, BM = 64, NT = NTW * WN, PR = NT + 2, PC = 34, PSZ = PR * PC;
    constexpr int AS_BYTES = 9 * 2 * BM * 32, XS_BYTES = 2 * PSZ * 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* As = (char*)smem;                                           // [tap][sub][half][64 columns][8 bf16]
    char* Xs = As + AS_BYTES;                                         // [sub][half][position][8 bf16]
    float* side = (float*)(Xs + XS_BYTES);                          // [1 + NSB][BM]
    float* sty = side + (1 + 4) * BM;                               // [2][Cin]: the styles of the two samples a block can touch
    const int H1 = p.H + R;
    const int tilesX = p.W >> 5, VR = p.B * H1;
    const int ty = blockIdx.x / tilesX, tx = blockIdx.x % tilesX;
    const int vr0 = ty * NT, n0 = tx * 32, m0 = blockIdx.y * BM;
    const int tid = threadIdx.x, l = tid & 63, wv = TDGP_WAVE_INDEX(tid), l32 = l & 31, half = l >> 5;
    const int wn = wv;

    constexpr int NSB = 4;
    const int sb0 = vr0 / H1, sb1 = min(p.B - 1, (vr0 + NT - 1) / H1);
    const bool side_ok = (sb1 - sb0 + 1) <= NSB;
    if (side_ok) {
        for (int i = tid; i < (2 + sb1 - sb0) * BM; i += 256) {
            const int slab = i / BM, o = m0 + i % BM;
            float v = slab == 0 ? 0.f : 1.f;
            if (o < p.e.Cout) {
                if (slab == 0) { if (p.e.bias) v = YBF ? round_bf16f(p.e.bias[o]) : p.e.bias[o]; }          // self.bias.to(x.dtype), :144
                else if (p.e.dcoef) v = p.e.dcoef[(sb0 + slab - 1) * p.e.Cout + o];
            }
            side[i] = v;
        }
    }
    const int b_lo = max(vr0 - R, 0) / H1;
    for (int i = tid; i < 2 * p.Cin; i += 256) {
        const int sb = i >= p.Cin ? 1 : 0;
        sty[i] = p.styles ? p.styles[min(b_lo + sb, p.B - 1) * p.Cin + (i - sb * p.Cin)] : 1.f;
    }
    // staging items = (channel quarter of the 32-channel chunk, patch row, aligned PIXEL PAIR): activations are NCHW bf16, so two
    // horizontally adjacent pixels of one channel are one aligned 4-byte load -- 18 pair slots per 34-column patch row (the halo columns
    // are the odd halves of their pairs) instead of 34 two-byte loads: the vector-memory path processes a wave-wide load in the same
    // ~16 cycles whatever its width, and with 2-byte loads it, not the matrix pipe, set the pace of this kernel.
    constexpr int SLOTS = 18, NITEM = 4 * PR * SLOTS, NSLOT = (NITEM + 255) / 256;
    uint32_t it_xo[NSLOT], it_st[NSLOT];
    int it_lo[NSLOT], it_hi[NSLOT];             // LDS byte offsets of the pair's two pixels (-1: outside the patch)
#pragma unroll
    for (int k = 0; k < NSLOT; k++) {
        const int e = tid + k * 256, q4 = min(e / (PR * SLOTS), 3), rem = e - q4 * (PR * SLOTS), pr = rem / SLOTS, sl = rem - pr * SLOTS;
        it_xo[k] = kOOB; it_st[k] = (uint32_t)(8 * q4); it_lo[k] = -1; it_hi[k] = -1;
        if (e < NITEM) {
            const int pa = 2 * sl - 1, pb = 2 * sl;                 // pair s = image columns n0 - 2 + 2 s, + 1 = patch columns 2 s - 1, 2 s
            const int base = q4 * (PSZ * 16);                        // q4 = sub * 2 + half
            if (pa >= 0 && pa < PC) it_lo[k] = base + (pr * PC + pa) * 16;
            if (pb >= 0 && pb < PC) it_hi[k] = base + (pr * PC + pb) * 16;
            const int vi = vr0 - R + pr, ix = n0 - 2 + 2 * sl;
            if (vi >= 0 && ix >= 0 && ix < p.W) {
                const int b = vi / H1, m = vi - b * H1;
                if (b < p.B && m < p.H) {
                    it_xo[k] = (uint32_t)(((b * p.Cin + 8 * q4) * p.H + m) * p.W + ix) * 2u;
                    it_st[k] = (uint32_t)((b - b_lo) * p.Cin + 8 * q4);
                }
            }
        }
    }
    const uint32_t chw2 = (uint32_t)(p.H * p.W) * 2u;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes), rw = make_rsrc(p.wb, p.wb_bytes);

    f32x16 acc[MTW][NTW];
#pragma unroll
    for (int m = 0; m < MTW; m++)
#pragma unroll
        for (int n = 0; n < NTW; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

    const int niter = p.Cin >> 5;                                   // the host only takes this kernel with Cin % 32 == 0
    constexpr int NAV = 9 * 2 * BM * 2, NA = NAV / 256;             // 16-byte vectors of one chunk of weights: 9 per thread
    uint32_t a_vo[NA];
#pragma unroll
    for (int i = 0; i < NA; i++) {
        const int e = tid + i * 256;
        const int ts = e / (BM * 2), rem = e % (BM * 2), hf = rem / BM, col = rem % BM;
        a_vo[i] = (uint32_t)((ts * 2 + hf) * p.CoutP + min(m0 + col, p.CoutP - 1)) * 16u;      // (columns past CoutP: a duplicate, never stored)
    }
    const uint32_t a_gstride = (uint32_t)(9 * 2 * p.CoutP) * 32u;
    uint32_t x_reg[NSLOT][8];
    u32x4 a_reg[NA];
    auto load_stage = [&](int it) {
        const int itc = it;
        const uint32_t a_so = (uint32_t)itc * a_gstride, c0 = (uint32_t)itc * 32u;
#pragma unroll
        for (int i = 0; i < NA; i++) a_reg[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, a_vo[i], a_so, 0);
#pragma unroll
        for (int k = 0; k < NSLOT; k++)
#pragma unroll
            for (int j = 0; j < 8; j++) x_reg[k][j] = __builtin_amdgcn_raw_buffer_load_b32(rx, it_xo[k], (c0 + j) * chw2, 0);      // two pixels of channel c0 + j
    };
    auto store_stage = [&](int it) {
        const uint32_t c0 = (uint32_t)it * 32u;
#pragma unroll
        for (int i = 0; i < NA; i++) *(u32x4*)(As + (tid + i * 256) * 16) = a_reg[i];
#pragma unroll
        for (int k = 0; k < NSLOT; k++) {
            const float4 s0 = *(const float4*)&sty[it_st[k] + c0], s1 = *(const float4*)&sty[it_st[k] + c0 + 4];
            const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            uint32_t lo[4], hi[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                lo[j] = pack_bf16x2(bf16_bits_to_f32(x_reg[k][2 * j]) * sc[2 * j], bf16_bits_to_f32(x_reg[k][2 * j + 1]) * sc[2 * j + 1]);
                hi[j] = pack_bf16x2(__uint_as_float(x_reg[k][2 * j] & 0xffff0000u) * sc[2 * j], __uint_as_float(x_reg[k][2 * j + 1] & 0xffff0000u) * sc[2 * j + 1]);
            }
            if (it_lo[k] >= 0) *(uint4*)(Xs + it_lo[k]) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
            if (it_hi[k] >= 0) *(uint4*)(Xs + it_hi[k]) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        }
    };
    auto frag = [&](const char* ptr) { const uint4 v = *(const uint4*)ptr; bf16x8_t r; __builtin_memcpy(&r, &v, 16); return r; };
    const int a_lane = (half * BM + l32) * 16;                                       // + ((tap*2 + sub)*2*BM + m*32) * 16
    const int b_lane = (half * PSZ + (wn * NTW + R) * PC + l32 + R) * 16;           // centre tap of subtile 0; + (sub*2*PSZ + (n + dy)*PC + dx) * 16

    load_stage(0);
    for (int it = 0; it < niter; it++) {
        __syncthreads();                        // the previous chunk's fragments have been read
        store_stage(it);
        __syncthreads();
        if (it + 1 < niter) load_stage(it + 1); // in flight during this chunk's MFMAs
        // 18 (tap, sub-chunk) steps of 4 MFMAs (128 matrix-pipe cycles): the fragments of step s + 1 are read while step s multiplies --
        // left to itself the compiler reads, waits, multiplies (one LDS round trip per 128 cycles of work, and the pipe idles through it)
        bf16x8_t fa[2][MTW], fb[2][NTW];
        auto read_frags = [&](int step, int buf) {
            const int t = step >> 1, sub = step & 1, dy = t / 3 - R, dx = t % 3 - R;
#pragma unroll
            for (int m = 0; m < MTW; m++) fa[buf][m] = frag(As + a_lane + ((t * 2 + sub) * 2 * BM + m * 32) * 16);
#pragma unroll
            for (int n = 0; n < NTW; n++) fb[buf][n] = frag(Xs + b_lane + (sub * 2 * PSZ + (n + dy) * PC + dx) * 16);
        };
        read_frags(0, 0);
#pragma unroll
        for (int step = 0; step < 18; step++) {
            if (step + 1 < 18) read_frags(step + 1, (step + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < MTW; m++)
#pragma unroll
                for (int n = 0; n < NTW; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[step & 1][m], fb[step & 1][n], acc[m][n], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();                            // every wave is done with the stage buffers the tiles below overlay

    float* ct = smem + wv * (32 * CT_LD);
    SideCache scache;
    scache.lds = side_ok ? side : nullptr; scache.b0 = sb0; scache.bm = BM; scache.m0 = m0;
    const int evar = epi_variant(p.e);
#pragma unroll 1
    for (int tile = 0; tile < MTW * NTW; tile++) {
#pragma unroll
        for (int k = 0; k < MTW * NTW; k++) {
            if (tile == k) {
#pragma unroll
                for (int r = 0; r < 16; r++) ct[((r & 3) + 8 * (r >> 2) + 4 * half) * CT_LD + l32] = acc[k % MTW][k / MTW][r];
            }
        }
        const int m = tile % MTW, n = tile / MTW;
        const int vi = vr0 + wn * NTW + n;
        const int pb = vi / H1, poy = vi - pb * H1;
        const int pok = (vi < VR && poy < p.H) ? 1 : 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (evar == 4) epilogue_tile_bf16<YBF, 4>(p.e, scache, p.y16, ct, m0 + m * 32, pb, poy, n0 + l32, pok);       // lrelu + clamp 256: the reduced-precision blocks' form
        else epilogue_tile_bf16<YBF, 0>(p.e, scache, p.y16, ct, m0 + m * 32, pb, poy, n0 + l32, pok);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- x2 layers in bf16: upconv_mfma_kernel's linearised-grid transposed convolution on the bf16 MFMA, same fp32 Z ---------------
struct UpBfParams {
    const uint16_t* x; const void* wb; const float* styles; float* z;
    int B, Cin, Cout, CoutP, H, W, G1, GS;
    int64_t zslice;
    uint32_t x_bytes, wb_bytes, st_bytes;
};

__global__ __launch_bounds__(256, 2) void upconv_bf16_kernel(UpBfParams p) {
    constexpr int MTW = 2, BM = 64, BN = 128, XP = BN + 2;
    constexpr int AS_BYTES = 9 * 2 * BM * 32, XS_BYTES = 2 * 2 * XP * 32;                 // Xs: [sub][half][run][position][8 bf16]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* As = (char*)smem;
    char* Xs = As + AS_BYTES;
    const int v0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    const int tid = threadIdx.x, l = tid & 63, wv = TDGP_WAVE_INDEX(tid), l32 = l & 31, half = l >> 5;
    const int wn = wv;

    // the styles of the samples this block's grid points can touch, once, in LDS
    float* sty = (float*)(Xs + XS_BYTES);
    const int b_lo = max(v0 - 1 - p.G1, 0) / p.GS;
    const int nsb = min(p.B - 1, (v0 + BN) / p.GS) - b_lo + 1;
    for (int i = tid; i < nsb * p.Cin; i += 256) sty[i] = p.styles ? p.styles[b_lo * p.Cin + i] : 1.f;

    // staging items = (channel quarter, run, aligned PAIR of grid points): 4 x 2 x 65; run 0 = grid points v - G1 (dy = -1), run 1 =
    // dy = 0.  G1, GS and v0 are even, so a pair (even g, g + 1) is two horizontally adjacent pixels of one row -- one aligned 4-byte
    // load per channel (both inside the image or both in the zero margin, W being even) -- and position 0 of a run is the odd half of
    // pair 0.  (See conv3_bf16_kernel: 2-byte loads made the vector-memory path, not the matrix pipe, the limit.)
    constexpr int NRUN = BN + 1, NPAIR = BN / 2 + 1, NITEM = 4 * 2 * NPAIR, NSLOT = (NITEM + 255) / 256;
    uint32_t it_xo[NSLOT], it_st[NSLOT];
    int it_lo[NSLOT], it_hi[NSLOT];
#pragma unroll
    for (int k = 0; k < NSLOT; k++) {
        const int e = tid + k * 256;
        const int q4 = min(e / (2 * NPAIR), 3), rem = e - q4 * (2 * NPAIR), seg = rem / NPAIR, sl = rem - seg * NPAIR;
        it_xo[k] = kOOB; it_st[k] = (uint32_t)(8 * q4); it_lo[k] = -1; it_hi[k] = -1;
        if (e < NITEM) {
            const int base = (q4 * 2 + seg) * XP * 16;               // q4 = sub * 2 + half
            if (sl > 0) it_lo[k] = base + (2 * sl - 1) * 16;
            it_hi[k] = base + (2 * sl) * 16;
            const int g = v0 + 2 * sl - 2 - (seg == 0 ? p.G1 : 0);
            if (g >= 0) {
                const int b = g / p.GS, vp = g - b * p.GS;
                const int m = vp / p.G1, n = vp - m * p.G1;
                if (b < p.B && m < p.H && n < p.W) {
                    it_xo[k] = (uint32_t)(((b * p.Cin + 8 * q4) * p.H + m) * p.W + n) * 2u;
                    it_st[k] = (uint32_t)((b - b_lo) * p.Cin + 8 * q4);
                }
            }
        }
    }
    const uint32_t chw2 = (uint32_t)(p.H * p.W) * 2u;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes), rw = make_rsrc(p.wb, p.wb_bytes);

    f32x16 acc[4][MTW];                                               // [py*2+px][channel tile]
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int m = 0; m < MTW; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[q][m][r] = 0.f;

    const int niter = p.Cin >> 5;
    constexpr int NAV = 9 * 2 * BM * 2, NA = NAV / 256;
    uint32_t a_vo[NA];
#pragma unroll
    for (int i = 0; i < NA; i++) {
        const int e = tid + i * 256;
        const int ts = e / (BM * 2), rem = e % (BM * 2), hf = rem / BM, col = rem % BM;
        a_vo[i] = (uint32_t)((ts * 2 + hf) * p.CoutP + min(m0 + col, p.CoutP - 1)) * 16u;
    }
    const uint32_t a_gstride = (uint32_t)(9 * 2 * p.CoutP) * 32u;
    uint32_t x_reg[NSLOT][8];
    u32x4 a_reg[NA];
    auto load_stage = [&](int it) {
        const int itc = it;
        const uint32_t a_so = (uint32_t)itc * a_gstride, c0 = (uint32_t)itc * 32u;
#pragma unroll
        for (int i = 0; i < NA; i++) a_reg[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, a_vo[i], a_so, 0);
#pragma unroll
        for (int k = 0; k < NSLOT; k++)
#pragma unroll
            for (int j = 0; j < 8; j++) x_reg[k][j] = __builtin_amdgcn_raw_buffer_load_b32(rx, it_xo[k], (c0 + j) * chw2, 0);
    };
    auto store_stage = [&](int it) {
        const uint32_t c0 = (uint32_t)it * 32u;
#pragma unroll
        for (int i = 0; i < NA; i++) *(u32x4*)(As + (tid + i * 256) * 16) = a_reg[i];
#pragma unroll
        for (int k = 0; k < NSLOT; k++) {
            const float4 s0 = *(const float4*)&sty[it_st[k] + c0], s1 = *(const float4*)&sty[it_st[k] + c0 + 4];
            const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            uint32_t lo[4], hi[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                lo[j] = pack_bf16x2(bf16_bits_to_f32(x_reg[k][2 * j]) * sc[2 * j], bf16_bits_to_f32(x_reg[k][2 * j + 1]) * sc[2 * j + 1]);
                hi[j] = pack_bf16x2(__uint_as_float(x_reg[k][2 * j] & 0xffff0000u) * sc[2 * j], __uint_as_float(x_reg[k][2 * j + 1] & 0xffff0000u) * sc[2 * j + 1]);
            }
            if (it_lo[k] >= 0) *(uint4*)(Xs + it_lo[k]) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
            if (it_hi[k] >= 0) *(uint4*)(Xs + it_hi[k]) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        }
    };
    auto frag = [&](const char* ptr) { const uint4 v = *(const uint4*)ptr; bf16x8_t r; __builtin_memcpy(&r, &v, 16); return r; };
    const int a_lane = (half * BM + l32) * 16;                      // + ((tap*2 + sub)*2*BM + m*32) * 16
    const int x_lane = (half * 2 * XP + wn * 32 + l32) * 16;        // + (sub*4*XP + run*XP + dxi) * 16

    load_stage(0);
    for (int it = 0; it < niter; it++) {
        __syncthreads();                        // the previous chunk's fragments have been read (first pass: the styles are in LDS)
        store_stage(it);
        __syncthreads();
        if (it + 1 < niter) load_stage(it + 1); // in flight during this chunk's MFMAs
        // 18 (tap, sub-chunk) steps of 2 MFMAs; the fragments of the next step are read while this one multiplies (see conv3_bf16_kernel)
        bf16x8_t fa[2][MTW], fb[2];
        auto read_frags = [&](int step, int buf) {
            const int t = step >> 1, sub = step & 1, a = t / 3, e = t % 3;
            const int run = a == 2 ? 0 : 1, dxi = e == 2 ? 0 : 1;   // which shifted run the tap reads
            fb[buf] = frag(Xs + x_lane + (sub * 4 * XP + run * XP + dxi) * 16);
#pragma unroll
            for (int m = 0; m < MTW; m++) fa[buf][m] = frag(As + a_lane + ((t * 2 + sub) * 2 * BM + m * 32) * 16);
        };
        read_frags(0, 0);
#pragma unroll
        for (int step = 0; step < 18; step++) {
            if (step + 1 < 18) read_frags(step + 1, (step + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            const int t = step >> 1, a = t / 3, e = t % 3;
            const int q = (a & 1) * 2 + (e & 1);                    // output parity of this tap
#pragma unroll
            for (int m = 0; m < MTW; m++) acc[q][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[step & 1][m], fb[step & 1], acc[q][m], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();                                                // every wave is done with the stage buffers the tiles below overlay

    // ---- epilogue (as in upconv_mfma_kernel): interleave px = 0/1 through a per-wave LDS tile, 16-B buffer stores into Z ----
    float* ct = smem + wv * (32 * UP_CT_W);
    const bool zbuf = (uint64_t)p.zslice * 4u < 0xFFFF0000ull;
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(p.z, zbuf ? (uint32_t)(p.zslice * 4) : 0u);
    const int q4 = l & 15, cr = l >> 4;
    const uint32_t z_vo = (uint32_t)(cr * 4 * p.GS + 4 * q4) * 4u;
    const uint32_t z_pass = (uint32_t)(16 * p.GS) * 4u;
    const int gbase = v0 + wn * 32;
    const int b = gbase / p.GS, vp0 = gbase - b * p.GS;                // GS is a multiple of 32: the 32 points of a wave share their sample
#pragma unroll 1
    for (int tile = 0; tile < 2 * MTW; tile++) {
#pragma unroll
        for (int k = 0; k < 2 * MTW; k++) {
            if (tile == k) {
                const int py = k / MTW, mm = k % MTW;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                    *(float2*)&ct[row * UP_CT_W + 2 * l32] = make_float2(acc[py * 2][mm][r], acc[py * 2 + 1][mm][r]);
                }
            }
        }
        const int py = tile / MTW, mm = tile % MTW;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int obase = m0 + mm * 32;
        if (b < p.B) {
            if (zbuf && obase + 32 <= p.Cout) {
                const uint32_t zb = (uint32_t)(((b * p.Cout + obase) * 2 + py) * (2 * p.GS) + 2 * vp0) * 4u;
#pragma unroll
                for (int pass = 0; pass < 8; pass++) {
                    const float4 v = *(const float4*)&ct[(pass * 4 + cr) * UP_CT_W + 4 * q4];
                    const u32x4 bits = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                    __builtin_amdgcn_raw_buffer_store_b128(bits, rz, z_vo, zb + (uint32_t)pass * z_pass, 0);
                }
            } else {
#pragma unroll
                for (int pass = 0; pass < 8; pass++) {
                    const int ch = pass * 4 + cr, o = obase + ch;
                    if (o < p.Cout) {
                        const float4 v = *(const float4*)&ct[ch * UP_CT_W + 4 * q4];
                        *(float4*)(p.z + (((int64_t)b * p.Cout + o) * 2 + py) * (2 * p.GS) + 2 * vp0 + 4 * q4) = v;
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

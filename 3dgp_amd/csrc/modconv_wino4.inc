// modconv_wino4.inc -- included by modconv.hip (inside its anonymous namespace), after modconv_wino.inc.
//
// The stride-1 3x3 layers with many output channels (networks_stylegan2.py:31-88 -> conv2d_resample.py:127-134, padding 1) as Winograd
// F(4x4, 3x3) in fp32: y = A^T [ (G g G^T) . (B^T d B) ] A per 4x4 output tile -- 36 multiplies for 16 outputs where F(2x2, 3x3) takes 64
// and the direct sum 144.  Round 3 left conv3_wino_kernel (F(2x2)) at 0.54 of the fp32 MFMA peak with ~4.4 non-MFMA instructions per
// MFMA on a datapath the two share; re-scheduling did not move it.  This kernel removes instructions instead:
//
//   * interpolation points (0, 1, -1, 1/2, -2, inf) instead of the textbook (0, +-1, +-2, inf): the transforms lose the +- symmetry
//     (a few more fmas per 1-D transform) but the fp32 error drops 2.5x -- measured in fp32 emulation against the double sum on
//     lrelu-shaped activations: Cin = 512: 5.9e-6 of the output range (textbook points 1.6e-5, F(2x2) 1.0e-6, direct fp32 sum 2.5e-6);
//     Cin = 256: 3.7e-6; 128: 3.1e-6; 64: 2.2e-6 -- inside the 1e-5 bound of the reduction rows (tests/test_gpu_parity.py);
//   * the INPUT transform is a pass of its own (wino4_input_kernel: style-modulated x -> V, 2.25 x the input bytes, HBM-bound), so it
//     runs once per input instead of once per 64-channel slice of the output (8 x at Cout = 512), and the GEMM kernel below has NO vector
//     work in its loop at all: both operands arrive by LDS-direct buffer loads (no staging registers, no ds_write), fragments are
//     address-free ds_read_b128, 36 MFMAs per 4-channel chunk and wave;
//   * 36 independent GEMMs M_xi[cout][tile] = sum_cin U_xi[cout][cin] V_xi[cin][tile] on v_mfma_f32_16x16x4_f32: a wave owns ALL 36
//     positions of a 16-channel x 16-tile block (36 x 4 = 144 accumulators), so the whole output transform is register-local -- no LDS
//     exchange, no barrier in the output stage -- and a lane ends up with 4 channels x one 4x4-pixel tile, stored as 16-byte rows
//     (16 lanes = 64 consecutive pixels).
//
// Block shapes (BM = W4_BM output channels per slice; 32 since the barrier measurements of round 4):
//   * 4 waves, two blocks per CU: a slice x one tile group of 32 tiles (2 x 16 tiles = 8 x 64 pixels, or 4 x 8 tiles for the 32-pixel-wide layers); wave w
//     takes channel half w & 1 of tile half w >> 1.  Per 4-channel chunk the block needs U [9 position quads][4 k][32 channels][4] (18 432 B) and
//     V [9][4 k][32 tiles][4] (18 432 B), both contiguous in global memory in exactly this order (pack_wino4_kernel / wino4_input_kernel write them so):
//     36 wave-wide 1-KB LDS-direct loads per chunk, two stages of 36 864 B;
//   * PAIR (the form the launcher instantiates): 8 waves, one block per CU: a slice x a PAIR of tile groups sharing the U stages, V three stages
//     deep (see the kernel).
// A lane's operands of four positions are ONE ds_read_b128 (conflict-free: the 16-lane groups of a 16-byte read cover 16 distinct 16-byte bank slots);
// position PAIRS read as ds_read_b64 were merged by the compiler into ds_read2st64_b64, which runs at half the LDS rate.  Persistent blocks; items are
// drawn from per-XCD tickets in rectangles of rs channel slices x rt tile groups (rs rt = blocks per XCD) so that an XCD's L2 sees each U chunk rs times
// and each V chunk rt times per pass instead of once per block (sized in the launcher).

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Wino4Params {
    const float* v; const float* u;
    EpiParams e;
    int B, Cin, Cout, CoutP, H, W;
    uint32_t v_bytes, u_bytes;
    int gxn, gyn;                  // tile groups per row / column of a sample
    int txl;                       // log2 of the tiles per row of a group: 4 = 16 x 2 tiles (64 x 8 pixels), 3 = 8 x 4 tiles (32 x 16 pixels, the 32^2 layers)
    int rs, rt;                    // rectangle of an XCD: rs channel slices x rt tile groups (rs * rt = blocks per XCD)
    int nxcd;                      // blocks = nxcd * rs * rt
    int* ticket;                   // [nxcd] item counters in the workspace, zeroed by wino4_input_kernel (the launch before this one on the stream)
    int ups;                       // 1: the x2 layers -- channel 4 o + 2 py + px is output parity (py, px) of real channel o (see the output stage)
    int ksl;                       // log2 of the K splits: launches with too few items for the chip (batch 4 at 32^2) run every (slice, tile group) as 2^ksl items
    float* partial;                //   over consecutive ranges of the input channels, each writing its raw output-transformed sums to partial[split][B,Cout,H,W];
};                                 //   splitk_reduce_kernel adds them in split order and applies the epilogue (plain layers only)

// B^T of F(4x4, 3x3) at the points (0, 1, -1, 1/2, -2, inf), applied along one axis: t = B^T d
__device__ __forceinline__ void wino4_bt(const float (&d)[6], float (&t)[6]) {
    t[0] = fmaf_(1.5f, d[3] - d[1], fmaf_(-2.0f, d[2], d[0] + d[4]));
    t[1] = fmaf_(2.5f, d[3], fmaf_(0.5f, d[2], d[4] - d[1]));
    t[2] = fmaf_(-2.5f, d[2], fmaf_(0.5f, d[3], d[1] + d[4]));
    t[3] = fmaf_(2.0f, d[3] - d[1], d[4] - d[2]);
    t[4] = fmaf_(0.5f, d[1] - d[3], d[4] - d[2]);
    t[5] = fmaf_(1.5f, d[4] - d[2], fmaf_(-2.0f, d[3], d[1] + d[5]));
}
// A^T at the same points: y = A^T m (6 -> 4)
__device__ __forceinline__ void wino4_at(const float (&m)[6], float (&y)[4]) {
    const float s = m[1] + m[2], d = m[1] - m[2];
    y[0] = (m[0] + s) + (m[3] + m[4]);
    y[1] = fmaf_(-2.0f, m[4], fmaf_(0.5f, m[3], d));
    y[2] = fmaf_(4.0f, m[4], fmaf_(0.25f, m[3], s));
    y[3] = fmaf_(-8.0f, m[4], fmaf_(0.125f, m[3], d)) + m[5];
}

// The output stage in PACKED form (round 6).  An accumulator register quad acc[xi] holds position xi of FOUR consecutive channels (r = 0..3), so the natural
// two-wide SIMD axis of the output transform is a channel PAIR -- (acc[xi][0], acc[xi][1]) and (acc[xi][2], acc[xi][3]) are adjacent registers: the same
// fma chains as wino4_at, element by element (same bits), as v_pk_* on pairs with no register shuffling.  Why it matters: written per channel the compiler
// re-packed the scalar chains across COLUMNS with ~410 v_mov per item and wave (1500 vector instructions per item: a third of the 512^2 x 64 layer's
// time at 16 chunks per item, 18 % of the x2 layer's at 32); this form is ~520.
typedef float w4_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wino4_at2(const w4_f2 (&m)[6], w4_f2 (&y)[4]) {
    const w4_f2 s = m[1] + m[2], d = m[1] - m[2];
    y[0] = (m[0] + s) + (m[3] + m[4]);
    y[1] = __builtin_elementwise_fma((w4_f2){-2.0f, -2.0f}, m[4], __builtin_elementwise_fma((w4_f2){0.5f, 0.5f}, m[3], d));
    y[2] = __builtin_elementwise_fma((w4_f2){4.0f, 4.0f}, m[4], __builtin_elementwise_fma((w4_f2){0.25f, 0.25f}, m[3], s));
    y[3] = __builtin_elementwise_fma((w4_f2){-8.0f, -8.0f}, m[4], __builtin_elementwise_fma((w4_f2){0.125f, 0.125f}, m[3], d)) + m[5];
}
// Y = A^T M A of the channel pair (2 pr, 2 pr + 1) of a lane's 36 accumulator quads: yy[a][i] = output row a, pixel i, as (channel 2 pr, channel 2 pr + 1)
__device__ __forceinline__ void wino4_output_pair(const f32x4 (&acc)[36], int pr, w4_f2 (&yy)[4][4]) {
    w4_f2 t[4][6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        w4_f2 col[6];
#pragma unroll
        for (int i = 0; i < 6; i++) col[i] = pr == 0 ? (w4_f2){acc[6 * i + j][0], acc[6 * i + j][1]} : (w4_f2){acc[6 * i + j][2], acc[6 * i + j][3]};
        w4_f2 y4[4];
        wino4_at2(col, y4);
#pragma unroll
        for (int a = 0; a < 4; a++) t[a][j] = y4[a];
    }
#pragma unroll
    for (int a = 0; a < 4; a++) wino4_at2(t[a], yy[a]);
}
// (v * d + nz) + b -> activation -> * gain on a pair of values with their own d / b and a common noise value: finish_act4's arithmetic, element by element.
// ACT = 1 (linear) / 3 (leaky ReLU as max(v, alpha v), 0 <= alpha <= 1): the generator's two forms.
template <int ACT>
__device__ __forceinline__ w4_f2 finish_pair(const EpiParams& e, w4_f2 v, w4_f2 d2, float nz, w4_f2 b2) {
    static_assert(ACT == 1 || ACT == 3, "packed output stage: linear / leaky ReLU without clamp");
    w4_f2 x = (v * d2 + (w4_f2){nz, nz}) + b2;
    if constexpr (ACT == 3) {
        const w4_f2 xa = x * (w4_f2){e.alpha, e.alpha};
        x = (w4_f2){__builtin_fmaxf(x.x, xa.x), __builtin_fmaxf(x.y, xa.y)};
    }
    return x * (w4_f2){e.gain, e.gain};
}

constexpr int W4_MIN_C = 64;        // fewest input / output channels (below: the direct / F(2x2) kernels)
constexpr int W4_BM = 32;           // output channels per slice (measured: see the kernel)
constexpr int W4_NW = W4_BM / 8;    // waves per block of the 4-wave form = (BM / 16 channel groups) x 2 tile rows
constexpr int W4_UCH = 9 * 4 * W4_BM * 4, W4_VCH = 9 * 4 * 32 * 4;     // floats per chunk
constexpr int W4_UP = W4_UCH / 256;                                     // 1-KB pieces of U
constexpr int W4_NPW = (W4_UP + 18) / W4_NW;                            // pieces per wave and chunk (9)
constexpr int W4_STAGE = W4_UCH + W4_VCH;
static_assert((W4_UP + 18) % W4_NW == 0, "wino4: piece count");

// weight [Cout,Cin,3,3] -> U [slice][chunk][xi4 9][k 4][cp BM][4]: U_xi = (G g G^T)[i][j], xi = 6 i + j = 4 xi4 + e, channel = 4 chunk + k,
// out-channel = BM slice + cp; zero beyond Cout / Cin.  Computed in double, rounded once.
__global__ __launch_bounds__(256) void pack_wino4_kernel(const float* __restrict__ w, float* __restrict__ u, int Cout, int Cin, int nslice, int nch4) {
    const int64_t total = (int64_t)nslice * nch4 * W4_UCH;
    const double G[6][3] = {{1.0, 0.0, 0.0}, {1.0 / 3, 1.0 / 3, 1.0 / 3}, {-1.0 / 3, 1.0 / 3, -1.0 / 3}, {-16.0 / 15, -8.0 / 15, -4.0 / 15},
                            {1.0 / 15, -2.0 / 15, 4.0 / 15}, {0.0, 0.0, 1.0}};
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 3), cp = (int)(idx >> 2) % W4_BM, k = (int)((idx >> 2) / W4_BM) & 3;
        int64_t r = idx / (16 * W4_BM);
        const int xi4 = (int)(r % 9); r /= 9;
        const int ch = (int)(r % nch4), sl = (int)(r / nch4);
        const int o = sl * W4_BM + cp, c = ch * 4 + k, xi = 4 * xi4 + e, i = xi / 6, j = xi % 6;
        double v = 0.0;
        if (o < Cout && c < Cin) {
            const float* g = w + ((int64_t)o * Cin + c) * 9;
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) v += G[i][a] * (double)g[a * 3 + b] * G[j][b];
        }
        u[idx] = (float)v;
    }
}

// x [B,Cin,H,W] (x style[b,cin]) -> V [tile group][chunk][xi4 9][k 4][tile 32][4], V_xi = (B^T d B)[i][j] of the 6x6 window of tile t
// (rows 4 ty - 1 .. 4 ty + 4 of its group, zero outside the image).  One block = one (tile group, chunk): thread = (k, tile); its 9 float4
// stores are 512 contiguous bytes per 32 threads.
__global__ __launch_bounds__(128) void wino4_input_kernel(const float* __restrict__ x, const float* __restrict__ styles, float* __restrict__ v, int B, int Cin,
                                                          int H, int W, int gxn, int gyn, int nch4, int txl, int* __restrict__ ticket) {
    if (blockIdx.x == 0 && threadIdx.x < 8) ticket[threadIdx.x] = 0;          // the GEMM kernel's item counters (one per XCD)
    const int k = threadIdx.x >> 5, t = threadIdx.x & 31, tx = t & ((1 << txl) - 1), ty = t >> txl;
    const int64_t blk = blockIdx.x;
    const int ch = (int)(blk % nch4);
    const int tg = (int)(blk / nch4);
    const int gx = tg % gxn, gy = (tg / gxn) % gyn, b = tg / (gxn * gyn);
    const int c = ch * 4 + k;
    const bool cok = c < Cin;
    const float s = (styles && cok) ? styles[b * Cin + c] : 1.0f;
    const int y0 = gy * (128 >> txl) + ty * 4 - 1, x0 = gx * (4 << txl) + tx * 4;      // window columns x0 - 1 .. x0 + 4
    const float* xp = x + ((int64_t)b * Cin + (cok ? c : 0)) * H * W;
    float d[6][6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        const int yy = y0 + r;
        const bool rok = cok && yy >= 0 && yy < H;
        const float* row = xp + (int64_t)(rok ? yy : 0) * W + x0;
        const float4 mid = rok ? *(const float4*)row : make_float4(0.f, 0.f, 0.f, 0.f);
        const float lft = (rok && x0 > 0) ? row[-1] : 0.f, rgt = (rok && x0 + 4 < W) ? row[4] : 0.f;
        d[r][0] = lft * s; d[r][1] = mid.x * s; d[r][2] = mid.y * s; d[r][3] = mid.z * s; d[r][4] = mid.w * s; d[r][5] = rgt * s;
    }
    float tmp[6][6];                                                                  // tmp = B^T d  (along rows)
#pragma unroll
    for (int cc = 0; cc < 6; cc++) {
        const float col[6] = {d[0][cc], d[1][cc], d[2][cc], d[3][cc], d[4][cc], d[5][cc]};
        float o[6];
        wino4_bt(col, o);
#pragma unroll
        for (int i = 0; i < 6; i++) tmp[i][cc] = o[i];
    }
    float vv[36];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        float o[6];
        wino4_bt(tmp[i], o);                                                          // V[i][.] = tmp[i][.] B
#pragma unroll
        for (int j = 0; j < 6; j++) vv[i * 6 + j] = o[j];
    }
    float* dst = v + (blk * (int64_t)W4_VCH) + (k * 32 + t) * 4;
#pragma unroll
    for (int q = 0; q < 9; q++) *(float4*)(dst + q * (4 * 32 * 4)) = make_float4(vv[4 * q], vv[4 * q + 1], vv[4 * q + 2], vv[4 * q + 3]);
}

// PAIR (BM = 32): one 8-wave block per CU takes a slice x a PAIR of neighbouring tile groups -- waves 0..3 the first, 4..7 the second -- sharing the
// U stages (a quarter fewer operand bytes per MFMA) and, with the LDS that frees, THREE stages of V: the V pieces of chunk c + 2 travel while chunk c is
// multiplied.  Why: an LDS-direct load takes about as long as a chunk lasts (SQ level counters), U always hits the L2, V is first touched by this item
// (tools/dev/ubench_ldsdma3.hip: a second chunk of look-ahead for V is worth 12-15 % when V comes from beyond the L2).  LDS: U [2][4608] floats,
// V [3][2 tile groups][4608], side: bias [BM], demodulation [2][BM], the ticket.  The waits count on LDS-direct loads completing in issue order.
template <bool UPS, bool PAIR = false>
__global__ __launch_bounds__(PAIR ? 512 : W4_NW * 64, PAIR ? 1 : 2) void conv3_wino4_kernel(Wino4Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const uint32_t lds0 = TDGP_LDS_BASE(smem);
    float* side = smem + (PAIR ? 8 * W4_UCH : 2 * W4_STAGE);     // [0..BM) bias, [BM..2 BM) demodulation coefficients (PAIR: [BM .. 3 BM): one set per tile group)
    const int tid = threadIdx.x, l = tid & 63, wvx = TDGP_WAVE_INDEX(tid), hsel = PAIR ? wvx >> 2 : 0, wv = PAIR ? (wvx & 3) : wvx;
    const int cg = wv % (W4_BM / 16), tr = wv / (W4_BM / 16), l15 = l & 15, kq = l >> 4;
    const int nch = (p.Cin + 3) >> 2;
    const int ntg1 = p.gxn * p.gyn * p.B, ntg = PAIR ? (ntg1 + 1) >> 1 : ntg1;                // (PAIR: an item's `tg` is a pair of tile groups 2 tg, 2 tg + 1)
    const int nsl = ((p.Cout + W4_BM - 1) / W4_BM) << p.ksl;         // (slice, K split) pairs count as slices: sl = slice << ksl | split
    const int nchk = nch >> p.ksl;                  // chunks per item
    // Rectangles of rs channel slices x rt tile groups, numbered R = 0 .. nrect - 1 = (slice block R % RS, tile-group block R / RS); XCD x works
    // through R = x, x + nxcd, ...  Blocks b, b + nxcd, ... share an XCD (dispatch is round-robin over the XCDs: a locality hint, not a contract).
    const int xcd = (int)blockIdx.x % p.nxcd;
    const int RS = (nsl + p.rs - 1) / p.rs, RT = (ntg + p.rt - 1) / p.rt, nrect = RS * RT;
    const uint32_t lane16 = (uint32_t)l * 16u;
    uint32_t u_base = 0, v_base = 0;                // byte offsets of the item's first chunk
    // LDS-direct loads are issued by hand: the compiler answers the builtin form with an `s_waitcnt vmcnt(0)` in front of the next ds_read
    // (it cannot tell which LDS bytes a load in flight will write), i.e. it would wait for chunk c + 1 before multiplying chunk c.  M0 (the
    // LDS destination base) is written in the statement that uses it.  It cannot be declared clobbered (hipcc rejects reserved registers on a clobber
    // list); instead the build checks the ISA of every conv3_wino4_kernel instantiation (3dgp_amd/isa_check.py:check_wino4_asm): m0 is written only by
    // these statements and read by nothing but the LDS-direct load that follows, the PAIR loop holds no other vector-memory instruction before its
    // hand-counted `vmcnt(4)`, and exactly the expected number of LDS-direct loads.
    typedef unsigned int w4_u32x4 __attribute__((ext_vector_type(4)));
    auto desc = [](const void* ptr, uint32_t bytes) {
        const uint64_t a = (uint64_t)(uintptr_t)ptr;
        return (w4_u32x4){(uint32_t)a, (uint32_t)((a >> 32) & 0xffffu), bytes, 0x00020000u};
    };
    const w4_u32x4 du = desc(p.u, p.u_bytes), dv = desc(p.v, p.v_bytes);
    // M0 (the LDS destination base) is written in the statement that uses it; nothing else in this kernel uses M0
    auto dma = [&](const w4_u32x4& d, uint32_t lds_dst, uint32_t voff, uint32_t soff) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(lds_dst), "v"(voff), "s"(d), "s"(soff) : "memory");
    };
    // the pieces of a chunk (18 of U + 18 of V): wave w issues pieces
    // q = w + NW i.  Pieces i <= 3 are U, i >= 5 are V, i = 4 is U for the first half of the waves and V for the second: the descriptor / chunk
    // offset of that one are selected once.
    uint32_t pv[W4_NPW];                            // per-lane global offsets inside the chunk
#pragma unroll
    for (int i = 0; i < W4_NPW; i++) {
        const int q = wv + W4_NW * i;
        pv[i] = lane16 + (uint32_t)(q < W4_UP ? q : min(q - W4_UP, 17)) * 1024u;
    }
    const bool p4u = wv < W4_NW / 2;
    const w4_u32x4 d4 = p4u ? du : dv;
    uint32_t uo = 0, vo = 0;                        // chunk offsets of the loads being issued (wave-uniform)
    auto piece = [&](int i, uint32_t stage_lds) {   // i is a compile-time constant at every call site
        const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)(stage_lds + (uint32_t)(wv + W4_NW * i) * 1024u));
        if (i <= 3) dma(du, dst, pv[i], uo);
        else if (i == 4) dma(d4, dst, pv[i], p4u ? uo : vo);
        else dma(dv, dst, pv[i], vo);
    };
    auto set_chunk = [&](int c) {
        uo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(u_base + (uint32_t)c * (W4_UCH * 4u)));
        vo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v_base + (uint32_t)c * (W4_VCH * 4u)));
    };
    auto issue = [&](int c, int buf) {              // a whole chunk at once (an item's first chunk)
        set_chunk(c);
        const uint32_t dst = lds0 + (uint32_t)buf * (W4_STAGE * 4u);
#pragma unroll
        for (int i = 0; i < W4_NPW; i++) piece(i, dst);
    };
    auto wait_loads = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };        // this wave's LDS-direct loads have landed
    // fragment addresses: A: U[xi4][k = kq][16 cg + l15][e];  B: V[xi4][kq][16 tr + l15][e]
    const int a_lane = (kq * W4_BM + cg * 16 + l15) * 4;
    const int b_lane = (PAIR ? 0 : W4_UCH) + (kq * 32 + tr * 16 + l15) * 4;
    // PAIR: pieces of a chunk -- U: q = wvx + 8 i < 18 (i = 2: waves 0, 1 only); V of both tile groups: q = wvx + 8 i < 36, tile group q / 18 (i = 2: waves 0, 1
    // finish the first group, the others start the second; i = 4: waves 0 .. 3 only)
    uint32_t v_base1 = 0, vo1 = 0;                  // the second tile group's V
    auto pairU = [&](int i, uint32_t ust_lds) {
        const int q = wvx + 8 * i;
        dma(du, (uint32_t)__builtin_amdgcn_readfirstlane((int)(ust_lds + (uint32_t)q * 1024u)), lane16 + (uint32_t)q * 1024u, uo);
    };
    auto pairV = [&](int i, uint32_t vst_lds) {       // vst_lds: LDS byte address of V stage s (both tile groups: 2 x W4_VCH floats)
        const int q = wvx + 8 * i;
        const bool second = i > 2 || (i == 2 && wvx >= 2);
        const int pc = second ? q - 18 : q;
        dma(dv, (uint32_t)__builtin_amdgcn_readfirstlane((int)(vst_lds + (second ? (uint32_t)(W4_VCH * 4) : 0u) + (uint32_t)pc * 1024u)), lane16 + (uint32_t)pc * 1024u, second ? vo1 : vo);
    };
    auto pair_offsets = [&](int cu, int cv) {       // chunk whose U / whose V the next pieces fetch
        uo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(u_base + (uint32_t)cu * (W4_UCH * 4u)));
        vo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v_base + (uint32_t)cv * (W4_VCH * 4u)));
        vo1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v_base1 + (uint32_t)cv * (W4_VCH * 4u)));
    };
    const uint32_t ldsU = lds0, ldsV = lds0 + 2u * (W4_UCH * 4u);
    auto pair_first = [&](int nck) {                // an item's first chunks at once: U(0), V(0), V(1)
        pair_offsets(0, 0);
#pragma unroll
        for (int i = 0; i < 3; i++) if (i < 2 || wvx < 2) pairU(i, ldsU);
#pragma unroll
        for (int i = 0; i < 5; i++) if (i < 4 || wvx < 4) pairV(i, ldsV);
        pair_offsets(nck > 1 ? 1 : 0, nck > 1 ? 1 : 0);
#pragma unroll
        for (int i = 0; i < 5; i++) if (i < 4 || wvx < 4) pairV(i, ldsV + 2u * (W4_VCH * 4u));
    };

    // Items are DRAWN, not dealt: a block takes the next ticket of its XCD's counter (ticket t -> rectangle t / per of that XCD, slot t % per
    // inside it), so the rectangle order that keeps an XCD's L2 on few U slices / V tile groups survives, and a grid that is only partly
    // resident -- another kernel on a second stream, another process -- still finishes in the time of the work it has (dealt statically, the
    // blocks that start late are the makespan: the ToRGB layers on a side stream cost 6 % next to the static grid).  The next ticket is drawn
    // at the START of an item into a register (its latency hides under the first chunk) and published to the block after the K loop.
    int* const tk = (int*)(side + (PAIR ? 3 : 2) * W4_BM);
    const int per = p.rs * p.rt;
    auto from_ticket = [&](int t, int& sl, int& tg) {     // 1: an item, 0: an empty slot of a ragged rectangle, -1: past the end
        const int R = (t / per) * p.nxcd + xcd, j = t % per;
        if (R >= nrect) return -1;
        sl = (R % RS) * p.rs + j % p.rs;
        tg = (R / RS) * p.rt + j / p.rs;
        return (sl < nsl && tg < ntg) ? 1 : 0;
    };
    auto acquire = [&](int t_have, bool have_t, int& sl, int& tg) {      // block-uniform: publish / draw tickets until an item or the end
        for (;;) {
            if (tid == 0) tk[0] = have_t ? t_have : atomicAdd(p.ticket + xcd, 1);
            lds_barrier();
            const int t = tk[0];
            lds_barrier();                            // everybody has read it before the next one overwrites it
            const int st = from_ticket(t, sl, tg);
            if (st != 0) return st > 0;
            have_t = false;
        }
    };
    int sl = 0, tg = 0;
    bool have = acquire(0, false, sl, tg);
    auto set_bases = [&](int sl_, int tg_) {         // first chunk of item (sl_, tg_): split ks of slice sl_ >> ksl starts at chunk ks * nchk
        const uint32_t c0 = (uint32_t)(sl_ & ((1 << p.ksl) - 1)) * (uint32_t)nchk;
        u_base = ((uint32_t)(sl_ >> p.ksl) * (uint32_t)nch + c0) * (W4_UCH * 4u);
        v_base = ((uint32_t)(PAIR ? 2 * tg_ : tg_) * (uint32_t)nch + c0) * (W4_VCH * 4u);
        if (PAIR) v_base1 = ((uint32_t)min(2 * tg_ + 1, ntg1 - 1) * (uint32_t)nch + c0) * (W4_VCH * 4u);      // (an odd count: the last pair's second group re-reads the first)
    };
    if (have) {
        set_bases(sl, tg);
        if (PAIR) pair_first(nchk); else issue(0, 0);
    }
    while (have) {
        const int tgw = PAIR ? min(2 * tg + hsel, ntg1 - 1) : tg;     // this wave's tile group
        const bool tg_ok = !PAIR || 2 * tg + hsel < ntg1;
        const int m0 = (sl >> p.ksl) * W4_BM, gx = tgw % p.gxn, gy = (tgw / p.gxn) % p.gyn, b = tgw / (p.gxn * p.gyn);
        int t_next = 0;
        if (tid == 0) t_next = atomicAdd(p.ticket + xcd, 1);          // consumed after the K loop
        if (tid < (PAIR ? 3 : 2) * W4_BM) {
            const int o = m0 + (tid % W4_BM), hh = tid / W4_BM;       // hh = 0: bias; 1 (, 2): demodulation of the (first, second) tile group's sample
            float vv = hh == 0 ? 0.f : 1.f;
            if (o < p.Cout) {
                if (hh == 0) { if (p.e.bias) vv = p.e.bias[o]; }
                else if (p.e.dcoef) vv = p.e.dcoef[((PAIR ? min(2 * tg + hh - 1, ntg1 - 1) : tg) / (p.gxn * p.gyn)) * p.e.Cout + o];
            }
            side[tid] = vv;
        }
        f32x4 acc[36];
#pragma unroll
        for (int i = 0; i < 36; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        wait_loads();
        lds_barrier();
        if constexpr (PAIR) {
            // Round 6 asked whether the 0.3 k cycles a chunk takes beyond its 2.30 k of MFMAs (cycle counters) are the LDS round trip of the next chunk's first fragments behind
            // the barrier.  Three A/B forms ran the fragment pipeline THROUGH the chunk boundary: the wait + barrier stand in front of group 7 (2) or 8 (1) -- the
            // chunk's last fragments are in registers by then, nobody reads its stages any more -- and the groups behind it prefetch groups 0, 1 of the next chunk under their
            // own MFMAs; the wait's arithmetic is unchanged (4 V pieces of groups 3..6 may fly).  Measured (x2 and plain layers of C3, interleaved A/B): form 2 is 3-5 % SLOWER
            // -- the U pieces requested at groups 0..2 have not landed by group 7: a chunk is about as long as an LDS-direct load takes --, form 1 +1 %; form 3 (form 2 with
            // the U pieces of chunk c + 2 requested BEHIND chunk c's barrier into the stage it has just released, so that they have a whole chunk again) is level with the
            // shipped form (-1 % on the plain layers, inside the noise on the x2 ones).  So the round trip behind the barrier is not what the 0.3 k are; the shipped form stays.
            int vs = 0;                                  // V stage of the chunk being multiplied (c % 3)
            float4 fa[3], fb[3];
            auto frags_at = [&](const float* ust_, const float* vst_, int g, int q) {
                fa[q] = *(const float4*)(ust_ + g * (16 * W4_BM) + a_lane);
                fb[q] = *(const float4*)(vst_ + g * 512 + b_lane);
            };
            for (int c = 0; c < nchk; c++) {
                const float* ust = smem + (c & 1) * W4_UCH;
                const float* vst = smem + 2 * W4_UCH + (vs * 2 + hsel) * W4_VCH;
                const uint32_t nus = ldsU + (uint32_t)((c + 1) & 1) * (W4_UCH * 4u);
                const int vs1 = vs == 2 ? 0 : vs + 1;     // (c + 1) % 3
                const int vs2 = vs == 0 ? 2 : vs - 1;     // (c + 2) % 3
                const uint32_t nvs = ldsV + (uint32_t)vs2 * (2u * W4_VCH * 4u);
                pair_offsets(c + 1 < nchk ? c + 1 : c, c + 2 < nchk ? c + 2 : nchk - 1);
                frags_at(ust, vst, 0, 0);
                frags_at(ust, vst, 1, 1);
#pragma unroll
                for (int g = 0; g < 9; g++) {
                    if (g + 2 < 9) frags_at(ust, vst, g + 2, (g + 2) % 3);
                    __builtin_amdgcn_sched_barrier(0);
                    const float4 a = fa[g % 3], bb = fb[g % 3];
                    acc[4 * g + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bb.x, acc[4 * g + 0], 0, 0, 0);
                    acc[4 * g + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bb.y, acc[4 * g + 1], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // U of the next chunk first, then V of the chunk after: the wait lets exactly the V pieces fly
                    if (g < 2 || (g == 2 && wvx < 2)) pairU(g, nus);
                    if (g >= 3 && (g < 7 || (g == 7 && wvx < 4))) pairV(g - 3, nvs);
                    __builtin_amdgcn_sched_barrier(0);
                    acc[4 * g + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bb.z, acc[4 * g + 2], 0, 0, 0);
                    acc[4 * g + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bb.w, acc[4 * g + 3], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // U(c + 1) and the older V(c + 1) have landed; the four (five: then one more) V(c + 2) pieces may be in flight
                lds_barrier();
                vs = vs1;
            }
            wait_loads();
            lds_barrier();
        } else
        for (int c = 0; c < nchk; c++) {
            // Chunk c + 1 goes to the other stage (every wave finished reading it before the barrier that ended iteration c - 1).  Its 7 loads
            // are issued ONE AT A TIME in the shadow of this chunk's MFMAs (a wave issues ~5 scalar / memory instructions for free behind a
            // 32-cycle MFMA): issued in a burst at the top of the iteration -- both waves of a SIMD at once -- they cost 0.19 of 0.82 ms on the
            // 64^2 x 512 layer.  The last iteration re-requests its own chunk (no branch in the loop; nobody reads that stage again).
            const float* st = smem + (c & 1) * W4_STAGE;
            const uint32_t nst = lds0 + (uint32_t)((c + 1) & 1) * (W4_STAGE * 4u);
            set_chunk(c + 1 < nchk ? c + 1 : c);
            {
                // 9 groups of four positions (two 16-byte reads, 4 MFMAs); the fragments of group g + 2 are requested before the MFMAs of group g
                float4 fa[3], fb[3];
                auto frags = [&](int g, int q) {
                    fa[q] = *(const float4*)(st + g * (16 * W4_BM) + a_lane);
                    fb[q] = *(const float4*)(st + g * 512 + b_lane);
                };
                frags(0, 0);
                frags(1, 1);
#pragma unroll
                for (int g = 0; g < 9; g++) {
                    if (g + 2 < 9) frags(g + 2, (g + 2) % 3);
                    __builtin_amdgcn_sched_barrier(0);
                    const float4 a = fa[g % 3], bb = fb[g % 3];
                    acc[4 * g + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bb.x, acc[4 * g + 0], 0, 0, 0);
                    acc[4 * g + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bb.y, acc[4 * g + 1], 0, 0, 0);
                    if (g < W4_NPW) { __builtin_amdgcn_sched_barrier(0); piece(g, nst); __builtin_amdgcn_sched_barrier(0); }
                    acc[4 * g + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bb.z, acc[4 * g + 2], 0, 0, 0);
                    acc[4 * g + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bb.w, acc[4 * g + 3], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            wait_loads();
            lds_barrier();
        }
        // the next item's first chunk travels under the output stage (both stages are free: the loop ended on a barrier)
        // The item's noise, fetched HERE -- before the ticket hand-over and the next item's requests -- and complete before those requests are issued.  Why: on
        // this ISA stores count in vmcnt and may complete out of order with loads, so a load between two stores is answered with `vmcnt(0)`: the x2 output stage
        // (per output row: two noise loads, two stores) ran as EIGHT full round trips per item, each also waiting for the next item's first chunks (cycle
        // counters: 11-12 k cycles per item, 11 % of the 256^2 -> 512^2 layer).  Plain layers: 4 rows in registers.  x2 layers, pair form:
        // the lane fetches rows 2 kq, 2 kq + 1 of its tile's 8 x 8 block (the four lanes kq of a tile share it) and parks them in the wave's 4 KB of V stage 2
        // -- free from the K loop's last barrier until the next item's third chunk is requested --, [row 8][tile 16][8 floats]; the output stage reads rows from LDS
        // and holds no vector-memory load at all.
        const int tt = tr * 16 + l15;
        const int oy = gy * (128 >> p.txl) + (tt >> p.txl) * 4, ox = gx * (4 << p.txl) + (tt & ((1 << p.txl) - 1)) * 4;
        constexpr bool NZ_LDS = PAIR && UPS;
        float* const nzw = smem + 2 * W4_UCH + 4 * W4_VCH + wvx * 1024;
        float4 nz[4];
#pragma unroll
        for (int a = 0; a < 4; a++) nz[a] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.e.noise) {
            if constexpr (NZ_LDS) {
                const float* np = p.e.noise + b * p.e.noise_bstride + (int64_t)(2 * oy + 2 * kq) * (2 * p.W) + 2 * ox;
                nz[0] = *(const float4*)np; nz[1] = *(const float4*)(np + 4);
                nz[2] = *(const float4*)(np + 2 * p.W); nz[3] = *(const float4*)(np + 2 * p.W + 4);
            } else if constexpr (!UPS) {
                const float* np = p.e.noise + b * p.e.noise_bstride + (int64_t)oy * p.W + ox;
#pragma unroll
                for (int a = 0; a < 4; a++) nz[a] = *(const float4*)(np + (int64_t)a * p.W);
            }
        }
        int nsl_ = 0, ntg_ = 0;
        const bool more = acquire(t_next, true, nsl_, ntg_);
        // (UNCONDITIONAL, zeros when the layer has no noise: under a second `if (noise)` the compiler cannot pair the loads with their use and guards every later
        //  reuse of their registers with `vmcnt(3)` -- behind the requests below, i.e. waiting for them; seen in the first build's ISA)
        if constexpr (NZ_LDS) {
            float* d = nzw + ((2 * kq) * 16 + l15) * 8;
            *(float4*)d = nz[0]; *(float4*)(d + 4) = nz[1];
            *(float4*)(d + 128) = nz[2]; *(float4*)(d + 132) = nz[3];
        } else if constexpr (!UPS) {
            // (the values are USED here: the compiler's wait for them stands in front of the requests below, not behind them)
            asm volatile("" : "+v"(nz[0].x), "+v"(nz[0].w), "+v"(nz[1].x), "+v"(nz[1].w), "+v"(nz[2].x), "+v"(nz[2].w), "+v"(nz[3].x), "+v"(nz[3].w));
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) {
            set_bases(nsl_, ntg_);
            if (PAIR) pair_first(nchk); else issue(0, 0);
        }
        // ---- output transform Y = A^T M A in registers; lane = (4 channels 16 cg + 4 kq + r, tile (tr, l15)) ----
        {
            // noise of output row r (0..7) of the lane's 8 x 8 block, x2 layers
            auto up_noise = [&](int r, float4& n0, float4& n1) {
                n0 = make_float4(0.f, 0.f, 0.f, 0.f); n1 = n0;
                if constexpr (!NZ_LDS) { if (!p.e.noise) return; }
                if constexpr (NZ_LDS) {
                    const float* q = nzw + (r * 16 + l15) * 8;
                    n0 = *(const float4*)q; n1 = *(const float4*)(q + 4);
                } else {
                    const float* np = p.e.noise + b * p.e.noise_bstride + (int64_t)(2 * oy + r) * (2 * p.W) + 2 * ox;
                    n0 = *(const float4*)np; n1 = *(const float4*)(np + 4);
                }
            };
            auto write_outputs = [&](auto act_tag) {
                constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int chl = cg * 16 + kq * 4 + r, o = m0 + chl;
                    float t[4][6];                                       // t[a][j] = sum_i A^T[a][i] M[i][j]
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        const float col[6] = {acc[j][r], acc[6 + j][r], acc[12 + j][r], acc[18 + j][r], acc[24 + j][r], acc[30 + j][r]};
                        float y4[4];
                        wino4_at(col, y4);
#pragma unroll
                        for (int a = 0; a < 4; a++) t[a][j] = y4[a];
                    }
                    if (o < p.Cout && tg_ok) {
                        const float dd = side[W4_BM * (1 + hsel) + chl], bs = side[chl];
                        float* yp = p.e.y + (((int64_t)b * p.Cout + o) * p.H + oy) * p.W + ox;
#pragma unroll
                        for (int a = 0; a < 4; a++) {
                            float y4[4];
                            wino4_at(t[a], y4);
                            *(float4*)(yp + (int64_t)a * p.W) = finish_act4<ACT>(p.e, make_float4(y4[0], y4[1], y4[2], y4[3]), dd, nz[a], bs);
                        }
                    }
                }
            };
            // The x2 layers (out_layout 2): the stride-2 transposed 3x3 convolution followed by the 4x4 FIR (conv2d_resample.py:108-125) is, per
            // output parity (py, px), a 3x3 'same' correlation of x with taps folded from the FIR and the weights (ops/modconv.py: fold_up2) --
            // four of the layers above sharing ONE input transform.  Channel 4 o + 2 py + px holds parity (py, px) of real channel o, so a
            // lane's four accumulator rows r are the four parities of one channel for its 4x4 tile: an 8x8 block of the x2 output, written as
            // 16-byte row pieces like the plain layers.  (No Z round trip, no FIR pass; the multiplies per input pixel stay 9.)
            auto write_up = [&](auto act_tag) {
                constexpr int ACT = decltype(act_tag)::value;
                const int och = (m0 >> 2) + cg * 4 + kq, Co = p.Cout >> 2, H2 = 2 * p.H, W2 = 2 * p.W;
                if (och < Co && tg_ok) {
                    const int chl = cg * 16 + kq * 4;
                    const float dd = side[W4_BM * (1 + hsel) + chl], bs = side[chl];   // (replicated per parity by the caller: the four entries are equal)
                    float* yp = p.e.y + (((int64_t)b * Co + och) * H2 + 2 * oy) * W2 + 2 * ox;
#pragma unroll
                    for (int py = 0; py < 2; py++) {                     // the two parities of a row pair at a time (48 instead of 96 live values)
                        float t[2][4][6];                                // [px][a][j]
#pragma unroll
                        for (int px = 0; px < 2; px++)
#pragma unroll
                            for (int j = 0; j < 6; j++) {
                                const int r = 2 * py + px;
                                const float col[6] = {acc[j][r], acc[6 + j][r], acc[12 + j][r], acc[18 + j][r], acc[24 + j][r], acc[30 + j][r]};
                                float y4[4];
                                wino4_at(col, y4);
#pragma unroll
                                for (int a = 0; a < 4; a++) t[px][a][j] = y4[a];
                            }
#pragma unroll
                        for (int a = 0; a < 4; a++) {
                            float e0[4], e1[4];
                            wino4_at(t[0][a], e0);                       // parity (py, 0): columns 0, 2, 4, 6 of this output row
                            wino4_at(t[1][a], e1);                       // parity (py, 1): columns 1, 3, 5, 7
                            const int64_t ro = (int64_t)(2 * a + py) * W2;
                            float4 n0, n1;
                            up_noise(2 * a + py, n0, n1);
                            *(float4*)(yp + ro) = finish_act4<ACT>(p.e, make_float4(e0[0], e1[0], e0[1], e1[1]), dd, n0, bs);
                            *(float4*)(yp + ro + 4) = finish_act4<ACT>(p.e, make_float4(e0[2], e1[2], e0[3], e1[3]), dd, n1, bs);
                        }
                    }
                }
            };
            // K split: the raw sums of this split, no epilogue (splitk_reduce_kernel applies it to the sum of the splits)
            auto write_partial = [&]() {
                float* part = p.partial + (int64_t)(sl & ((1 << p.ksl) - 1)) * ((int64_t)p.B * p.Cout * p.H * p.W);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = m0 + cg * 16 + kq * 4 + r;
                    float t[4][6];
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        const float col[6] = {acc[j][r], acc[6 + j][r], acc[12 + j][r], acc[18 + j][r], acc[24 + j][r], acc[30 + j][r]};
                        float y4[4];
                        wino4_at(col, y4);
#pragma unroll
                        for (int a = 0; a < 4; a++) t[a][j] = y4[a];
                    }
                    if (o < p.Cout && tg_ok) {
                        float* yp = part + (((int64_t)b * p.Cout + o) * p.H + oy) * p.W + ox;
#pragma unroll
                        for (int a = 0; a < 4; a++) {
                            float y4[4];
                            wino4_at(t[a], y4);
                            *(float4*)(yp + (int64_t)a * p.W) = make_float4(y4[0], y4[1], y4[2], y4[3]);
                        }
                    }
                }
            };
            // packed forms (linear / leaky ReLU, the generator's layers): a channel pair at a time -- see wino4_output_pair
            auto write_outputs_pk = [&](auto act_tag) {
                constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
                for (int pr = 0; pr < 2; pr++) {
                    const int chl = cg * 16 + kq * 4 + 2 * pr, o = m0 + chl;
                    w4_f2 yy[4][4];
                    wino4_output_pair(acc, pr, yy);
                    if (tg_ok && o < p.Cout) {
                        const bool two = o + 1 < p.Cout;
                        const w4_f2 d2 = {side[W4_BM * (1 + hsel) + chl], side[W4_BM * (1 + hsel) + chl + 1]}, b2 = {side[chl], side[chl + 1]};
                        float* yp = p.e.y + (((int64_t)b * p.Cout + o) * p.H + oy) * p.W + ox;
                        const int64_t cs = (int64_t)p.H * p.W;
#pragma unroll
                        for (int a = 0; a < 4; a++) {
                            const float nq[4] = {nz[a].x, nz[a].y, nz[a].z, nz[a].w};
                            w4_f2 f[4];
#pragma unroll
                            for (int i = 0; i < 4; i++) f[i] = finish_pair<ACT>(p.e, yy[a][i], d2, nq[i], b2);
                            *(float4*)(yp + (int64_t)a * p.W) = make_float4(f[0].x, f[1].x, f[2].x, f[3].x);
                            if (two) *(float4*)(yp + cs + (int64_t)a * p.W) = make_float4(f[0].y, f[1].y, f[2].y, f[3].y);
                        }
                    }
                }
            };
            // x2 layers: channel 4 o + 2 py + px -- the pair (2 py, 2 py + 1) IS (px = 0, px = 1) of output row parity py: pixel i of the pair is the two
            // horizontally adjacent output pixels (2 x + 0, 2 x + 1), so a 16-byte row piece is two pairs as they stand (no transposition at all)
            auto write_up_pk = [&](auto act_tag) {
                constexpr int ACT = decltype(act_tag)::value;
                const int och = (m0 >> 2) + cg * 4 + kq, Co = p.Cout >> 2, H2 = 2 * p.H, W2 = 2 * p.W;
                const int chl = cg * 16 + kq * 4;
                const float dd = side[W4_BM * (1 + hsel) + chl], bs = side[chl];       // (replicated per parity by the caller: the four entries are equal)
                const w4_f2 d2 = {dd, dd}, b2 = {bs, bs};
                float* yp = p.e.y + (((int64_t)b * Co + och) * H2 + 2 * oy) * W2 + 2 * ox;
#pragma unroll
                for (int py = 0; py < 2; py++) {
                    w4_f2 yy[4][4];
                    wino4_output_pair(acc, py, yy);
                    if (och < Co && tg_ok) {
#pragma unroll
                        for (int a = 0; a < 4; a++) {
                            const int64_t ro = (int64_t)(2 * a + py) * W2;
                            float4 n0, n1;
                            up_noise(2 * a + py, n0, n1);
                            // the noise map is per output pixel: the two halves of a pair take different noise values
                            auto fin = [&](w4_f2 v, float na, float nb) {
                                w4_f2 x = (v * d2 + (w4_f2){na, nb}) + b2;
                                if constexpr (ACT == 3) { const w4_f2 xa = x * (w4_f2){p.e.alpha, p.e.alpha}; x = (w4_f2){__builtin_fmaxf(x.x, xa.x), __builtin_fmaxf(x.y, xa.y)}; }
                                return x * (w4_f2){p.e.gain, p.e.gain};
                            };
                            const w4_f2 f0 = fin(yy[a][0], n0.x, n0.y), f1 = fin(yy[a][1], n0.z, n0.w), f2 = fin(yy[a][2], n1.x, n1.y), f3 = fin(yy[a][3], n1.z, n1.w);
                            *(float4*)(yp + ro) = make_float4(f0.x, f0.y, f1.x, f1.y);
                            *(float4*)(yp + ro + 4) = make_float4(f2.x, f2.y, f3.x, f3.y);
                        }
                    }
                }
            };
            const int evar = epi_variant(p.e);
            if (!UPS && p.ksl > 0) write_partial();
            else
            if constexpr (UPS) {
                if (evar == 3) write_up_pk(std::integral_constant<int, 3>{});
                else if (evar == 1) write_up_pk(std::integral_constant<int, 1>{});
                else write_up(std::integral_constant<int, 0>{});
            } else {
                if (evar == 3) write_outputs_pk(std::integral_constant<int, 3>{});
                else if (evar == 1) write_outputs_pk(std::integral_constant<int, 1>{});
                else write_outputs(std::integral_constant<int, 0>{});
            }
            // the noise rows are USED here whatever path ran: a load still pending at the loop's back edge makes the compiler guard its destination registers with
            // vmcnt waits inside the K loop (seen in the ISA of the first packed build, caught by isa_check: vmcnt(2) / vmcnt(0) at the loop head -- they would
            // also wait for the V pieces the hand-counted vmcnt(4) lets fly)
            asm volatile("" :: "v"(nz[0].x), "v"(nz[0].w), "v"(nz[1].x), "v"(nz[1].w), "v"(nz[2].x), "v"(nz[2].w), "v"(nz[3].x), "v"(nz[3].w));
        }
        lds_barrier();                               // `side` is free for the next item
        have = more; sl = nsl_; tg = ntg_;
    }
}

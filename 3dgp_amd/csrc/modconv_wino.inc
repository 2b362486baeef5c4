// modconv_wino.inc -- included by modconv.hip (inside its anonymous namespace).
//
// The stride-1 3x3 layers of the synthesis blocks (networks_stylegan2.py:31-88 -> conv2d_resample.py:127-134, padding 1) as
// Winograd F(2x2, 3x3) in fp32: y = A^T [ (G g G^T) . (B^T d B) ] A per 2x2 output tile and (cin, cout) pair -- 16 multiplies
// for 4 outputs instead of 36, an algebraic identity of the convolution (cuDNN picks the same algorithm for the reference's fp32
// 3x3 convolutions); the rounding differs from the direct sum the way any re-association does (measured against the double-
// accumulating oracle in tests/test_gpu_parity.py).  The direct kernel runs the fp32 matrix pipe 83 % busy, so fewer multiplies is
// the only lever left in this arithmetic.
//
// Formulation: 16 independent GEMMs, one per position xi = (i, j) of the 4x4 transform:
//     Y_xi[cout][tile] = sum_cin U_xi[cout][cin] * V_xi[cin][tile],   U = G g G^T (packed once), V = B^T (s * d) B (per block),
// on v_mfma_f32_32x32x2_f32.  Block = 8 waves, 64 output channels x 64 tiles (8 rows x 32 columns of one sample); wave w owns
// transform ROW i = w & 3 (its 4 positions j = 0..3) of channel half w >> 2: 4 x (32 channels x 64 tiles) = 128 accumulators, and
// the j-half of the output transform, Z[i][b] = sum_j Y[i][j] A[j][b], is register-local; the i-half goes through LDS once.
// K chunk = 8 input channels:
//   * U chunk [xi][half][64 channels][4 k] (32 KB): a lane's A operands of the 4 k-steps are one 16-byte read, conflict-free;
//   * raw patch [8 k][10 rows][34 columns] of the style-scaled activations (row pitch 48: the two tile rows a 32-lane LDS access
//     covers fall on disjoint banks), wave w transforms channel k = w for all 64 tiles (lane = tile): 8 x ds_read_b64, 32 adds,
//     16 x ds_write_b32 into V [xi][k][tile] (4-byte accesses with lanes on consecutive tiles: conflict-free both ways);
//   * 32 MFMAs per wave and chunk (4 positions x 2 tile halves x 4 k-steps), k-step s multiplying channels {s, s + 4}.
// Double-buffered U / V / patch (2 x (32 + 32 + 15) KB): one block per CU, ONE barrier per chunk, and the two waves of a SIMD run a
// chunk's three parts (stage, transform, multiply) in different orders, see the loop; global loads run 2-3 chunks ahead.  The vector work (transform) and the matrix work share the SIMD's issue port (DESIGN.md
// (e)), so the transform is priced in matrix time: ~100 vector instructions against 32 x 64 cycles per chunk and wave.
// Staging per FLOP is 3.4x the direct kernel's (K = Cin per position instead of 9 Cin): 47 KB per block and chunk from L2.

struct WinoParams {
    const float* x; const float* u; const float* styles;
    EpiParams e;
    int B, Cin, Cout, CoutP, H, W;
    uint32_t x_bytes, u_bytes;
};

// weight [Cout,Cin,3,3] -> U [chunk8][xi = 4i + j][half][CoutP][4 k] with U_xi = (G g G^T)[i][j], channel = 8 chunk + 4 half + k
__global__ __launch_bounds__(256) void pack_wino_kernel(const float* __restrict__ w, float* __restrict__ u, int Cout, int Cin, int CoutP, int nch8) {
    const int64_t total = (int64_t)nch8 * 16 * 2 * CoutP * 4;
    const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int kq = (int)(idx % 4);
        int64_t r = idx / 4;
        const int col = (int)(r % CoutP); r /= CoutP;
        const int hf = (int)(r % 2); r /= 2;
        const int xi = (int)(r % 16);
        const int ch = (int)(r / 16);
        const int c = ch * 8 + hf * 4 + kq, i = xi >> 2, j = xi & 3;
        double v = 0.0;
        if (col < Cout && c < Cin) {
            const float* g = w + ((int64_t)col * Cin + c) * 9;
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) v += G[i][a] * (double)g[a * 3 + b] * G[j][b];      // exact in double: one rounding to fp32 below
        }
        u[idx] = (float)v;
    }
}

__global__ __launch_bounds__(512, 1) void conv3_wino_kernel(WinoParams p) {
    constexpr int KC = 8, BM = 64, NTL = 64, RP = 48, RAW = KC * 10 * RP, UB = 16 * 2 * BM * 4, VB = 16 * KC * NTL;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Us = smem;                   // [2][xi][half][64][4]
    float* Vs = Us + 2 * UB;            // [2][xi][k][tile]
    float* raw = Vs + 2 * VB;           // [2][k][row][RP]: patch column q (image column n0 - 4 + q) sits at q + 1 -> a tile's window starts 8-byte aligned
    float* side = raw + 2 * RAW;        // [0..64) bias, [64..128) demodulation coefficients of this block's sample
    const int tid = threadIdx.x, l = tid & 63, wv = TDGP_WAVE_INDEX(tid), l32 = l & 31, half = l >> 5;
    const int tilesX = p.W >> 5, tilesY = p.H >> 3;
    // PERSISTENT blocks (one per CU -- the LDS allows no second one): a block walks the (tile, channel-slice) items its index strides over, tiles
    // fastest, so that the CUs work on one channel slice's weights at a time as the 2-D grid did.  With a block per item the 64 blocks a CU
    // runs back to back for the 512^2 layer (8 chunks of K each) each paid their own dispatch; the layers with few input channels sat
    // at 0.49-0.55 of the MFMA peak where the 512-channel layer reaches 0.60.
    const int nbx = tilesX * tilesY * p.B, nitems = nbx * ((p.Cout + BM - 1) / BM);
    // Staging state lives across items: the first chunk of the NEXT item is requested while the current item's output stage runs (its global
    // latency was exposed once per item: 64 times per CU for the 512^2 layer).
    // patch: 8 channels x 10 rows x 10 aligned 16-byte vectors (image columns n0 - 4 .. n0 + 35): 800 items, <= 2 per thread;  U chunk: 2048
    // 16-byte vectors, 4 per thread, LDS destination linear
    uint32_t r_vo[2], r_so[2], u_vo[4];
    int r_ld[2];
    auto setup_item = [&](int it) {
        const int bx = it % nbx, tx = bx % tilesX, ty = (bx / tilesX) % tilesY, b = bx / (tilesX * tilesY);
        const int n0 = tx * 32, r0 = ty * 8, m0 = (it / nbx) * BM;
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int e = tid + s * 512, k = min(e / 100, KC - 1), rem = e - k * 100, row = rem / 10, v = rem - row * 10;
            const int iy = r0 - 1 + row, ix = n0 - 4 + 4 * v;
            r_vo[s] = kOOB; r_so[s] = (uint32_t)(b * p.Cin + k) * 4u; r_ld[s] = e < 800 ? (k * 10 + row) * RP + 4 * v + 1 : -1;
            if (e < 800 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) r_vo[s] = (uint32_t)(((b * p.Cin + k) * p.H + iy) * p.W + ix) * 4u;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = tid + i * 512, xh = e >> 6, ch = e & 63;
            u_vo[i] = (uint32_t)(xh * p.CoutP + min(m0 + ch, p.CoutP - 1)) * 16u;
        }
    };
    const uint32_t r_cstride = (uint32_t)(KC * p.H * p.W) * 4u;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.styles ? (const void*)p.styles : (const void*)p.x, p.styles ? (uint32_t)(p.B * p.Cin) * 4u : 0u);
    const uint32_t u_cstride = (uint32_t)(32 * p.CoutP) * 16u;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes), ru = make_rsrc(p.u, p.u_bytes);

    // the style of an item's channel rides along with its activations (one dword per item and chunk, an L1 hit)
    u32x4 u_reg[4], x_reg[2];
    float s_reg[2];
    auto load_u = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; i++) u_reg[i] = __builtin_amdgcn_raw_buffer_load_b128(ru, u_vo[i], (uint32_t)c * u_cstride, 0);
    };
    auto load_x = [&](int c) {
#pragma unroll
        for (int s = 0; s < 2; s++) {
            x_reg[s] = __builtin_amdgcn_raw_buffer_load_b128(rx, r_vo[s], (uint32_t)c * r_cstride, 0);
            s_reg[s] = p.styles ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, r_so[s], (uint32_t)(c * KC) * 4u, 0)) : 1.f;
        }
    };
    auto store_u = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; i++) *(u32x4*)(Us + buf * UB + (tid + i * 512) * 4) = u_reg[i];
    };
    auto store_x = [&](int rbuf) {
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (r_ld[s] >= 0) {
                const float sc = s_reg[s];
                float* d = raw + rbuf * RAW + r_ld[s];
                d[0] = __uint_as_float(x_reg[s].x) * sc;
                *(float2*)(d + 1) = make_float2(__uint_as_float(x_reg[s].y) * sc, __uint_as_float(x_reg[s].z) * sc);
                d[3] = __uint_as_float(x_reg[s].w) * sc;
            }
        }
    };
    const int item0 = (int)blockIdx.x, istep = (int)gridDim.x;
    if (item0 < nitems) { setup_item(item0); load_u(0); load_x(0); }
  for (int item = item0; item < nitems; item += istep) {
    const int bx = item % nbx, tx = bx % tilesX, ty = (bx / tilesX) % tilesY, b = bx / (tilesX * tilesY);
    const int n0 = tx * 32, r0 = ty * 8, m0 = (item / nbx) * BM;

    if (tid < 2 * BM) {
        const int o = m0 + (tid & (BM - 1));
        float v = tid < BM ? 0.f : 1.f;
        if (o < p.Cout) {
            if (tid < BM) { if (p.e.bias) v = p.e.bias[o]; }
            else if (p.e.dcoef) v = p.e.dcoef[b * p.e.Cout + o];
        }
        side[tid] = v;
    }

    // input transform of channel k = wv of the staged patch for tile = lane: V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
    const int tyl = l >> 4, txl = l & 15;
    const float* win0 = raw + (wv * 10 + 2 * tyl) * RP + 2 * txl + 4;
    auto transform = [&](int rbuf, int buf) {
        const float* win = win0 + rbuf * RAW;
        float d[4][4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float2 a = *(const float2*)(win + r * RP), c2 = *(const float2*)(win + r * RP + 2);
            d[r][0] = a.x; d[r][1] = a.y; d[r][2] = c2.x; d[r][3] = c2.y;
        }
        float t[4][4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            t[0][c] = d[0][c] - d[2][c];
            t[1][c] = d[1][c] + d[2][c];
            t[2][c] = d[2][c] - d[1][c];
            t[3][c] = d[1][c] - d[3][c];
        }
        float* vdst = Vs + buf * VB + wv * NTL + l;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            vdst[(4 * i + 0) * KC * NTL] = t[i][0] - t[i][2];
            vdst[(4 * i + 1) * KC * NTL] = t[i][1] + t[i][2];
            vdst[(4 * i + 2) * KC * NTL] = t[i][2] - t[i][1];
            vdst[(4 * i + 3) * KC * NTL] = t[i][1] - t[i][3];
        }
    };

    f32x16 acc[4][2];                   // [j][tile half]
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[j][n][r] = 0.f;

    const int wi = wv & 3, mh = wv >> 2;
    // A: Us[buf][((xi*2 + half)*64 + mh*32 + l32)*4 .. +3]; B: Vs[buf][(xi*8 + 4*half + s)*64 + n*32 + l32]
    const int a_lane = ((wi * 4 * 2 + half) * BM + mh * 32 + l32) * 4;          // + j * 2*BM*4
    const int b_lane = (wi * 4 * KC + 4 * half) * NTL + l32;                    // + (j*KC + s)*NTL + n*32
    auto mma_chunk = [&](int buf) {
        const float* ua = Us + buf * UB + a_lane;
        const float* vb = Vs + buf * VB + b_lane;
        float4 fa[2];
        float fb[2][2][4];
        auto read_frags = [&](int j, int q) {
            fa[q] = *(const float4*)(ua + j * 2 * BM * 4);
#pragma unroll
            for (int n = 0; n < 2; n++)
#pragma unroll
                for (int s = 0; s < 4; s++) fb[q][n][s] = vb[(j * KC + s) * NTL + n * 32];
        };
        read_frags(0, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j + 1 < 4) read_frags(j + 1, (j + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            const float av[4] = {fa[j & 1].x, fa[j & 1].y, fa[j & 1].z, fa[j & 1].w};
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int n = 0; n < 2; n++) acc[j][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], fb[j & 1][n][s], acc[j][n], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // One barrier per chunk.  Entering iteration c: U[c & 1], V[c & 1] hold chunk c, the patch of chunk c + 1 sits in raw[(c + 1) & 1], the
    // staging registers hold U of chunk c + 1 and the activations of chunk c + 2.  Its three parts touch disjoint buffers:
    //   stage     : registers -> U[nxt] (chunk c + 1) and raw[c & 1] (chunk c + 2); loads of U (c + 2) and activations (c + 3) issued;
    //   transform : raw[(c + 1) & 1] -> V[nxt];
    //   multiply  : chunk c.
    // so the two waves of a SIMD (w and w + 4) run them in different orders -- one multiplies while the other stages and transforms,
    // and the LDS / memory waits of one are covered by the MFMAs of the other (the instructions still share the issue port).
    const int nchunk = p.Cin / KC;
    store_u(0); store_x(0);             // chunk 0 was requested before the loop / during the previous item's output stage
    __syncthreads();
    if (nchunk > 1) { load_u(1); load_x(1); }
    transform(0, 0);
    if (nchunk > 1) store_x(1);
    if (nchunk > 2) load_x(2);
    auto stage = [&](int c) {
        if (c + 1 < nchunk) store_u((c + 1) & 1);
        if (c + 2 < nchunk) { store_x(c & 1); load_u(c + 2); }
        if (c + 3 < nchunk) load_x(c + 3);
    };
    // (one copy of the code: the second group runs the same loop skewed by half an iteration -- its multiply of chunk c + 1 follows its
    //  stage / transform of iteration c -- and the barrier sits on the other side of the stage part; every wave executes nchunk + 1 barriers)
    const bool g1 = wv >= 4;
    for (int c = g1 ? -1 : 0; c < nchunk; c++) {
        if (!g1) __syncthreads();
        if (c >= 0) {
            stage(c);
            if (c + 1 < nchunk) transform((c + 1) & 1, (c + 1) & 1);
        }
        if (g1) __syncthreads();
        const int cm = c + (g1 ? 1 : 0);
        if (cm < nchunk) {
            mma_chunk(cm & 1);
        }
    }
    if (!g1) __syncthreads();

    // ---- output transform, A^T = [1 1 1 0; 0 1 -1 -1]: the j-half in registers, the i-half through LDS (overlaying the stage buffers)
    float* Zs = smem;                   // [mh][i][b][32 channels][64 tiles]
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float y0 = acc[0][n][r], y1 = acc[1][n][r], y2 = acc[2][n][r], y3 = acc[3][n][r];
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            float* z = Zs + (((mh * 4 + wi) * 2) * 32 + row) * NTL + n * 32 + l32;
            z[0] = (y0 + y1) + y2;
            z[32 * NTL] = (y1 - y2) - y3;
        }
    // the next item's first chunk (unconditional: the block's last item re-requests itself -- a load under a condition makes hipcc wait for it at the join)
    setup_item(item + istep < nitems ? item + istep : item);
    load_u(0); load_x(0);
    __syncthreads();
    const int oy = r0 + 2 * tyl, ox = n0 + 2 * txl;
    float2 nz0 = make_float2(0.f, 0.f), nz1 = nz0;
    if (p.e.noise) {
        const float* np = p.e.noise + b * p.e.noise_bstride + (int64_t)oy * p.W + ox;
        nz0 = *(const float2*)np; nz1 = *(const float2*)(np + p.W);
    }
    auto write_outputs = [&](auto act_tag) {
        constexpr int ACT = decltype(act_tag)::value;
#pragma unroll 2
        for (int q = 0; q < 8; q++) {
            const int ch = q * 8 + wv, o = m0 + ch;
            if (o < p.Cout) {
                const float* z = Zs + (((ch >> 5) * 4 * 2) * 32 + (ch & 31)) * NTL + l;
                float zz[4][2];
#pragma unroll
                for (int i = 0; i < 4; i++) { zz[i][0] = z[(i * 2) * 32 * NTL]; zz[i][1] = z[(i * 2 + 1) * 32 * NTL]; }
                const float d = side[BM + ch], bb = side[ch];
                float o0[2], o1[2];
#pragma unroll
                for (int bc = 0; bc < 2; bc++) {
                    o0[bc] = (zz[0][bc] + zz[1][bc]) + zz[2][bc];
                    o1[bc] = (zz[1][bc] - zz[2][bc]) - zz[3][bc];
                }
                float* yp = p.e.y + (((int64_t)b * p.Cout + o) * p.H + oy) * p.W + ox;
                *(float2*)yp = make_float2(finish_act<ACT>(p.e, (o0[0] * d + nz0.x) + bb), finish_act<ACT>(p.e, (o0[1] * d + nz0.y) + bb));
                *(float2*)(yp + p.W) = make_float2(finish_act<ACT>(p.e, (o1[0] * d + nz1.x) + bb), finish_act<ACT>(p.e, (o1[1] * d + nz1.y) + bb));
            }
        }
    };
    // the generator's form (leaky ReLU, no clamp) with the activation decided at compile time, everything else through the run-time switch
    const int evar = epi_variant(p.e);
    if (evar == 3) write_outputs(std::integral_constant<int, 3>{});
    else if (evar == 4) write_outputs(std::integral_constant<int, 4>{});
    else write_outputs(std::integral_constant<int, 0>{});
    __syncthreads();                    // the output stage has read Zs / side: the next item may stage over them
  }
}

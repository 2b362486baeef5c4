// modconv_wino4f.inc -- included by modconv.hip (inside its anonymous namespace), after modconv_wino4.inc.
//
// F(4x4, 3x3) for the stride-1 3x3 layers with FEW input channels (Cin <= 128: the 256^2 and 512^2 blocks of the tri-plane backbone,
// networks_stylegan2.py:31-88 -> conv2d_resample.py:127-134) with the INPUT transform inside the GEMM kernel (round 6).
//
// Why: with the transform as a pass of its own (wino4_input_kernel) V = B^T d B is 2.25 x the input, written to HBM and read back.  At
// Cin = Cout = 64 on 512^2 (B = 16) that is 2.4 GB written + 2.4 GB read for a layer whose own input and output are 1.07 GB each and
// whose multiplies take 0.5 ms at the fp32 MFMA peak: measured 0.75 ms (transform pass, at the HBM rate) + 0.90 ms (GEMM, waiting for
// V) = 1.65 ms; 256^2 x 128: 0.35 + 0.79 ms.  Here a block takes ALL 64 output channels of a slice x one tile group (32 tiles = 8 x 64
// pixels), so at Cout = 64 every input window is transformed exactly once -- by the block that multiplies it -- and V only ever exists
// in LDS.  HBM traffic of the layer = x once (+ halo rows) + y once.
//
//   block = 8 waves, one per CU.  Wave (cg = w & 3, tr = w >> 2) owns all 36 positions of 16 channels x 16 tiles (144 accumulators, as
//   conv3_wino4_kernel: the output transform stays register-local).  U arrives by LDS-direct loads, 2 stages of [2 slices of 32][9][4][32][4]
//   (the BM = 32 pack of pack_wino4_kernel, two neighbouring slices); V lives in a ring of 4 chunk slots [9][4][32][4] filled by the waves
//   themselves:
//   * a wave PAIR p = w >> 1 prepares the chunks c = p (mod 4); wave half h = w & 1 takes channels 2 h, 2 h + 1 of the chunk, lane =
//     (channel, tile): one 6x6 window per lane (exactly wino4_input_kernel's arithmetic: x * style, B^T d B with the same fma chains --
//     V, and with it every output bit, equals the two-kernel path's);
//   * the K loop is unrolled by four and the transform of the NEXT four chunks is spread over it -- chunk 4 q: request the windows (18 loads
//     per lane, unconditional, at a fixed place), 4 q + 1: modulate + column pass, 4 q + 2: row pass, 4 q + 3: pairs 0..2 store their V
//     (pair 3's slot is being read; it stores at the top of the next round).  Every wave does the same share in the same chunk, so the four
//     SIMDs stay balanced under the one barrier per chunk, and the transform state is ONE array of 36 registers that lives in the K loop's
//     spare registers (the 239-register peak of this kernel family is the output stage).
//   Cost on the issue port the matrix pipe shares: ~55 vector instructions + 4.5 loads + 2.25 LDS stores per wave and chunk next to 36 MFMAs
//   (+ ~20 %), against the whole transform pass and the V round trip.  Requires Cin % 16 == 0, Cout % 64 == 0, whole 64 x 8-pixel tile
//   groups (txl = 4), a plain layer (no K split, out_layout 0).

struct Wino4fParams {
    const float* x; const float* styles; const float* u;
    EpiParams e;
    int B, Cin, Cout, H, W;
    uint32_t u_bytes, x_bytes, st_bytes, nz_bytes;       // nz_bytes: size of the noise tensor (0: no noise)
    int gxn, gyn;                  // tile groups per row / column of a sample (64 x 8 pixels each)
    int rs, rt, nxcd;              // as Wino4Params: rectangle of an XCD, rs channel slices (of 64) x rt tile groups
    int* ticket;                   // [nxcd] item counters, zeroed by the launcher (a memset node on the stream)
};

constexpr int W4F_MAXCIN = 128;    // most input channels the fused kernel takes (the styles table of W4F_SIDE)
static_assert(W4_BM == 32, "wino4f: two BM = 32 slices of the U pack per block");
constexpr int W4F_UST = 2 * W4_UCH;            // floats per U stage: two slices
constexpr int W4F_NV = 4;                      // V ring slots (chunks)
constexpr int W4F_SIDE = 64 + 64 + 128 + 4;    // bias, demodulation coefficients, the sample's styles (Cin <= 128), the ticket
constexpr int W4F_HALO = 8 * 256;              // per wave 1 KB: the windows' left / right neighbour columns that belong to other tile groups
constexpr int W4F_NOISE = 2 * 8 * 64;           // two 8 x 64-pixel noise patches (the item being multiplied and the next one)
constexpr int W4F_LDS_FLOATS = 2 * W4F_UST + W4F_NV * W4_VCH + W4F_SIDE + W4F_HALO + W4F_NOISE;
static_assert(W4F_LDS_FLOATS * 4 <= 160 * 1024 && W4F_MAXCIN <= 128, "wino4f: LDS layout");

__global__ __launch_bounds__(512, 1) void conv3_wino4f_kernel(Wino4fParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const uint32_t lds0 = TDGP_LDS_BASE(smem);
    float* const vring = smem + 2 * W4F_UST;
    float* const side = vring + W4F_NV * W4_VCH;            // [0..64) bias, [64..128) demodulation coefficients, [128..256) styles of the item's sample
    int* const tk = (int*)(side + 256);
    const uint32_t lds_v = lds0 + (uint32_t)(2 * W4F_UST) * 4u, lds_sty = lds_v + (uint32_t)(W4F_NV * W4_VCH + 128) * 4u;
    const uint32_t lds_halo = lds_v + (uint32_t)(W4F_NV * W4_VCH + W4F_SIDE) * 4u;
    const uint32_t lds_noise = lds_halo + (uint32_t)W4F_HALO * 4u;
    const int tid = threadIdx.x, l = tid & 63, wvx = TDGP_WAVE_INDEX(tid);
    const int cg = wvx & 3, tr = wvx >> 2;
    const int pairw = wvx >> 1, hsel = wvx & 1;             // transform role: chunks = pairw (mod 4), channels 2 hsel, 2 hsel + 1 of the chunk
    const int nch = p.Cin >> 2;                             // chunks per item (a multiple of 4)
    const int ntg = p.gxn * p.gyn * p.B, nsl = p.Cout >> 6;
    const int xcd = (int)blockIdx.x % p.nxcd;
    const int RS = (nsl + p.rs - 1) / p.rs, RT = (ntg + p.rt - 1) / p.rt, nrect = RS * RT;
    const uint32_t lane16 = (uint32_t)l * 16u;
    typedef unsigned int w4_u32x4 __attribute__((ext_vector_type(4)));
    const uint64_t ua = (uint64_t)(uintptr_t)p.u, xa = (uint64_t)(uintptr_t)p.x;
    const w4_u32x4 du = {(uint32_t)ua, (uint32_t)((ua >> 32) & 0xffffu), p.u_bytes, 0x00020000u};
    const w4_u32x4 dx = {(uint32_t)xa, (uint32_t)((xa >> 32) & 0xffffu), p.x_bytes, 0x00020000u};
    const uint64_t na = (uint64_t)(uintptr_t)(p.e.noise ? p.e.noise : p.x);
    const uint64_t sa = (uint64_t)(uintptr_t)(p.styles ? p.styles : p.x);
    const w4_u32x4 ds = {(uint32_t)sa, (uint32_t)((sa >> 32) & 0xffffu), p.styles ? p.st_bytes : 0u, 0x00020000u};
    const w4_u32x4 dn = {(uint32_t)na, (uint32_t)((na >> 32) & 0xffffu), p.e.noise ? p.nz_bytes : 0u, 0x00020000u};
    // LDS-direct loads by hand (see conv3_wino4_kernel: the compiler would wait for every load in flight in front of the next ds_read); M0 is written
    // in the statement that uses it
    auto dma = [&](const w4_u32x4& d, uint32_t lds_dst, uint32_t voff, uint32_t soff) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(lds_dst), "v"(voff), "s"(d), "s"(soff) : "memory");
    };
    // U pieces of a chunk: 36 x 1 KB (slice 0: pieces 0..17, slice 1: 18..35, contiguous in the stage); wave w issues q = w + 8 i (i = 4: waves 0..3 only)
    uint32_t u_base = 0, u_slice = 0;            // byte offset of the item's first chunk in slice 0; distance to slice 1
    auto pieceU = [&](int i, int c, uint32_t stage_lds) {       // i is a compile-time constant at every call site
        const int q = wvx + 8 * i;
        // (the piece's place inside its slice goes into the SCALAR offset: one vector offset -- the lane's 16 bytes -- serves every piece)
        const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane((int)(u_base + (q >= 18 ? u_slice : 0u) + (uint32_t)c * (W4_UCH * 4u) + (uint32_t)(q >= 18 ? q - 18 : q) * 1024u));
        dma(du, (uint32_t)__builtin_amdgcn_readfirstlane((int)(stage_lds + (uint32_t)q * 1024u)), lane16, so);
    };
    auto issueU = [&](int c, int buf) {
        const uint32_t dst = lds0 + (uint32_t)buf * (W4F_UST * 4u);
#pragma unroll
        for (int i = 0; i < 5; i++) if (i < 4 || wvx < 4) pieceU(i, c, dst);
    };
    auto wait_loads = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    // fragments: A: U[slice cg >> 1][xi4][k = kq][16 (cg & 1) + l15][e];  B: V[xi4][kq][16 tr + l15][e]
    const int a_lane = (cg >> 1) * W4_UCH + ((l >> 4) * 32 + (cg & 1) * 16 + (l & 15)) * 4;
    const int b_lane = ((l >> 4) * 32 + tr * 16 + (l & 15)) * 4;
    const uint32_t a_base = lds0 + (uint32_t)a_lane * 4u, b_base = lds_v + (uint32_t)b_lane * 4u;

    // ---- the transform role of this wave: lane = (channel kk of the chunk, tile tt of the group) --------------------------------------------------
    // A window never lives in registers across a chunk of MFMAs (round 6, second form: 36 registers of window state beside 144 accumulators spilled, and every
    // spill reload waited for the LDS-direct loads in flight).  Instead the window ROWS travel by LDS-direct loads straight into the place the lane's V
    // will occupy: lane (k, t) owns the nine 16-byte slots [q][k][t] of its chunk's ring slot; rows 0..5 of its window (the four middle columns) land in
    // q = 0..5 -- a wave's 64 lanes are 1 KB contiguous there --, the left / right neighbour column of a row is the neighbouring LANE's slot (tile t -+ 1)
    // or, at the ends of the tile group, one of 24 + 24 aligned quads fetched into the wave's 1 KB halo area by a seventh load.  The transform then reads
    // 6 x (16 + 4 + 4) bytes from LDS, runs B^T d B in registers BETWEEN two chunks and overwrites its nine slots with V.  Same arithmetic as
    // wino4_input_kernel (x * style, the wino4_bt fma chains): same V, same output bits.
    // (everything below that is a function of the lane id alone is RECOMPUTED from an opaque copy of it where it is used -- a dozen vector instructions per item
    //  instead of a dozen registers live through the K loop and the output stage, the register peak of this kernel family)
    const uint32_t rowB = (uint32_t)p.W * 4u, chB = (uint32_t)(p.H * p.W) * 4u;
    const uint32_t halo_w = lds_halo + (uint32_t)wvx * 1024u;
    // halo quad j = ((kkl 2 x tty 2) x side 2) x row 6 of the wave's halo area: lane j < 48 FETCHES quad j; lane (kkl, tty) READS quads ((kkl * 2 + tty) * 2 + side) * 6 + r
    uint32_t item_vo = 0, item_hv = 0;              // byte offset of window row 1 (always inside the image), column x0, channel kk of chunk 0; of this lane's halo quad (or kOOB)
    uint32_t m_top = 0, m_bot = 0;                  // 0 where the top / bottom window row lies inside the image, else kOOB (OR-ed into an offset: out of range, reads 0)
    int item_b = 0;
    auto set_item_x = [&](int tg_) {
        int lq = l;
        asm volatile("" : "+v"(lq));
        const int kk = 2 * hsel + (lq >> 5), ttx = lq & 15, tty = (lq >> 4) & 1;
        const int hj_r = lq % 6, hj_side = (lq / 6) & 1, hj_tty = (lq / 12) & 1, hj_kk = 2 * hsel + ((lq / 24) & 1);
        const int gx_ = tg_ % p.gxn, gy_ = (tg_ / p.gxn) % p.gyn, b_ = tg_ / (p.gxn * p.gyn);
        const int y0 = gy_ * 8 + tty * 4 - 1, x0 = gx_ * 64 + ttx * 4;              // first window row (may be -1), first tile column
        item_b = b_;
        item_vo = (uint32_t)(b_ * p.Cin + kk) * chB + (uint32_t)(y0 + 1) * rowB + (uint32_t)x0 * 4u;
        m_top = y0 >= 0 ? 0u : kOOB; m_bot = y0 + 5 < p.H ? 0u : kOOB;
        const int hy = gy_ * 8 + hj_tty * 4 - 1 + hj_r, hx = hj_side ? gx_ * 64 + 64 : gx_ * 64 - 4;
        item_hv = (lq < 48 && hy >= 0 && hy < p.H && hx >= 0 && hx < p.W) ? (uint32_t)(b_ * p.Cin + hj_kk) * chB + (uint32_t)hy * rowB + (uint32_t)hx * 4u : kOOB;
    };
    auto request = [&](int chunk) {                 // 6 window rows + the halo quads of chunk `chunk` -> ring slot chunk & 3 / the halo area (7 LDS-direct loads)
        const uint32_t cso = (uint32_t)__builtin_amdgcn_readfirstlane(chunk * 4) * chB;
        const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_v + (uint32_t)(chunk & 3) * (W4_VCH * 4u) + (uint32_t)hsel * 1024u));
        uint32_t vo1 = item_vo, mt = m_top, mb = m_bot;
        asm volatile("" : "+v"(vo1), "+v"(mt), "+v"(mb));       // (opaque: the offset variants are formed here, not hoisted out of the K loop as live registers)
        // rows 1..5 from row 1's offset with (r - 1) rows in the SCALAR offset; row 0 is one row above: the step goes into the vector offset, which is
        // only in range where the row exists (a scalar offset cannot go below zero, and a wrapped vector offset fails the descriptor's range check)
        dma(dx, dst, (vo1 - rowB) | mt, cso);
#pragma unroll
        for (int r = 1; r < 6; r++) dma(dx, dst + (uint32_t)r * 2048u, r == 5 ? (vo1 | mb) : vo1, cso + (uint32_t)(r - 1) * rowB);
        dma(dx, (uint32_t)__builtin_amdgcn_readfirstlane((int)halo_w), item_hv, cso);
    };
    // the transform of chunk `chunk`, between two chunks of MFMAs: LDS -> 36 registers -> LDS
    typedef const __attribute__((address_space(3))) f32x4* lds_f4p;
    typedef const __attribute__((address_space(3))) float* lds_f1p;
    typedef __attribute__((address_space(3))) f32x4* lds_f4w;
    auto transform = [&](int chunk) {
        int lq = l;
        asm volatile("" : "+v"(lq));                             // (opaque: the per-row halo addresses are lane constants, and hoisted out of the K loop they were eight spilled registers)
        const int kkl = lq >> 5, kk = 2 * hsel + kkl, ttx_ = lq & 15, tty = (lq >> 4) & 1;
        const uint32_t own = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_v + (uint32_t)(chunk & 3) * (W4_VCH * 4u))) + (uint32_t)(64 * hsel + lq) * 16u;
        const float sty = p.styles ? *(lds_f1p)lds_ptr(lds_sty + (uint32_t)(chunk * 4 + kk) * 4u) : 1.0f;
        // left / right neighbour pixel of row r: the last pixel of tile t - 1's quad / the first of tile t + 1's, or the halo quads at the group's ends
        const uint32_t hrd = halo_w + (uint32_t)((kkl * 2 + tty) * 2) * 96u;         // + side * 96 + r * 16 (+ 12: the last pixel of the left quad)
        const uint32_t la = ttx_ > 0 ? own - 4u : hrd + 12u, ra = ttx_ < 15 ? own + 16u : hrd + 96u;
        const uint32_t ls = ttx_ > 0 ? 2048u : 16u, rs_ = ttx_ < 15 ? 2048u : 16u;
        float st[36];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const f32x4 mid = *(lds_f4p)lds_ptr(own + (uint32_t)r * 2048u);
            st[r * 6 + 0] = *(lds_f1p)lds_ptr(la + (uint32_t)r * ls);
            st[r * 6 + 1] = mid[0]; st[r * 6 + 2] = mid[1]; st[r * 6 + 3] = mid[2]; st[r * 6 + 4] = mid[3];
            st[r * 6 + 5] = *(lds_f1p)lds_ptr(ra + (uint32_t)r * rs_);
        }
#pragma unroll
        for (int cc = 0; cc < 6; cc++) {            // d = x * style;  B^T d along rows, column by column
            const float col[6] = {st[0 + cc] * sty, st[6 + cc] * sty, st[12 + cc] * sty, st[18 + cc] * sty, st[24 + cc] * sty, st[30 + cc] * sty};
            float o[6];
            wino4_bt(col, o);
#pragma unroll
            for (int i = 0; i < 6; i++) st[i * 6 + cc] = o[i];
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {               // (B^T d) B, row by row
            const float rw[6] = {st[i * 6 + 0], st[i * 6 + 1], st[i * 6 + 2], st[i * 6 + 3], st[i * 6 + 4], st[i * 6 + 5]};
            float o[6];
            wino4_bt(rw, o);
#pragma unroll
            for (int j = 0; j < 6; j++) st[i * 6 + j] = o[j];
        }
        // V[xi4 9][k 4][tile 32][4]: the lane's nine slots (every read of this wave -- its own rows and its neighbours' -- was issued above: LDS runs a
        // wave's instructions in order)
#pragma unroll
        for (int q = 0; q < 9; q++) *(lds_f4w)lds_ptr(own + (uint32_t)q * 2048u) = (f32x4){st[4 * q], st[4 * q + 1], st[4 * q + 2], st[4 * q + 3]};
    };

    // ---- items: tickets of the XCD's counter, as conv3_wino4_kernel ----
    const int per = p.rs * p.rt;
    auto from_ticket = [&](int t, int& sl, int& tg) {
        const int R = (t / per) * p.nxcd + xcd, j = t % per;
        if (R >= nrect) return -1;
        sl = (R % RS) * p.rs + j % p.rs;
        tg = (R / RS) * p.rt + j / p.rs;
        return (sl < nsl && tg < ntg) ? 1 : 0;
    };
    auto acquire = [&](int t_have, bool have_t, int& sl, int& tg) {
        for (;;) {
            if (tid == 0) tk[0] = have_t ? t_have : atomicAdd(p.ticket + xcd, 1);
            lds_barrier();
            const int t = __builtin_amdgcn_readfirstlane(tk[0]);      // (wave-uniform: the ticket -> item arithmetic, a dozen integer divisions per item, runs on the scalar unit)
            lds_barrier();
            const int stt = from_ticket(t, sl, tg);
            if (stt != 0) return stt > 0;
            have_t = false;
        }
    };
    int item_par = 0;                                // parity of the NEXT item to begin (its noise patch buffer)
    int sl = 0, tg = 0;
    bool have = acquire(0, false, sl, tg);
    auto set_item_u = [&](int sl_) {                 // the item's U chunks (needed before the output stage of the previous item: its first chunk travels under it)
        u_base = (uint32_t)(2 * sl_) * (uint32_t)nch * (W4_UCH * 4u);
        u_slice = (uint32_t)nch * (W4_UCH * 4u);
    };
    // Start of an item, issued as early as possible -- for the first item here, for every later one BEFORE the previous item's output stage, so that the one
    // exposed round trip (the windows of chunks 0..3) travels under it: first U chunk, the windows of chunk `pairw` into ring slot `pairw` (the ring is free:
    // the K loop ended on a barrier), the sample's styles into their own LDS table (not the one the output stage reads).  Nothing of it needs a register.
    auto begin_item = [&](int sl_, int tg_) {
        set_item_u(sl_);
        issueU(0, 0);
        set_item_x(tg_);
        request(pairw);
        const int b_ = tg_ / (p.gxn * p.gyn);
        // the sample's styles: 64 channels per 4-byte LDS-direct load (waves 2, 3), like everything else requested here WITHOUT a register or a wait of the compiler's
        if (p.styles && (wvx == 2 || (wvx == 3 && p.Cin > 64)))
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds" :: "s"((uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_sty + (uint32_t)(wvx - 2) * 256u))),
                         "v"((uint32_t)(b_ * p.Cin + (wvx - 2) * 64) * 4u + (uint32_t)l * 4u), "s"(ds), "s"(0u) : "memory");
        // the item's 8 x 64-pixel noise patch, by two LDS-direct loads (waves 0 and 1: four rows each) into the patch buffer of this item's parity.  The output
        // stage must hold NO vector-memory load of the compiler's: its wait counts do not know the hand-issued loads, and a `vmcnt(3)` for a noise row also
        // waits for every older LDS-direct load -- the next item's windows, requested just before the output stage precisely so that they travel under it
        // (first form of this kernel: the output stage opened with that wait, and the spill reloads around it with `vmcnt(0)`).
        if (p.e.noise && wvx < 2) {
            const int gx_ = tg_ % p.gxn, gy_ = (tg_ / p.gxn) % p.gyn;
            const uint32_t vo = (uint32_t)(b_ * (int)p.e.noise_bstride + (gy_ * 8 + wvx * 4 + (l >> 4)) * p.W + gx_ * 64) * 4u + (uint32_t)(l & 15) * 16u;
            dma(dn, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_noise + (uint32_t)item_par * 2048u + (uint32_t)wvx * 1024u)), vo, 0u);
        }
        item_par ^= 1;
    };
    if (have) begin_item(sl, tg);
    while (have) {
        const int m0 = sl * 64, gx = tg % p.gxn, gy = (tg / p.gxn) % p.gyn, b = tg / (p.gxn * p.gyn);
        // prologue of the item: the windows of chunks 0..3 (requested by begin_item), one chunk per wave pair, transformed at once
        {
            int tgx = tg;
            asm volatile("" : "+s"(tgx));            // (recomputed here rather than kept live across the previous item's output stage, the register peak of the kernel)
            set_item_x(tgx);
        }
        f32x4 acc[36];
#pragma unroll
        for (int i = 0; i < 36; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        wait_loads();
        lds_barrier();                               // (the styles are in place for every wave)
        // the next ticket (a returning atomic) and the slice's bias / demodulation values are REQUESTED here and used behind the transform: their round trip
        // (1.8 k cycles exposed at the item top, cycle counters of the first build) runs under its ~2 k cycles of arithmetic
        // (the atomic by hand: `atomicAdd` under `tid == 0` becomes the wave-aggregated form, whose `v_readfirstlane` of the result waits for it on the spot.  The
        //  register is increment in, old value out; nothing reads it before the K loop's first chunk-end `vmcnt(0)` -- isa_check looks)
        int t_next = 1;
        float side_v = tid < 64 ? 0.f : 1.f;
        if (tid == 0) asm volatile("global_atomic_add %0, %1, %0, %2 sc0" : "+v"(t_next) : "v"(xcd * 4), "s"(p.ticket) : "memory");
        if (tid < 64) { if (p.e.bias) side_v = p.e.bias[m0 + tid]; }
        else if (tid < 128 && p.e.dcoef) side_v = p.e.dcoef[b * p.e.Cout + m0 + (tid & 63)];
        __builtin_amdgcn_sched_barrier(0);
        transform(pairw);
        __builtin_amdgcn_sched_barrier(0);
        if (tid < 128) side[tid] = side_v;
        lds_barrier();
        // one chunk: 36 MFMAs on U stage c & 1 / V slot c & 3, the U pieces of chunk c + 1 issued one per group behind the first MFMA pair
        auto mfma_chunk = [&](int c) {
            // Stage / slot bases as OPAQUE per-chunk scalars + immediate offsets (g * 2 KB): with the loop unrolled by four the slot of a chunk is a
            // compile-time constant, the V ring lies beyond the 64 KB an LDS immediate reaches, and the compiler then materialises one address register per
            // (slot, group) outside the loop -- 60-odd registers, spilled (seen in the first build's ISA).
            uint32_t uso = (uint32_t)(c & 1) * (W4F_UST * 4u), vso = (uint32_t)(c & 3) * (W4_VCH * 4u);
            uint32_t nus = lds0 + (uint32_t)((c + 1) & 1) * (W4F_UST * 4u);
            asm volatile("" : "+s"(uso), "+s"(vso), "+s"(nus));
            const uint32_t ua_ = a_base + uso, vb_ = b_base + vso;      // (one add per chunk from two loop-invariant lane addresses)
            const int cn = c + 1 < nch ? c + 1 : c;                 // (the last chunk re-requests itself: no branch around the loads)
            f32x4 fa[3], fb[3];
            auto frags = [&](int g, int q) {
                fa[q] = *(lds_f4p)lds_ptr(ua_ + (uint32_t)g * 2048u);
                fb[q] = *(lds_f4p)lds_ptr(vb_ + (uint32_t)g * 2048u);
            };
            frags(0, 0);
            frags(1, 1);
#pragma unroll
            for (int g = 0; g < 9; g++) {
                if (g + 2 < 9) frags(g + 2, (g + 2) % 3);
                __builtin_amdgcn_sched_barrier(0);
                const f32x4 a = fa[g % 3], bb = fb[g % 3];
                acc[4 * g + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bb[0], acc[4 * g + 0], 0, 0, 0);
                acc[4 * g + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bb[1], acc[4 * g + 1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (g < 4 || (g == 4 && wvx < 4)) pieceU(g, cn, nus);
                __builtin_amdgcn_sched_barrier(0);
                acc[4 * g + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bb[2], acc[4 * g + 2], 0, 0, 0);
                acc[4 * g + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bb[3], acc[4 * g + 3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            wait_loads();
            lds_barrier();
            __builtin_amdgcn_sched_barrier(0);
        };
        // The K loop, unrolled by four.  Chunk n >= 4 (slot n & 3, prepared by pair n & 3): its slot is free once chunk n - 4 has been multiplied, so its
        // windows are requested at the top of iteration n - 3 and have landed at that iteration's end (the chunk-end wait covers every LDS-direct load of the
        // wave); the transforms run in two balanced bursts -- pairs 0, 1 (waves 0..3: one per SIMD) at the top of iteration 3 (mod 4) for chunks n = 0, 1 (mod 4)
        // of the next round, pairs 2, 3 (waves 4..7) at the top of iteration 1 for this round's chunks 2, 3.
        for (int c4 = 0; c4 < nch; c4 += 4) {
            const bool more_v = c4 + 4 < nch, later = c4 > 0;
            if (pairw == 3 && later) request(c4 + 3);
            mfma_chunk(c4);
            if (pairw == 0 && more_v) request(c4 + 4);
            if (pairw >= 2 && later) transform(c4 + pairw);
            mfma_chunk(c4 + 1);
            if (pairw == 1 && more_v) request(c4 + 5);
            mfma_chunk(c4 + 2);
            if (pairw == 2 && more_v) request(c4 + 6);
            if (pairw < 2 && more_v) transform(c4 + 4 + pairw);
            mfma_chunk(c4 + 3);
        }
        // the next item: its ticket was drawn at the start; its first U chunk travels under the output stage (both U stages are free)
        int nsl_ = 0, ntg_ = 0;
        const bool more = acquire(t_next, true, nsl_, ntg_);
        if (more) begin_item(nsl_, ntg_);
        int lo = l;
        asm volatile("" : "+v"(lo));                 // (the output stage's lane constants from an opaque copy of the lane id: not live through the K loop)
        const int kq = lo >> 4, l15 = lo & 15;
        const int tt = tr * 16 + l15;
        const int oy = gy * 8 + (tt >> 4) * 4, ox = gx * 64 + (tt & 15) * 4;
        // ---- output transform Y = A^T M A in registers; lane = (4 channels 16 cg + 4 kq + r, tile (tr, l15)) ----
        {
            float4 nz[4];
#pragma unroll
            for (int a = 0; a < 4; a++) nz[a] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.e.noise) {                         // this item's patch: the buffer of the parity it was begun with (`more`: begin_item has flipped it once more)
                const uint32_t nb = lds_noise + (uint32_t)((item_par ^ (more ? 0 : 1)) & 1) * 2048u + (uint32_t)(((tt >> 4) * 4) * 64 + (tt & 15) * 4) * 4u;
#pragma unroll
                for (int a = 0; a < 4; a++) { const f32x4 v = *(lds_f4p)lds_ptr(nb + (uint32_t)a * 256u); nz[a] = make_float4(v[0], v[1], v[2], v[3]); }
            }
            auto write_outputs = [&](auto act_tag) {
                constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int chl = cg * 16 + kq * 4 + r, o = m0 + chl;
                    float t[4][6];
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        const float col[6] = {acc[j][r], acc[6 + j][r], acc[12 + j][r], acc[18 + j][r], acc[24 + j][r], acc[30 + j][r]};
                        float y4[4];
                        wino4_at(col, y4);
#pragma unroll
                        for (int a = 0; a < 4; a++) t[a][j] = y4[a];
                    }
                    const float dd = side[64 + chl], bs = side[chl];
                    float* yp = p.e.y + (((int64_t)b * p.Cout + o) * p.H + oy) * p.W + ox;
#pragma unroll
                    for (int a = 0; a < 4; a++) {
                        float y4[4];
                        wino4_at(t[a], y4);
                        *(float4*)(yp + (int64_t)a * p.W) = finish_act4<ACT>(p.e, make_float4(y4[0], y4[1], y4[2], y4[3]), dd, nz[a], bs);
                    }
                }
            };
            // packed form (linear / leaky ReLU): a channel pair at a time -- modconv_wino4.inc: wino4_output_pair
            auto write_outputs_pk = [&](auto act_tag) {
                constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
                for (int pr = 0; pr < 2; pr++) {
                    const int chl = cg * 16 + kq * 4 + 2 * pr, o = m0 + chl;
                    w4_f2 yy[4][4];
                    wino4_output_pair(acc, pr, yy);
                    const w4_f2 d2 = {side[64 + chl], side[64 + chl + 1]}, b2 = {side[chl], side[chl + 1]};
                    float* yp = p.e.y + (((int64_t)b * p.Cout + o) * p.H + oy) * p.W + ox;
                    const int64_t cs = (int64_t)p.H * p.W;
#pragma unroll
                    for (int a = 0; a < 4; a++) {
                        const float nq[4] = {nz[a].x, nz[a].y, nz[a].z, nz[a].w};
                        w4_f2 f[4];
#pragma unroll
                        for (int i = 0; i < 4; i++) f[i] = finish_pair<ACT>(p.e, yy[a][i], d2, nq[i], b2);
                        *(float4*)(yp + (int64_t)a * p.W) = make_float4(f[0].x, f[1].x, f[2].x, f[3].x);
                        *(float4*)(yp + cs + (int64_t)a * p.W) = make_float4(f[0].y, f[1].y, f[2].y, f[3].y);
                    }
                }
            };
            const int evar = epi_variant(p.e);
            if (evar == 3) write_outputs_pk(std::integral_constant<int, 3>{});
            else if (evar == 1) write_outputs_pk(std::integral_constant<int, 1>{});
            else write_outputs(std::integral_constant<int, 0>{});
            // the noise rows are USED here whatever path ran: a load still pending at the loop's back edge makes the compiler guard its destination registers with
            // vmcnt waits inside the K loop (seen in the ISA of the first packed build: vmcnt(2) / vmcnt(0) at the loop head -- they would also wait for the pieces in flight)
            asm volatile("" :: "v"(nz[0].x), "v"(nz[0].w), "v"(nz[1].x), "v"(nz[1].w), "v"(nz[2].x), "v"(nz[2].w), "v"(nz[3].x), "v"(nz[3].w));
        }
        lds_barrier();                               // `side` and the V ring are free for the next item
        have = more; sl = nsl_; tg = ntg_;
    }
}

// modconv_host.inc -- the host half of modconv.hip (included as its last line: one translation unit, so every kernel template is
// instantiated from here).  In order: the packed-weight layout, the launch helpers of the kernel families, plan_modconv() -- WHICH family a
// call takes, decided once and read by the workspace query, the shape queries and the launch --, the workspace layout, one builder per
// parameter struct, one launcher per path, the exported entry points.

// ---- thresholds of the host side ----
// F(4x4): the batch goes through the two kernels in sub-batches whose V fits one buffer descriptor (< 4 GiB):
// C4's 512^2 x 128 layer at B = 16 has 4.8 GB of V.  The sub-batches share one V buffer (stream order).
constexpr int W4_VCAP_MB = 4095;
// Layers with few channels move 2.25 x their input through V for little arithmetic: there a sub-batch whose V stays inside the 256 MB
// Infinity Cache between the two kernels (W4_VSMALL_MB) beats one big launch (measured B = 16: 256^2 x 128 1.38 (one sample per launch) /
// 1.22 (two) / 1.25 (three) ms; 128^2 x 256 0.93 -> 1.03 ms -- hence Cin <= 128 only, and at least two samples per launch).
constexpr int W4_VSMALL_MB = 192;
constexpr int W4_VSMALL_MINB = 2;         // fewest samples per launch on that path
// Winograd F(2x2) kernel (modconv_wino.inc): below WINO_MIN_CIN the direct kernel's staging economy wins (K = Cin per position instead
// of 9 Cin); measured per layer, see DESIGN.md.
constexpr int WINO_MIN_CIN = 64;

namespace {

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// The packed weights of a layer (tdgp_modconv_pack): six sections in this order.  *_floats: their lengths; wp .. wino4: the float offset at which
// each starts (the ONE place where the lengths are summed); total: floats of the whole buffer.
struct PackInfo {
    int T, KC, CoutP, nchunks, niter16, nch32, nch8, nch4, nsl64;
    int64_t wp_floats, wsq_floats, wsplit_floats, wbf_floats, wino_floats, wino4_floats;
    int64_t wp, wsq, wsplit, wbf, wino, wino4, total;
};
inline PackInfo pack_info(int Cout, int Cin, int k) {
    PackInfo pi;
    pi.T = k * k;
    pi.KC = KC3;
    pi.CoutP = round_up(Cout, 4);
    pi.nchunks = round_up((Cin + pi.KC - 1) / pi.KC, k == 1 ? 16 : 2);      // zero-padded to whole K iterations (1x1 kernels stage up to 16 chunks)
    pi.wp_floats = (int64_t)pi.nchunks * pi.T * pi.KC * pi.CoutP;
    pi.wsq_floats = (int64_t)Cin * pi.CoutP;
    pi.niter16 = (Cin + 15) / 16;
    pi.wsplit_floats = k == 3 ? (int64_t)pi.niter16 * 9 * 3 * pi.CoutP * 8 : 0;      // split-bf16 copy of the 3x3 weights (opt-in arithmetic)
    pi.nch32 = (Cin + 31) / 32;
    pi.wbf_floats = k == 3 ? (int64_t)pi.nch32 * 9 * 2 * pi.CoutP * 8 : 0;          // bf16 copy of the 3x3 weights (reduced-precision blocks)
    pi.nch8 = (Cin + 7) / 8;
    pi.wino_floats = k == 3 ? (int64_t)pi.nch8 * 16 * 2 * pi.CoutP * 4 : 0;          // Winograd-domain weights G g G^T (modconv_wino.inc)
    pi.nch4 = (Cin + 3) / 4; pi.nsl64 = (Cout + 63) / 64;
    pi.wino4_floats = (k == 3 && Cin >= W4_MIN_C && Cout >= W4_MIN_C) ? (int64_t)cdiv(Cout, W4_BM) * pi.nch4 * W4_UCH : 0;      // F(4x4,3x3)-domain weights (modconv_wino4.inc)
    pi.wp = 0;
    pi.wsq = pi.wp + pi.wp_floats;
    pi.wsplit = pi.wsq + pi.wsq_floats;
    pi.wbf = pi.wsplit + pi.wsplit_floats;
    pi.wino = pi.wbf + pi.wbf_floats;
    pi.wino4 = pi.wino + pi.wino_floats;
    pi.total = pi.wino4 + pi.wino4_floats;
    return pi;
}

// pixel tiles of a launch whose blocks cover NT 32-pixel subtiles
inline int px_tiles(const ConvParams& p, int NT) {
    const int TW = 1 << p.tw_log2, RPS = 32 >> p.tw_log2, TR = NT * RPS;
    return cdiv(p.ph.gridW, TW) * cdiv(p.B * p.ph.gridH, TR);
}

// Split-K factor: low-resolution layers have K = Cin*9 = 4608 but only a handful of output tiles, so a plain launch
// leaves most of the 256 CUs idle behind a 64-iteration serial K loop.  Split K until ~2 blocks per CU exist.
inline int pick_ksplit(int blocks, int niter) {
    if (blocks >= 256 || niter < 4) return 1;
    int ks = cdiv(512, blocks);
    if (ks > niter / 2) ks = niter / 2;
    if (ks > 32) ks = 32;
    return ks < 1 ? 1 : ks;
}

template <int MTW, int NTW, int WM, int WN, int KCS, int MAXT>
int launch_conv(ConvParams& p, float* partial, int64_t partial_floats, hipStream_t s) {
    constexpr int BM = 32 * MTW * WM, NT = NTW * WN, BN = 32 * NT;
    constexpr int HALO = MAXT == 25 ? 2 : 1;
    constexpr int XS_MAX = (BN / 4 + 2 * HALO) * (4 + 2 * HALO) > (BN / 32 + 2 * HALO) * (32 + 2 * HALO) ? (BN / 4 + 2 * HALO) * (4 + 2 * HALO) : (BN / 32 + 2 * HALO) * (32 + 2 * HALO);
    const size_t lds = (size_t)(2 * (MAXT * KCS * BM + KCS * XS_MAX + 64) + 32 + 5 * BM) * sizeof(float);
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)conv_mfma_kernel<MTW, NTW, WM, WN, KCS, MAXT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds););   // raise the dynamic-LDS cap once per instantiation and device
    const int gx = px_tiles(p, NT), gy = cdiv(p.Cout, BM);
    const int niter = cdiv(cdiv(p.Cin, KC3), KCS / KC3);
    const int64_t slice = (int64_t)p.e.B * p.e.Cout * p.e.Hout * p.e.Wout;
    int ks = pick_ksplit(gx * gy, niter);
    while (ks > 1 && ks * slice > partial_floats) ks--;          // never exceed the caller's workspace
    p.ksplit = ks;
    p.partial = partial;
    dim3 grid(gx, gy, ks);
    TDGP_LAUNCH("conv_mfma_kernel", (conv_mfma_kernel<MTW, NTW, WM, WN, KCS, MAXT>), grid, dim3(256), lds, s, p);
    if (ks > 1)
        TDGP_LAUNCH("splitk_reduce_kernel", splitk_reduce_kernel, dim3((int)min((int64_t)2048, cdiv64(slice, 256))), dim3(256), 0, s, partial, ks, p.e);
    return 0;
}

// Split-K for launches that already fill the chip: tail balancing.  512 block slots (2 blocks per CU); a launch of n blocks
// runs n / 512 full rounds plus a tail that costs ~0.7 of a round when <= 256 blocks are left (one block per CU runs faster)
// -- e.g. 560 blocks are 1.7 rounds for 1.09 rounds of work.  Splitting K by ks shrinks the rounds; each extra slice costs
// one more pass over the partial sums (~4 TB/s, mostly served by the 256 MB MALL).  Times in microseconds at ~100 TFLOP/s of
// block throughput.
inline int tail_ksplit(int blocks, int niter, double flop, int64_t slice_floats, int max_ks) {
    double best = 1e30;
    int ks = 1;
    for (int k = 1; k <= max_ks && k <= 4 && niter / k >= 16; k++) {
        const int n = blocks * k, full = n / 512, rem = n % 512;
        const double rounds = full + (rem == 0 ? 0.0 : (rem <= 256 ? 0.7 : 1.0));
        const double t = rounds * (flop / n) / (100e12 / 512) * 1e6 + (k - 1) * (double)slice_floats * 4.0 / 4e12 * 1e6;
        if (t < best * 0.97) { best = t; ks = k; }
    }
    return ks;
}

// x2 layers: tile configuration, split-K factor and Z geometry -- shared by the workspace query and the launch.
struct UpPlan { int cfg, BM, BN, G1, GS, ksplit; int64_t zslice; };
inline UpPlan up_plan(int B, int Cin, int Cout, int H, int W) {
    UpPlan u;
    u.cfg = Cout > 64 ? 0 : 1;
    u.BM = Cout > 64 ? 128 : 64; u.BN = Cout > 64 ? 64 : 128;
    u.G1 = W + 2;                  // grid pitch: W + 1 would do (one zero column); W + 2 makes the Z row pitch 2*G1 a multiple of 4 floats -> 16-B FIR loads
    u.GS = round_up((H + 1) * (W + 2), 32);
    u.zslice = (int64_t)B * Cout * 4 * u.GS;
    const int blocks = cdiv(B * u.GS, u.BN) * cdiv(Cout, u.BM);
    const int niter = cdiv(Cin, 4);
    int ks;
    if (blocks < 256) {
        ks = pick_ksplit(blocks, niter);
        const int64_t cap = ((int64_t)64 << 20) / 4;             // low-resolution layers: at most 64 MiB of slices
        while (ks > 1 && ks * u.zslice > cap) ks--;
    } else {
        ks = tail_ksplit(blocks, niter, 2.0 * Cin * Cout * 9.0 * H * W * B, u.zslice, 4);
    }
    u.ksplit = ks;
    return u;
}

template <int MTW, int NTW, int WM, int WN, bool DEEP>
void launch_upconv(const UpParams& u, hipStream_t s) {
    constexpr int BM = 32 * MTW * WM, BN = 32 * NTW * WN, NW = WM * WN;
    constexpr int stage = 2 * (9 * BM * 4 + 2 * (BN + 2) * 4), epi = NW * 32 * UP_CT_W;
    const size_t lds = (size_t)(stage > epi ? stage : epi) * sizeof(float);
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)upconv_mfma_kernel<MTW, NTW, WM, WN, DEEP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds););
    dim3 grid(cdiv(u.B * u.GS, BN), cdiv(u.Cout, BM), u.ksplit);
    TDGP_LAUNCH("upconv_mfma_kernel", (upconv_mfma_kernel<MTW, NTW, WM, WN, DEEP>), grid, dim3(64 * NW), lds, s, u);
}

template <int MT, bool RESIDENT, bool FAST, bool XBF>
void launch_torgb_v(const RgbParams& r, hipStream_t s) {
    constexpr int BM = 32 * MT;
    const size_t lds = (size_t)(16 * BM * 4 + 16 * 128 * 4 + BM) * sizeof(float);
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)torgb_mfma_kernel<MT, RESIDENT, FAST, XBF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds););
    // RESIDENT: several consecutive tiles per block once there are more tiles than ~4 rounds of the 512 resident blocks
    RgbParams rr = r;
    const int64_t ntiles = cdiv64(r.P, 128);
    if constexpr (RESIDENT && FAST && !XBF) {
        // the two-role form: enough tiles for >= 16 per block on a grid of four blocks per CU (C3 / C4: the 512^2 layer; at B = 1 the 512^2 layer still has 2048 tiles)
        const int cus = tdgp_cu_count();
        if (r.e.skip && ntiles >= (int64_t)cus * 8) {
            constexpr size_t lds_ws = (size_t)(16 * BM * 4 + 2 * 16 * 128 * 4 + 4 * MT * 32 * CT_LD + BM) * sizeof(float);
            TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)torgb_ws_kernel<MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ws););
            const int64_t blocks = (int64_t)cus * 4;
            rr.tpb = (int)cdiv64(ntiles, blocks);
            TDGP_LAUNCH("torgb_mfma_kernel", (torgb_ws_kernel<MT>), dim3((unsigned)cdiv64(ntiles, rr.tpb)), dim3(512), lds_ws, s, rr);
            return;
        }
    }
    rr.tpb = RESIDENT ? (int)max((int64_t)1, min((int64_t)8, ntiles / 2048)) : 1;
    TDGP_LAUNCH("torgb_mfma_kernel", (torgb_mfma_kernel<MT, RESIDENT, FAST, XBF>), dim3((unsigned)cdiv64(ntiles, rr.tpb)), dim3(256), lds, s, rr);
}

template <int MT, bool XBF = false>
void launch_torgb(const RgbParams& r, hipStream_t s) {
    const bool fast = r.lw >= 0 && r.e.clamp < 0.f && r.e.gain == 1.f;
    if constexpr (XBF) {                                    // the reduced-precision blocks always clamp: one output stage
        if (r.Cin <= 64) launch_torgb_v<MT, true, false, true>(r, s); else launch_torgb_v<MT, false, false, true>(r, s);
    } else {
        if (r.Cin <= 64) { if (fast) launch_torgb_v<MT, true, true, false>(r, s); else launch_torgb_v<MT, true, false, false>(r, s); }
        else { if (fast) launch_torgb_v<MT, false, true, false>(r, s); else launch_torgb_v<MT, false, false, false>(r, s); }
    }
}

// KS x KS stride-1 fast path (W % 32 == 0)
template <int KS, int MTW, int NTW, int WM, int WN>
int launch_conv3(Conv3Params& p, float* partial, int64_t partial_floats, hipStream_t s) {
    constexpr int BM = 32 * MTW * WM, NT = NTW * WN, R = KS / 2;
    constexpr int stage = 2 * (KS * KS * BM * 4 + (NT + 2 * R) * (32 + 2 * R) * 4) + 5 * BM, epi = 4 * 32 * CT_LD;
    const size_t lds = (size_t)(stage > epi ? stage : epi) * sizeof(float);
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)conv3_mfma_kernel<KS, MTW, NTW, WM, WN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds););
    const int gx = (p.W >> 5) * cdiv(p.B * (p.H + R), NT), gy = cdiv(p.Cout, BM);
    const int niter = cdiv(p.Cin, 4);
    const int64_t slice = (int64_t)p.B * p.Cout * p.H * p.W;
    const int max_ks = (int)min((int64_t)32, partial_floats / slice);
    int ks = gx * gy < 256 ? pick_ksplit(gx * gy, niter) : tail_ksplit(gx * gy, niter, 2.0 * p.Cin * p.Cout * KS * KS * p.H * p.W * p.B, 2 * slice, max_ks);
    if (ks > max_ks) ks = max_ks;
    if (ks < 1) ks = 1;
    p.ksplit = ks;
    p.partial = partial;
    TDGP_LAUNCH("conv_mfma_kernel", (conv3_mfma_kernel<KS, MTW, NTW, WM, WN>), dim3(gx, gy, ks), dim3(256), lds, s, p);
    if (ks > 1)
        TDGP_LAUNCH("splitk_reduce_kernel", splitk_reduce_kernel, dim3((int)min((int64_t)2048, cdiv64(slice, 256))), dim3(256), 0, s, partial, ks, p.e);
    return 0;
}

inline int pick_tw_log2(int gridW) {
    int tw = 4, lg = 2;
    while (tw < 32 && tw < gridW) { tw <<= 1; lg++; }
    return lg;
}

// F(4x4,3x3) Winograd (modconv_wino4.inc): which stride-1 3x3 layers take it -- by shape only (the workspace is sized from the same test).
// whole tile groups of 512 pixels (64 x 8, or 32 x 16 for the 32-pixel-wide layers); Cin, Cout >= 128: below, the separate input-transform pass (2.25 x the input, written and
// read back) costs more than it saves; at least one item per CU; V addressed through a 4 GiB buffer descriptor.
inline int64_t wino4_v_bytes(int B, int Cin, int H, int W) { return (int64_t)B * ((H * W) >> 9) * ((Cin + 3) / 4) * (9 * 4 * 32 * 4) * 4; }       // 512 pixels per tile group
inline int wino4_txl(int H, int W) { return (W & 63) == 0 && (H & 7) == 0 ? 4 : ((W & 31) == 0 && (H & 15) == 0 ? 3 : 0); }
inline int64_t wino4_items(int bs, int Cout, int H, int W) { return (int64_t)bs * ((H * W) >> 9) * cdiv(Cout, 64); }
inline int wino4_sub_batch(int B, int Cin, int Cout, int H, int W) {
    const int64_t per = wino4_v_bytes(1, Cin, H, W);
    if (Cin <= 128) {
        const int bs = (int)std::min<int64_t>(B, ((int64_t)W4_VSMALL_MB << 20) / per);
        if (bs >= W4_VSMALL_MINB && wino4_items(bs, Cout, H, W) >= 256) return bs;      // (one sample per launch -- 512^2 x 64: 151 MB of V next to 134 MB of x and y -- does not stay in the cache anyway: 1.84 vs 1.77 ms for the whole batch at once)
    }
    return (int)std::min<int64_t>(B, ((int64_t)W4_VCAP_MB << 20) / per);
}
// Launches with too few items for the chip (the 32^2 layers at batch 4 .. 8) split the input channels of every item 2 or 4 ways (plain layers
// only; >= 16 chunks per split; the whole batch in one launch); the splits' raw sums go through the split-K buffer of the direct kernels.
// 0 = not a split-K shape.  B = 4, 32^2 x 512: direct sums 0.235 ms -> 4 splits (measured, DESIGN.md).
inline int wino4_ksplit_log2(int B, int Cin, int Cout, int H, int W) {
    if (wino4_v_bytes(B, Cin, H, W) > ((int64_t)W4_VSMALL_MB << 20)) return 0;
    const int64_t base = wino4_items(B, Cout, H, W);
    const int nch = Cin >> 2;
    for (int l = 1; l <= 2; l++)
        if ((base << l) >= 256 && (nch & ((1 << l) - 1)) == 0 && (nch >> l) >= 16) return l;
    return 0;
}
inline bool wino4_shape_ok(int B, int Cin, int Cout, int H, int W, int k, int up, bool plain = false) {
    if (!(k == 3 && up == 1 && wino4_txl(H, W) != 0 && (Cin & 3) == 0 && Cin >= W4_MIN_C && Cout >= W4_MIN_C)) return false;
    const int bs = wino4_sub_batch(B, Cin, Cout, H, W);
    if (bs >= 1 && wino4_items(bs, Cout, H, W) >= 256) return true;
    return plain && wino4_items(B, Cout, H, W) < 256 && wino4_ksplit_log2(B, Cin, Cout, H, W) > 0;
}

// Winograd F(2x2) kernel (modconv_wino.inc): which stride-1 3x3 layers take it.
inline size_t wino_lds_bytes(int) { return (size_t)(2 * 8192 + 2 * 8192 + 2 * 8 * 10 * 48 + 128) * 4; }
inline bool wino_ok(int B, int Cin, int Cout, int H, int W) {
    // (fewer than one block per CU: the direct kernel's split-K fills the chip better)
    return (W & 31) == 0 && (H & 7) == 0 && (Cin & 7) == 0 && Cin >= WINO_MIN_CIN && wino_lds_bytes(Cin) <= 160 * 1024 &&
           (int64_t)(W >> 5) * (H >> 3) * B * cdiv(Cout, 64) >= 256;
}

// x, y and the noise map of a call aligned for the vector loads and stores of the Winograd kernels: `a` = 16 bytes (F(4x4)) or 8 (F(2x2): 8-byte
// noise loads / stores; its activation loads are 16-byte all the same).  The noise batch stride is a multiple of a / 4 floats.
inline bool noise_aligned(const float* noise, int64_t noise_bstride, int a) { return !noise || (((uintptr_t)noise & (a - 1)) == 0 && (noise_bstride & (a / 4 - 1)) == 0); }
inline bool io_aligned(const void* x, const void* y, const float* noise, int64_t noise_bstride, int a) {
    return ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & (a - 1)) == 0 && noise_aligned(noise, noise_bstride, a);
}

int g_conv_arith = 0;                  // tdgp_set_conv_arith
inline bool arith_wino4(int arith) { return arith == 0 || arith == 4; }

// ---- the launch plan ----
// What plan_modconv needs of a call: the shape, and the facts only the call can see.  aligned16 / aligned8: io_aligned(x, y, noise, stride, 16 / 8).
struct ConvCall {
    int B, Cin, Cout, H, W, k, up, out_layout, out_feat;
    bool has_styles, has_skip, has_noise, demodulate;
    int act;
    float alpha, gain, clamp;
    bool aligned16, aligned8;
    int arith;                         // tdgp_set_conv_arith mode
};
// Which kernel family the call takes and the numbers its launcher needs.  The CU-dependent grid geometry is not in here (xcd_rect at launch;
// the two-role ToRGB form and RESIDENT / FAST are decided in launch_torgb, which the reduced-precision entry shares).
struct ConvPlan {
    int path;                          // tdgp_conv_path
    int tile;                          // direct / conv3 kernels: output channels per block 0 = 64 (1 x 4 waves), 1 = 128 (2 x 2 waves), 2 = 96 (1 x 1 kernels with 64 < Cout <= 96)
    int bsub, ksl;                     // F(4x4): samples per launch; log2 of the K split
    UpPlan up; bool up_split; int fir_tile;      // x2: Z geometry and split-K; split-bf16 arithmetic; tile form of the FIR pass
    int rgb_mt;                        // ToRGB: 32-row MFMA tiles of output channels per block
};

// split-K buffer of the stride-1 layers, in floats: split-K is only chosen for launches with < 256 blocks: bound its buffer at 32 slices and 64 MiB
inline int64_t splitk_floats(int64_t out_elems) {
    int64_t pf = out_elems * 32;
    const int64_t cap = ((int64_t)64 << 20) / 4;
    if (pf > cap) pf = (cap / out_elems) * out_elems;
    return pf;
}

// FIR pass of the x2 layers: the tile form, chosen once for the fp32 and the bf16 output (which has no 4-adjacent-rows instantiation).
enum FirTile { FIR_32x128_ADJ, FIR_16x128_LRELU, FIR_16x128, FIR_32x64 };
inline int fir_tile(int OH, int OW, int ksplit, int act, float alpha, bool bf16_out) {
    const bool lrelu = act == 3 && alpha >= 0.f && alpha <= 1.f;
    if (!bf16_out && OW >= 128 && (OH & 31) == 0 && ksplit == 1 && lrelu) return FIR_32x128_ADJ;
    if (OW >= 128) return lrelu ? FIR_16x128_LRELU : FIR_16x128;
    return FIR_32x64;
}

// The F(4x4) kernels take the call: arithmetic mode, shape (plain layers may split K) and alignment.  Also the acceptance test of out_layout 2.
inline bool wino4_takes(const ConvCall& c) {
    return arith_wino4(c.arith) && wino4_shape_ok(c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.up, c.out_layout == 0) && c.aligned16;
}

// Pure: no HIP call, no launch, no pointer read -- the same answer for the workspace bound, the shape queries and the launch.  Expects a call that
// passed the argument checks of tdgp_modconv2d.  Branch order and thresholds are the dispatch's as measured (DESIGN.md); the first match wins.
ConvPlan plan_modconv(const ConvCall& c) {
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W, k = c.k, up = c.up;
    ConvPlan p{};
    p.tile = Cout > 64 ? 1 : 0;
    if (up == 2) {
        // transposed conv, stride 2 -> parity-planar Z -> FIR + output stage; opt-in split-bf16 arithmetic (tdgp_set_conv_arith(1)): same Z, one slice
        p.path = TDGP_PATH_UP;
        p.up = up_plan(B, Cin, Cout, H, W);
        const int s_blocks = cdiv(B * p.up.GS, 128) * cdiv(Cout, 64);
        p.up_split = c.arith == 1 && s_blocks >= 256 && c.has_styles && (Cin & 15) == 0 && Cin <= 2048 && p.up.GS >= 2 * (128 + p.up.G1 + 2);
        p.fir_tile = fir_tile(2 * H, 2 * W, p.up_split ? 1 : p.up.ksplit, c.act, c.alpha, false);
    } else if (k >= 3 && (W & 31) == 0) {
        const bool w4_weights = pack_info(Cout, Cin, k).wino4_floats > 0;
        if (k == 3 && c.arith == 1 && (W >> 5) * cdiv(B * (H + 1), 8) * cdiv(Cout, 64) >= 256 && c.has_styles && (Cin & 15) == 0 && Cin <= 2048 && H >= 16) {
            p.path = TDGP_PATH_SPLIT3;
        } else if (c.arith == 0 && c.out_layout == 0 && Cin <= W4F_MAXCIN && (Cin & 15) == 0 && (Cout & 63) == 0 && wino4_txl(H, W) == 4 &&
                   wino4_shape_ok(B, Cin, Cout, H, W, k, up) && w4_weights && (int64_t)B * ((H * W) >> 9) * (Cout >> 6) >= 256 && !c.has_skip && c.aligned16) {
            // few input channels (the 256^2 / 512^2 blocks): the input transform runs inside the GEMM kernel, V never leaves the CU (modconv_wino4f.inc)
            p.path = TDGP_PATH_WINO4F;
        } else if (wino4_takes(c) && w4_weights && (c.out_layout == 0 || c.out_layout == 2) && !c.has_skip) {
            // K split (too few items for the chip): only when the unsplit shape does not qualify, the split-K buffer holds the slices, plain layers
            int ksl = (c.out_layout == 0 && !wino4_shape_ok(B, Cin, Cout, H, W, k, up)) ? wino4_ksplit_log2(B, Cin, Cout, H, W) : 0;
            const int64_t kslice = (int64_t)B * Cout * H * W;
            if ((kslice << ksl) > splitk_floats(kslice)) ksl = 0;           // (cannot happen for shapes under 256 items: 4 splits x 255 items x 32768 floats < the 64 MiB buffer; unsplit is still correct)
            p.ksl = ksl;
            p.bsub = ksl ? B : wino4_sub_batch(B, Cin, Cout, H, W);
            p.path = c.out_layout == 2 ? TDGP_PATH_WINO4_FOLDED : (ksl ? TDGP_PATH_WINO4_SPLITK : TDGP_PATH_WINO4);
        } else if (k == 3 && (arith_wino4(c.arith) || c.arith == 3) && wino_ok(B, Cin, Cout, H, W) && c.out_layout == 0 && !c.has_skip && c.aligned8) {
            p.path = TDGP_PATH_WINO2;
        } else {
            p.path = TDGP_PATH_CONV3;
        }
    } else if (k == 3 || k == 5) {
        p.path = TDGP_PATH_DIRECT;
    } else if (c.out_layout == 1 && Cout <= 96 && !c.demodulate && !c.has_noise && c.act == 1 && ((H * W) & 3) == 0) {
        p.path = TDGP_PATH_TORGB;
        p.rgb_mt = Cout <= 32 ? 1 : (Cout <= 64 ? 2 : 3);
    } else {
        p.path = TDGP_PATH_CONV1;
        if (Cout > 64 && Cout <= 96) p.tile = 2;
    }
    return p;
}

// Workspace layout: [demod coefficients B*Cout] [transposed-conv intermediate, up=2 only] [split-K partial sums] [Winograd-domain input V] [item counters]
// The workspace query knows the shape, not the arithmetic mode, the alignment or the output layout of the call that will come: the size is an
// UPPER BOUND over every path plan_modconv can give the shape.  V and the item counters are reserved where wino4_shape_ok(.., plain = true) holds --
// the shape test of every F(4x4) branch of plan_modconv with its widest argument -- so the fused-transform path, which never writes V, still
// reserves it: arithmetic mode 4 runs the same shape through V.
struct WsLayout { int64_t dco, z, partial, partial_floats, wino_v, ticket, total; };
WsLayout ws_layout(int B, int Cin, int Cout, int H, int W, int k, int up) {
    WsLayout w;
    auto al = [](int64_t v) { return (v + 255) / 256 * 256; };
    w.dco = 0;
    w.z = al((int64_t)B * Cout * sizeof(float));
    if (up == 2) {
        // the parity-planar transposed-conv intermediate (x its split-K slices); the FIR kernel reduces the slices itself
        const UpPlan u = up_plan(B, Cin, Cout, H, W);
        w.partial = w.z + al(u.zslice * u.ksplit * (int64_t)sizeof(float));
        w.partial_floats = 0;
        w.wino_v = w.ticket = w.total = w.partial;
        return w;
    }
    w.partial = w.z;
    w.partial_floats = splitk_floats((int64_t)B * Cout * H * W);
    w.wino_v = w.ticket = w.total = w.partial + al(w.partial_floats * (int64_t)sizeof(float));
    if (wino4_shape_ok(B, Cin, Cout, H, W, k, up, true)) {
        w.ticket = w.wino_v + al(wino4_v_bytes(wino4_sub_batch(B, Cin, Cout, H, W), Cin, H, W));
        w.total = w.ticket + 256;
    }
    return w;
}
inline int* ticket_ptr(void* ws, const WsLayout& wl) { return (int*)((char*)ws + wl.ticket); }      // the item counters of the persistent F(4x4) grids

// Persistent F(4x4) grids: the blocks of an XCD (b, b + 8, ...) take a rectangle of rs slices x rt tile groups per pass: per pass an XCD's L2 then
// fetches rs U slices + rt V tile groups instead of one of each per block (bytes ~ rs * BM + rt * tpi: a slice's U chunk : a tile group's V chunk).
// nsl slices of BM output channels, bpc resident blocks per CU, tpi tiles per item.  The grid is nxcd * per blocks.
struct XcdRect { int nxcd, per, rs, rt; };
inline XcdRect xcd_rect(int nsl, int bpc, int BM, int tpi) {
    XcdRect r;
    const int cus = tdgp_cu_count();
    r.nxcd = (cus % 8 == 0 && cus >= 64) ? 8 : 1;
    r.per = cus / r.nxcd * bpc;
    int rs = 1;
    while (rs * 2 <= nsl && (r.per % (rs * 2)) == 0 && (rs * 2) * BM + r.per / (rs * 2) * tpi < rs * BM + r.per / rs * tpi) rs *= 2;
    r.rs = rs; r.rt = r.per / rs;
    return r;
}

// ---- one builder per parameter struct ----
// Output stage.  fir4x4 is a HOST pointer (the filter is a static 64-byte buffer; reading it on the host keeps the call async).
inline EpiParams make_epi(const ConvCall& c, const float* fir4x4, const float* dco, const float* noise, int64_t noise_bstride, const float* bias, const float* skip,
                          float* y, int round_bf16) {
    EpiParams e;
    e.B = c.B; e.Cout = c.Cout; e.round_bf16 = round_bf16;
    for (int i = 0; i < 16; i++) e.fir[i] = 0.f;
    if (fir4x4)
        for (int ky = 0; ky < 4; ky++)
            for (int kx = 0; kx < 4; kx++) e.fir[ky * 4 + kx] = fir4x4[(3 - ky) * 4 + (3 - kx)] * 4.0f;   // no flip_filter: taps = flipped f; gain up^2
    e.dcoef = dco; e.noise = noise; e.noise_bstride = noise_bstride; e.bias = bias; e.skip = skip; e.y = y;
    e.Hout = c.H * c.up; e.Wout = c.W * c.up; e.out_layout = c.out_layout; e.out_feat = c.out_feat > 0 ? c.out_feat : 1;
    e.act = c.act; e.alpha = c.alpha; e.gain = c.gain; e.clamp = c.clamp;
    return e;
}

inline RgbParams make_rgb(const ConvCall& c, const PackInfo& pi, const float* x, uint32_t x_bytes, const float* wp, const float* styles, const EpiParams& e) {
    const int B = c.B, H = c.H, W = c.W;
    RgbParams r;
    r.x = x; r.wp = wp; r.styles = styles; r.e = e;
    r.B = B; r.Cin = c.Cin; r.Cout = c.Cout; r.CoutP = pi.CoutP; r.HW = H * W; r.W = W; r.P = (int64_t)B * H * W;
    r.lw = r.lhw = -1;
    if ((W & (W - 1)) == 0 && (H & (H - 1)) == 0 && (int64_t)B * H * W < ((int64_t)1 << 31) - 512) {
        r.lw = 0; while ((1 << r.lw) < W) r.lw++;
        r.lhw = 0; while ((1 << r.lhw) < H * W) r.lhw++;
    }
    r.x_bytes = x_bytes; r.wp_bytes = (uint32_t)(pi.wp_floats * 4); r.st_bytes = (uint32_t)((int64_t)B * c.Cin * 4);
    return r;
}

inline UpParams make_up(int B, int Cin, int Cout, int H, int W, const PackInfo& pi, const UpPlan& pl, const float* x, const float* wp, const float* styles, float* z) {
    UpParams u;
    u.x = x; u.wp = wp; u.styles = styles; u.z = z;
    u.B = B; u.Cin = Cin; u.Cout = Cout; u.CoutP = pi.CoutP; u.H = H; u.W = W; u.G1 = pl.G1; u.GS = pl.GS; u.ksplit = pl.ksplit; u.zslice = pl.zslice;
    u.x_bytes = (uint32_t)((int64_t)B * Cin * H * W * 4); u.wp_bytes = (uint32_t)(pi.wp_floats * 4); u.st_bytes = (uint32_t)((int64_t)B * Cin * 4);
    return u;
}

// FIR + output stage of a x2 layer over Z; everything of the output stage comes from `e` (e.y is the bf16 output when bf16_out).  ksplit: slices of Z to reduce.
inline FirParams make_fir(const EpiParams& e, const float* z, const UpPlan& pl, int H, int W, int ksplit, bool bf16_out) {
    FirParams f;
    f.z = z; f.dcoef = e.dcoef; f.noise = e.noise; f.noise_bstride = e.noise_bstride; f.bias = e.bias;
    f.y = bf16_out ? nullptr : e.y; f.y16 = bf16_out ? (uint16_t*)e.y : nullptr;
    f.noise_vec = e.noise && noise_aligned(e.noise, e.noise_bstride, 16);
    for (int i = 0; i < 16; i++) f.fir[i] = e.fir[i];
    f.B = e.B; f.C = e.Cout; f.ZROWS = 2 * H + 2; f.P2 = 2 * pl.G1; f.GS2 = 2 * pl.GS; f.ksplit = ksplit; f.zslice = pl.zslice;
    f.OH = 2 * H; f.OW = 2 * W;
    f.act = e.act; f.alpha = e.alpha; f.gain = e.gain; f.clamp = e.clamp;
    return f;
}

// ---- one launcher per path ----
template <int TH, int TW, bool BF, bool LRELU = false, bool ADJ = false>
void launch_fir_tile(const FirParams& f, hipStream_t s) {
    const int64_t ntiles = (int64_t)f.B * f.C * cdiv(f.OH, TH) * cdiv(f.OW, TW);
    TDGP_LAUNCH("fir_act_kernel", (fir_act_kernel<TH, TW, BF, LRELU, ADJ>), dim3((int)min((int64_t)(256 * 32), ntiles)), dim3(256), 0, s, f);
}
void launch_fir(const FirParams& f, int tile, bool bf16_out, hipStream_t s) {
    if (bf16_out) {
        if (tile == FIR_16x128_LRELU) launch_fir_tile<16, 128, true, true>(f, s);
        else if (tile == FIR_16x128) launch_fir_tile<16, 128, true>(f, s);
        else launch_fir_tile<32, 64, true>(f, s);
    } else {
        if (tile == FIR_32x128_ADJ) launch_fir_tile<32, 128, false, true, true>(f, s);
        else if (tile == FIR_16x128_LRELU) launch_fir_tile<16, 128, false, true>(f, s);
        else if (tile == FIR_16x128) launch_fir_tile<16, 128, false>(f, s);
        else launch_fir_tile<32, 64, false>(f, s);
    }
}

// demodulation coefficients of a call: precomputed (tdgp_demod_batch), computed here into the workspace, or none
inline const float* demod_coefs(int demodulate, const float* dcoef_in, const float* styles, const float* wsq, float* dco, int B, int Cin, int Cout, int CoutP, hipStream_t s) {
    if (demodulate && dcoef_in) return dcoef_in;
    if (!demodulate) return nullptr;
    TDGP_LAUNCH("demod_kernel", demod_kernel, dim3(cdiv(Cout, 64), B), dim3(1024), 0, s, styles, wsq, dco, B, Cin, Cout, CoutP);
    return dco;
}

// What the launchers of tdgp_modconv2d share: the call, its plan, the two layouts, the tensors and the output stage.
struct ConvLaunch {
    ConvCall c; ConvPlan plan; PackInfo pi; WsLayout wl;
    const float *x, *wp, *styles;
    EpiParams e;
    char* ws;
    hipStream_t s;
    float* z() const { return (float*)(ws + wl.z); }
    float* partial() const { return (float*)(ws + wl.partial); }
    float* vbuf() const { return (float*)(ws + wl.wino_v); }
    uint32_t x_bytes() const { return (uint32_t)((int64_t)c.B * c.Cin * c.H * c.W * 4); }
    uint32_t st_bytes() const { return (uint32_t)((int64_t)c.B * c.Cin * 4); }
};

void launch_direct(const ConvLaunch& L) {
    const ConvCall& c = L.c;
    const int k = c.k, tile = L.plan.tile;
    ConvParams p;
    p.x = L.x; p.wp = L.wp; p.styles = L.styles; p.B = c.B; p.Cin = c.Cin; p.Cout = c.Cout; p.CoutP = L.pi.CoutP; p.Hin = c.H; p.Win = c.W;
    p.T = L.pi.T; p.ksplit = 1; p.partial = nullptr; p.e = L.e;
    TapTable& ph = p.ph;
    ph.ntaps = k * k; ph.halo = k / 2;
    for (int t = 0; t < k * k; t++) {
        ph.tap_w[t] = t;
        ph.tap_off_y[t] = t / k - k / 2;                 // correlation, padding k/2 (conv2d_resample.py:132-134)
        ph.tap_off_x[t] = t % k - k / 2;
    }
    ph.gridH = c.H; ph.gridW = c.W;
    p.tw_log2 = pick_tw_log2(c.W);
    float* partial = L.partial();
    const int64_t pf = L.wl.partial_floats;
    if (k == 3) {
        if (tile) launch_conv<2, 2, 2, 2, 4, 9>(p, partial, pf, L.s);
        else launch_conv<2, 2, 1, 4, 4, 9>(p, partial, pf, L.s);
    } else if (k == 5) {
        if (tile) launch_conv<2, 2, 2, 2, 4, 25>(p, partial, pf, L.s);
        else launch_conv<2, 2, 1, 4, 4, 25>(p, partial, pf, L.s);
    } else {
        if (tile == 2) launch_conv<3, 1, 1, 4, 32, 1>(p, partial, pf, L.s);
        else if (tile) launch_conv<2, 2, 2, 2, 16, 1>(p, partial, pf, L.s);
        else launch_conv<2, 2, 1, 4, 16, 1>(p, partial, pf, L.s);
    }
}

void launch_conv3_path(const ConvLaunch& L) {
    const ConvCall& c = L.c;
    Conv3Params q;
    q.x = L.x; q.wp = L.wp; q.styles = L.styles; q.partial = nullptr; q.e = L.e;
    q.B = c.B; q.Cin = c.Cin; q.Cout = c.Cout; q.CoutP = L.pi.CoutP; q.H = c.H; q.W = c.W; q.ksplit = 1;
    q.x_bytes = L.x_bytes(); q.wp_bytes = (uint32_t)(L.pi.wp_floats * 4); q.st_bytes = L.st_bytes();
    if (c.k == 3) {
        if (L.plan.tile) launch_conv3<3, 2, 2, 2, 2>(q, L.partial(), L.wl.partial_floats, L.s);
        else launch_conv3<3, 2, 2, 1, 4>(q, L.partial(), L.wl.partial_floats, L.s);
    } else {
        if (L.plan.tile) launch_conv3<5, 2, 2, 2, 2>(q, L.partial(), L.wl.partial_floats, L.s);
        else launch_conv3<5, 2, 2, 1, 4>(q, L.partial(), L.wl.partial_floats, L.s);
    }
}

void launch_split3(const ConvLaunch& L) {
    const ConvCall& c = L.c;
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W;
    Conv3sParams q;
    q.x = L.x; q.wsp = L.wp + L.pi.wsplit; q.styles = L.styles; q.e = L.e;
    q.B = B; q.Cin = Cin; q.Cout = Cout; q.CoutP = L.pi.CoutP; q.H = H; q.W = W;
    q.x_bytes = L.x_bytes(); q.wsp_bytes = (uint32_t)(L.pi.wsplit_floats * 4); q.st_bytes = L.st_bytes();
    const size_t lds = (size_t)(2 * 3 * 3 * 64 * 32 + 3 * 10 * 34 * 32 + 5 * 64 * 4 + 2 * Cin * 4);
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)conv3s_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds - 2 * Cin * 4 + 2 * 2048 * 4)););
    TDGP_LAUNCH("conv_mfma_kernel", conv3s_mfma_kernel, dim3((W >> 5) * cdiv(B * (H + 1), 8), cdiv(Cout, 64)), dim3(256), lds, L.s, q);
}

int launch_wino4f(const ConvLaunch& L) {
    const ConvCall& c = L.c;
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W;
    int* ticket = ticket_ptr(L.ws, L.wl);
    const XcdRect r = xcd_rect(Cout >> 6, 1, 64, 32);
    Wino4fParams q;
    q.x = L.x; q.styles = L.styles; q.u = L.wp + L.pi.wino4; q.e = L.e;
    q.B = B; q.Cin = Cin; q.Cout = Cout; q.H = H; q.W = W; q.u_bytes = (uint32_t)(L.pi.wino4_floats * 4); q.x_bytes = L.x_bytes(); q.st_bytes = L.st_bytes();
    q.nz_bytes = L.e.noise ? (uint32_t)(((L.e.noise_bstride ? (int64_t)(B - 1) * L.e.noise_bstride : 0) + (int64_t)H * W) * 4) : 0u;
    q.gxn = W / 64; q.gyn = H / 8; q.rs = r.rs; q.rt = r.rt; q.nxcd = r.nxcd; q.ticket = ticket;
    const size_t lds = (size_t)W4F_LDS_FLOATS * 4;
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)conv3_wino4f_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds););
    TDGP_CHECK(hipMemsetAsync(ticket, 0, 32, L.s) == hipSuccess, TDGP_ELAUNCH, "modconv2d: clearing the item counters failed");
    TDGP_LAUNCH("conv_wino4f_kernel", conv3_wino4f_kernel, dim3((unsigned)(r.nxcd * r.per)), dim3(512), lds, L.s, q);
    return TDGP_OK;
}

// F(4x4) through V: plain, K-split (plan.ksl) and folded x2 (out_layout 2) layers; the batch in sub-batches of plan.bsub samples
void launch_wino4(const ConvLaunch& L) {
    const ConvCall& c = L.c;
    const PackInfo& pi = L.pi;
    const EpiParams& e = L.e;
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W, ksl = L.plan.ksl, bsub = L.plan.bsub;
    const XcdRect r = xcd_rect(cdiv(Cout, W4_BM) << ksl, 1, W4_BM, 64);       // (one resident block per CU; tiles per item: 64 for a pair of tile groups)
    const size_t lds = (size_t)(8 * W4_UCH + 3 * W4_BM + 4) * 4;          // the stages, bias + demodulation of the slice, the ticket
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)conv3_wino4_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); (void)hipFuncSetAttribute((const void*)conv3_wino4_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds););
    float* vbuf = L.vbuf();
    float* partial = L.partial();
    int* ticket = ticket_ptr(L.ws, L.wl);
    const int64_t kslice = (int64_t)B * Cout * H * W;
    for (int b0 = 0; b0 < B; b0 += bsub) {
        const int bn = std::min(bsub, B - b0);
        Wino4Params q;
        q.v = vbuf; q.u = L.wp + pi.wino4; q.e = e;
        q.e.y = e.y + (int64_t)b0 * Cout * H * W;                        // (out_layout 2: Cout / 4 channels of 4 H W pixels -- the same count)
        q.ups = c.out_layout == 2 ? 1 : 0;
        if (e.dcoef) q.e.dcoef = e.dcoef + (int64_t)b0 * Cout;
        if (e.noise) q.e.noise = e.noise + (int64_t)b0 * e.noise_bstride;
        q.e.B = bn;
        q.B = bn; q.Cin = Cin; q.Cout = Cout; q.CoutP = pi.CoutP; q.H = H; q.W = W;
        q.v_bytes = (uint32_t)wino4_v_bytes(bn, Cin, H, W); q.u_bytes = (uint32_t)(pi.wino4_floats * 4);
        q.txl = wino4_txl(H, W); q.gxn = W / (4 << q.txl); q.gyn = H / (128 >> q.txl);
        q.rs = r.rs; q.rt = r.rt; q.nxcd = r.nxcd; q.ticket = ticket; q.ksl = ksl; q.partial = partial;
        const int ntg = q.gxn * q.gyn * bn;
        TDGP_LAUNCH("wino4_input_kernel", wino4_input_kernel, dim3((unsigned)(ntg * pi.nch4)), dim3(128), 0, L.s, L.x + (int64_t)b0 * Cin * H * W,
                    L.styles ? L.styles + (int64_t)b0 * Cin : nullptr, vbuf, bn, Cin, H, W, q.gxn, q.gyn, pi.nch4, q.txl, ticket);
        if (q.ups) TDGP_LAUNCH("upconv_wino4_kernel", (conv3_wino4_kernel<true, true>), dim3((unsigned)(r.nxcd * r.per)), dim3(512), lds, L.s, q);
        else TDGP_LAUNCH("conv_wino4_kernel", (conv3_wino4_kernel<false, true>), dim3((unsigned)(r.nxcd * r.per)), dim3(512), lds, L.s, q);
        if (ksl) TDGP_LAUNCH("splitk_reduce_kernel", splitk_reduce_kernel, dim3((int)min((int64_t)2048, cdiv64(kslice, 256))), dim3(256), 0, L.s, partial, 1 << ksl, e);
    }
}

void launch_wino2(const ConvLaunch& L) {
    const ConvCall& c = L.c;
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W;
    WinoParams q;
    q.x = L.x; q.u = L.wp + L.pi.wino; q.styles = L.styles; q.e = L.e;
    q.B = B; q.Cin = Cin; q.Cout = Cout; q.CoutP = L.pi.CoutP; q.H = H; q.W = W;
    q.x_bytes = L.x_bytes(); q.u_bytes = (uint32_t)(L.pi.wino_floats * 4);
    const size_t lds = wino_lds_bytes(Cin);
    TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)conv3_wino_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024););
    const int cus = tdgp_cu_count();
    const int64_t nitems = (int64_t)(W >> 5) * (H >> 3) * B * cdiv(Cout, 64);
    TDGP_LAUNCH("conv_wino_kernel", conv3_wino_kernel, dim3((unsigned)min((int64_t)cus, nitems)), dim3(512), lds, L.s, q);
}

// transposed conv, stride 2, UNFLIPPED weights (conv2d_resample.py:108-125) -> parity-planar Z -> FIR + output stage
void launch_up(const ConvLaunch& L) {
    const ConvCall& c = L.c;
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W;
    const UpPlan& pl = L.plan.up;
    float* z = L.z();
    if (L.plan.up_split) {
        Up3sParams q;
        q.x = L.x; q.wsp = L.wp + L.pi.wsplit; q.styles = L.styles; q.z = z;
        q.B = B; q.Cin = Cin; q.Cout = Cout; q.CoutP = L.pi.CoutP; q.H = H; q.W = W; q.G1 = pl.G1; q.GS = pl.GS; q.zslice = pl.zslice;
        q.x_bytes = L.x_bytes(); q.wsp_bytes = (uint32_t)(L.pi.wsplit_floats * 4);
        const size_t lds = (size_t)(2 * 3 * 3 * 64 * 32 + 3 * 2 * 130 * 32 + (2 * 8 * 256 + 8 * 64) * 4 + 2 * 64 * 4);
        TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)upconv3s_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds););
        TDGP_LAUNCH("upconv_mfma_kernel", upconv3s_mfma_kernel, dim3(cdiv(B * pl.GS, 128), cdiv(Cout, 64)), dim3(256), lds, L.s, q);
    } else {
        // (Round 3, measured and not kept: 8-wave blocks -- 128 x 128 for Cout > 64, 64 x 256 below -- so that one staged weight chunk serves twice the
        //  MFMAs: -0.7 % / -1.3 % on the whole step; the staging instructions are not what holds this kernel at 0.65 of the MFMA peak.)
        const UpParams u = make_up(B, Cin, Cout, H, W, L.pi, pl, L.x, L.wp, L.styles, z);
        if (pl.cfg == 0) launch_upconv<2, 1, 2, 2, true>(u, L.s);
        else launch_upconv<2, 1, 1, 4, false>(u, L.s);
    }
    launch_fir(make_fir(L.e, z, pl, H, W, L.plan.up_split ? 1 : pl.ksplit, false), L.plan.fir_tile, false, L.s);
}

// The call a shape query asks about: `flags` = TDGP_PATHQ_* (include/tdgp.h); plain lrelu layer or linear output, under the current arithmetic mode
inline ConvCall query_call(int B, int Cin, int Cout, int H, int W, int k, int up, int out_layout, int flags) {
    const bool lrelu = (flags & TDGP_PATHQ_LRELU) != 0, aligned = (flags & TDGP_PATHQ_ALIGNED) != 0;
    return ConvCall{B, Cin, Cout, H, W, k, up, out_layout, out_layout == 1 ? 4 : 0,
                    (flags & TDGP_PATHQ_STYLES) != 0, (flags & TDGP_PATHQ_SKIP) != 0, (flags & TDGP_PATHQ_NOISE) != 0, (flags & TDGP_PATHQ_DEMODULATE) != 0,
                    lrelu ? 3 : 1, lrelu ? 0.2f : 0.f, lrelu ? 1.41421356f : 1.f, -1.f, aligned, aligned, g_conv_arith};
}

}  // namespace

TDGP_API int64_t tdgp_modconv_pack_bytes(int Cout, int Cin, int k) {
    if (Cout < 1 || Cin < 1 || (k != 1 && k != 3 && k != 5)) return -1;
    return pack_info(Cout, Cin, k).total * (int64_t)sizeof(float);
}

TDGP_API int tdgp_modconv_pack(const float* weight, void* wpack, int Cout, int Cin, int k, tdgp_stream_t stream) {
    TDGP_CHECK(weight && wpack, TDGP_EINVAL, "modconv_pack: null pointer");
    TDGP_CHECK(Cout >= 1 && Cin >= 1, TDGP_EINVAL, "modconv_pack: bad channel counts");
    TDGP_CHECK(k == 1 || k == 3 || k == 5, TDGP_EUNSUPPORTED, "modconv_pack: kernel size %d not on the generator path (1, 3 or 5)", k);
    const PackInfo pi = pack_info(Cout, Cin, k);
    float* wp = (float*)wpack;
    TDGP_LAUNCH("pack_kernel", pack_kernel, dim3((int)min((int64_t)4096, cdiv64(pi.wp_floats, 256))), dim3(256), 0, (hipStream_t)stream, weight, wp + pi.wp,
                       wp + pi.wsq, Cout, Cin, pi.T, pi.KC, pi.CoutP, pi.nchunks);
    if (pi.wsplit_floats > 0)
        TDGP_LAUNCH("pack_kernel", pack_split_kernel, dim3((int)min((int64_t)4096, cdiv64(pi.wsplit_floats, 256))), dim3(256), 0, (hipStream_t)stream, weight,
                    (uint32_t*)(wp + pi.wsplit), Cout, Cin, pi.CoutP, pi.niter16);
    if (pi.wbf_floats > 0)
        TDGP_LAUNCH("pack_kernel", pack_bf16_kernel, dim3((int)min((int64_t)4096, cdiv64(pi.wbf_floats, 256))), dim3(256), 0, (hipStream_t)stream, weight,
                    (uint32_t*)(wp + pi.wbf), Cout, Cin, pi.CoutP, pi.nch32);
    if (pi.wino_floats > 0)
        TDGP_LAUNCH("pack_kernel", pack_wino_kernel, dim3((int)min((int64_t)4096, cdiv64(pi.wino_floats, 256))), dim3(256), 0, (hipStream_t)stream, weight,
                    wp + pi.wino, Cout, Cin, pi.CoutP, pi.nch8);
    if (pi.wino4_floats > 0)
        TDGP_LAUNCH("pack_kernel", pack_wino4_kernel, dim3((int)min((int64_t)4096, cdiv64(pi.wino4_floats, 256))), dim3(256), 0, (hipStream_t)stream, weight,
                    wp + pi.wino4, Cout, Cin, cdiv(Cout, W4_BM), pi.nch4);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_set_conv_arith(int mode) {
    TDGP_CHECK(mode >= 0 && mode <= 4, TDGP_EINVAL, "set_conv_arith: mode %d (0 = fp32 MFMA, Winograd F(4x4,3x3) / F(2x2,3x3) where they pay; 1 = split-bf16 MFMA with fp32 accumulation; 2 = fp32 MFMA, direct sums only; 3 = as 0 without F(4x4); 4 = as 0 with the F(4x4) input transform always as a pass of its own)", mode);
    const int old = g_conv_arith;
    g_conv_arith = mode;
    return old;
}

// Cheap shape query (no launch, no allocation): does tdgp_modconv2d take a FOLDED x2 layer (out_layout 2: four parity 3x3 kernels, Cout4 = 4 x the
// layer's output channels) of this shape on the Winograd F(4x4) kernels under the current arithmetic mode?  The binding asks BEFORE it folds and
// packs the [4 Cout, Cin, 3, 3] weights (ADVICE r04: small launches paid the fold, the pack and an exception to learn the answer).
TDGP_API int tdgp_modconv2d_takes_folded_up2(int B, int Cin, int Cout4, int H, int W) {
    return (B >= 1 && (Cout4 & 3) == 0 && plan_modconv(query_call(B, Cin, Cout4, H, W, 3, 1, 2, TDGP_PATHQ_ALIGNED)).path == TDGP_PATH_WINO4_FOLDED) ? 1 : 0;
}

// Which kernel family tdgp_modconv2d gives a call of this shape under the current arithmetic mode (include/tdgp.h): the plan the launch itself reads.
TDGP_API int tdgp_modconv2d_path(int B, int Cin, int Cout, int H, int W, int k, int up, int out_layout, int flags) {
    TDGP_CHECK(B >= 1 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1, TDGP_EINVAL, "modconv2d_path: bad shape");
    TDGP_CHECK(k == 1 || k == 3 || k == 5, TDGP_EUNSUPPORTED, "modconv2d_path: kernel size %d not supported (1, 3 or 5)", k);
    TDGP_CHECK(up == 1 || (up == 2 && k == 3), TDGP_EUNSUPPORTED, "modconv2d_path: up=%d with k=%d not supported", up, k);
    const ConvCall c = query_call(B, Cin, Cout, H, W, k, up, out_layout, flags);
    TDGP_CHECK(!c.has_skip || (up == 1 && k == 1 && (H % 2) == 0 && (W % 2) == 0), TDGP_EINVAL, "modconv2d_path: skip needs k=1, up=1 and even H/W");
    TDGP_CHECK(!c.demodulate || c.has_styles, TDGP_EINVAL, "modconv2d_path: demodulate needs styles");
    TDGP_CHECK(out_layout == 0 || (out_layout == 2 && k == 3 && up == 1 && (Cout & 3) == 0 && !c.has_skip) || (out_layout == 1 && up == 1 && k == 1), TDGP_EINVAL,
               "modconv2d_path: out_layout %d does not go with k=%d, up=%d", out_layout, k, up);
    TDGP_CHECK((int64_t)B * Cin * H * W < ((int64_t)1 << 30) && (int64_t)B * Cout * (H * up + 1) * (W * up + 1) <= INT32_MAX, TDGP_EINVAL,
               "modconv2d_path: tensor too large (activations are addressed through 4 GiB buffer descriptors)");
    TDGP_CHECK(out_layout != 2 || wino4_takes(c), TDGP_EUNSUPPORTED, "modconv2d_path: out_layout 2 is written by the Winograd F(4x4) kernels only");
    return plan_modconv(c).path;
}

TDGP_API int64_t tdgp_modconv2d_workspace_bytes(int B, int Cin, int Cout, int H, int W, int k, int up) {
    return ws_layout(B, Cin, Cout, H, W, k, up).total;
}

TDGP_API int tdgp_modconv2d(const float* x, const void* wpack, const float* styles, const float* dcoef_in, const float* noise, int64_t noise_bstride,
                            const float* bias, const float* fir4x4, const float* skip, float* y, int B, int Cin, int Cout, int H, int W,
                            int k, int up, int demodulate, int act, float alpha, float gain, float clamp, int out_layout, int out_feat,
                            void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(x && wpack && y, TDGP_EINVAL, "modconv2d: null pointer");
    TDGP_CHECK(B >= 1 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1, TDGP_EINVAL, "modconv2d: bad shape");
    TDGP_CHECK(k == 1 || k == 3 || k == 5, TDGP_EUNSUPPORTED, "modconv2d: kernel size %d not supported (1, 3 or 5)", k);
    TDGP_CHECK(up == 1 || (up == 2 && k == 3), TDGP_EUNSUPPORTED, "modconv2d: up=%d with k=%d not supported", up, k);
    TDGP_CHECK(up == 1 || fir4x4, TDGP_EINVAL, "modconv2d: up=2 needs the 4x4 resample filter");
    TDGP_CHECK(!skip || (up == 1 && k == 1 && fir4x4 && (H % 2) == 0 && (W % 2) == 0), TDGP_EINVAL, "modconv2d: skip needs k=1, up=1, even H/W and the filter");
    TDGP_CHECK(!demodulate || styles, TDGP_EINVAL, "modconv2d: demodulate needs styles");
    TDGP_CHECK(act >= 1 && act <= 9, TDGP_EUNSUPPORTED, "modconv2d: unknown activation %d", act);
    TDGP_CHECK(out_layout == 0 || out_layout == 2 || (out_layout == 1 && out_feat >= 4 && (out_feat % 4) == 0 && (Cout % out_feat) == 0 && up == 1 && k == 1), TDGP_EINVAL,
               "modconv2d: the channel-last plane layout is a ToRGB (k=1, up=1) output");
    // out_layout 2: the x2 layers with the FIR folded into four 3x3 parity kernels (Cout = 4 x the real channels, channel 4 o + 2 py + px;
    // y is [B, Cout / 4, 2H, 2W], noise a 2H x 2W map, bias / dcoef_in replicated per parity by the caller).  Only the F(4x4) kernels write it.
    TDGP_CHECK(out_layout != 2 || (k == 3 && up == 1 && (Cout & 3) == 0 && !skip && (!demodulate || dcoef_in)), TDGP_EINVAL,
               "modconv2d: out_layout 2 (folded x2 layer) needs k=3, up=1, Cout %% 4 == 0, no skip and precomputed demodulation coefficients");
    const ConvCall c{B, Cin, Cout, H, W, k, up, out_layout, out_feat, styles != nullptr, skip != nullptr, noise != nullptr, demodulate != 0, act, alpha, gain, clamp,
                     io_aligned(x, y, noise, noise_bstride, 16), io_aligned(x, y, noise, noise_bstride, 8), g_conv_arith};
    TDGP_CHECK(out_layout != 2 || wino4_takes(c), TDGP_EUNSUPPORTED,
               "modconv2d: out_layout 2 is written by the Winograd F(4x4) kernels only (shape %dx%d, %d -> %d channels, batch %d does not take them)", H, W, Cin, Cout, B);
    TDGP_CHECK((int64_t)B * Cin * H * W < ((int64_t)1 << 30) && (int64_t)B * Cout * (H * up + 1) * (W * up + 1) <= INT32_MAX, TDGP_EINVAL,
               "modconv2d: tensor too large (activations are addressed through 4 GiB buffer descriptors)");
    ConvLaunch L;
    L.c = c; L.plan = plan_modconv(c); L.pi = pack_info(Cout, Cin, k); L.wl = ws_layout(B, Cin, Cout, H, W, k, up);
    TDGP_CHECK(workspace && workspace_bytes >= L.wl.total, TDGP_EWORKSPACE, "modconv2d: workspace %lld < %lld bytes", (long long)workspace_bytes,
               (long long)L.wl.total);
    L.x = x; L.wp = (const float*)wpack; L.styles = styles; L.ws = (char*)workspace; L.s = (hipStream_t)stream;
    const float* dco = demod_coefs(demodulate, dcoef_in, styles, L.wp + L.pi.wsq, (float*)(L.ws + L.wl.dco), B, Cin, Cout, L.pi.CoutP, L.s);
    L.e = make_epi(c, fir4x4, dco, noise, noise_bstride, bias, skip, y, 0);
    switch (L.plan.path) {
        case TDGP_PATH_DIRECT:
        case TDGP_PATH_CONV1: launch_direct(L); break;
        case TDGP_PATH_CONV3: launch_conv3_path(L); break;
        case TDGP_PATH_SPLIT3: launch_split3(L); break;
        case TDGP_PATH_WINO2: launch_wino2(L); break;
        case TDGP_PATH_WINO4:
        case TDGP_PATH_WINO4_SPLITK:
        case TDGP_PATH_WINO4_FOLDED: launch_wino4(L); break;
        case TDGP_PATH_WINO4F: if (const int rc = launch_wino4f(L)) return rc; break;
        case TDGP_PATH_UP: launch_up(L); break;
        case TDGP_PATH_TORGB: {
            const RgbParams r = make_rgb(c, L.pi, x, L.x_bytes(), L.wp, styles, L.e);
            if (L.plan.rgb_mt == 1) launch_torgb<1>(r, L.s);
            else if (L.plan.rgb_mt == 2) launch_torgb<2>(r, L.s);
            else launch_torgb<3>(r, L.s);
            break;
        }
    }
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// Reduced-precision blocks (BASELINE configs[4], modconv_bf16.inc): x is bf16 NCHW; y is bf16 NCHW (3x3 layers) or, for the ToRGB
// form (k = 1, channel-last planes + fused skip), fp32.  Forms the bf16 MFMA kernels take: 3x3 with Cin % 32 == 0, Cin <= 2048 and, for
// up = 1, W % 32 == 0 and H >= 8 (conv3_bf16_kernel stages the styles of TWO samples per block: with H + 1 <= 7 its 10-row window reaches
// real rows of a third); the channel-last ToRGB.  Anything else returns TDGP_EUNSUPPORTED (the caller widens to fp32 and uses tdgp_modconv2d).
TDGP_API int tdgp_modconv2d_bf16(const void* x, const void* wpack, const float* styles, const float* dcoef_in, const float* noise, int64_t noise_bstride,
                                 const float* bias, const float* fir4x4, const float* skip, void* y, int B, int Cin, int Cout, int H, int W, int k, int up,
                                 int demodulate, int act, float alpha, float gain, float clamp, int out_layout, int out_feat, void* workspace,
                                 int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(x && wpack && y, TDGP_EINVAL, "modconv2d_bf16: null pointer");
    TDGP_CHECK(B >= 1 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1, TDGP_EINVAL, "modconv2d_bf16: bad shape");
    TDGP_CHECK(act >= 1 && act <= 9, TDGP_EUNSUPPORTED, "modconv2d_bf16: unknown activation %d", act);
    TDGP_CHECK(!demodulate || styles, TDGP_EINVAL, "modconv2d_bf16: demodulate needs styles");
    TDGP_CHECK((int64_t)B * Cin * H * W < ((int64_t)1 << 30) && (int64_t)B * Cout * (H * up + 1) * (W * up + 1) <= INT32_MAX, TDGP_EINVAL,
               "modconv2d_bf16: tensor too large (activations are addressed through 4 GiB buffer descriptors)");
    const bool rgb = k == 1 && up == 1 && out_layout == 1 && Cout <= 96 && !demodulate && !noise && act == 1 && ((H * W) & 3) == 0 && out_feat >= 4 &&
                     (out_feat % 4) == 0 && (Cout % out_feat) == 0 && (!skip || (fir4x4 && (H % 2) == 0 && (W % 2) == 0));
    const bool c3 = k == 3 && up == 1 && out_layout == 0 && !skip && (W & 31) == 0 && (Cin & 31) == 0 && Cin <= 2048 && H >= 8;
    bool u3 = k == 3 && up == 2 && out_layout == 0 && !skip && fir4x4 && (Cin & 31) == 0 && Cin <= 2048 && (W & 1) == 0;
    size_t u3_lds = 0;
    if (u3) {                                     // every acceptance test before the first launch: the x2 kernel keeps the styles of all samples a block's
        const UpPlan pl0 = up_plan(B, Cin, Cout, H, W);                                   // grid points can touch in LDS
        const int nsb0 = std::min(B, (130 + pl0.G1) / pl0.GS + 2);
        u3_lds = (size_t)(9 * 2 * 64 * 32 + 2 * 2 * 130 * 32) + (size_t)nsb0 * Cin * 4;
        TDGP_CHECK(u3_lds <= 80 * 1024, TDGP_EUNSUPPORTED, "modconv2d_bf16: x2 layer with Cin=%d, B=%d, H=%d needs %zu bytes of LDS (> 80 KiB)", Cin, B, H, u3_lds);
    }
    TDGP_CHECK(rgb || c3 || u3, TDGP_EUNSUPPORTED, "modconv2d_bf16: no bf16 kernel for k=%d up=%d Cin=%d H=%d W=%d layout=%d", k, up, Cin, H, W, out_layout);
    const bool nz16 = noise_aligned(noise, noise_bstride, 16);
    TDGP_CHECK(nz16, TDGP_EINVAL, "modconv2d_bf16: noise must be 16-byte aligned with a batch stride that is a multiple of 4 floats");
    const WsLayout wl = ws_layout(B, Cin, Cout, H, W, k, up);
    TDGP_CHECK(workspace && workspace_bytes >= wl.total, TDGP_EWORKSPACE, "modconv2d_bf16: workspace %lld < %lld bytes", (long long)workspace_bytes,
               (long long)wl.total);
    hipStream_t s = (hipStream_t)stream;
    const PackInfo pi = pack_info(Cout, Cin, k);
    const float* wp = (const float*)wpack;
    const void* wb = wp + pi.wbf;
    float* z = (float*)((char*)workspace + wl.z);
    const float* dco = demod_coefs(demodulate, dcoef_in, styles, wp + pi.wsq, (float*)((char*)workspace + wl.dco), B, Cin, Cout, pi.CoutP, s);
    const ConvCall c{B, Cin, Cout, H, W, k, up, out_layout, out_feat, styles != nullptr, skip != nullptr, noise != nullptr, demodulate != 0, act, alpha, gain, clamp,
                     false, false, g_conv_arith};                  // (alignment and mode: not read here -- the forms were decided above)
    const EpiParams e = make_epi(c, fir4x4, dco, noise, noise_bstride, bias, skip, (float*)y, 1);
    const uint32_t x_bytes = (uint32_t)((int64_t)B * Cin * H * W * 2);
    if (rgb) {
        const RgbParams r = make_rgb(c, pi, (const float*)x, x_bytes, wp, styles, e);
        if (Cout <= 32) launch_torgb<1, true>(r, s);
        else if (Cout <= 64) launch_torgb<2, true>(r, s);
        else launch_torgb<3, true>(r, s);
    } else if (c3) {
        ConvBfParams q;
        q.x = (const uint16_t*)x; q.wb = wb; q.styles = styles; q.e = e; q.y16 = (uint16_t*)y;
        q.B = B; q.Cin = Cin; q.Cout = Cout; q.CoutP = pi.CoutP; q.H = H; q.W = W;
        q.x_bytes = x_bytes; q.wb_bytes = (uint32_t)(pi.wbf_floats * 4);
        const size_t lds = (size_t)(9 * 2 * 64 * 32 + 2 * 10 * 34 * 32 + 5 * 64 * 4 + 2 * Cin * 4);
        TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)conv3_bf16_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds - 2 * Cin * 4 + 2 * 2048 * 4)););
        TDGP_LAUNCH("conv_bf16_kernel", conv3_bf16_kernel<true>, dim3((W >> 5) * cdiv(B * (H + 1), 8), cdiv(Cout, 64)), dim3(256), lds, s, q);
    } else {
        const UpPlan pl = up_plan(B, Cin, Cout, H, W);
        UpBfParams q;
        q.x = (const uint16_t*)x; q.wb = wb; q.styles = styles; q.z = z;
        q.B = B; q.Cin = Cin; q.Cout = Cout; q.CoutP = pi.CoutP; q.H = H; q.W = W; q.G1 = pl.G1; q.GS = pl.GS; q.zslice = pl.zslice;
        q.x_bytes = x_bytes; q.wb_bytes = (uint32_t)(pi.wbf_floats * 4); q.st_bytes = (uint32_t)((int64_t)B * Cin * 4);
        const size_t lds = u3_lds;                                              // checked against the 80 KiB budget above
        TDGP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)upconv_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024););
        TDGP_LAUNCH("upconv_bf16_kernel", upconv_bf16_kernel, dim3(cdiv(B * pl.GS, 128), cdiv(Cout, 64)), dim3(256), lds, s, q);
        launch_fir(make_fir(e, z, pl, H, W, 1, true), fir_tile(2 * H, 2 * W, 1, act, alpha, true), true, s);
    }
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_cast_f32_bf16(const float* x, void* y_bf16, int64_t n, tdgp_stream_t stream) {
    TDGP_CHECK((x && y_bf16) || n == 0, TDGP_EINVAL, "cast_f32_bf16: null pointer");
    if (n <= 0) return TDGP_OK;
    TDGP_LAUNCH("cast_f32_bf16_kernel", cast_f32_bf16_kernel, dim3((int)min((int64_t)8192, cdiv64(n, 512))), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)y_bf16, n);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_conv_transpose2d_x2(const float* x, const void* wpack, const float* styles, float* y, int B, int Cin, int Cout, int H, int W,
                                      void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(x && wpack && y, TDGP_EINVAL, "conv_transpose2d_x2: null pointer");
    TDGP_CHECK(B >= 1 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1, TDGP_EINVAL, "conv_transpose2d_x2: bad shape");
    TDGP_CHECK((int64_t)B * Cin * H * W < ((int64_t)1 << 30) && (int64_t)B * Cout * (H * 2 + 1) * (W * 2 + 1) <= INT32_MAX, TDGP_EINVAL,
               "conv_transpose2d_x2: tensor too large (activations are addressed through 4 GiB buffer descriptors)");
    const WsLayout wl = ws_layout(B, Cin, Cout, H, W, 3, 2);
    TDGP_CHECK(workspace && workspace_bytes >= wl.total, TDGP_EWORKSPACE, "conv_transpose2d_x2: workspace %lld < %lld bytes", (long long)workspace_bytes,
               (long long)wl.total);
    hipStream_t s = (hipStream_t)stream;
    const PackInfo pi = pack_info(Cout, Cin, 3);
    float* z = (float*)((char*)workspace + wl.z);
    const UpPlan pl = up_plan(B, Cin, Cout, H, W);
    const UpParams u = make_up(B, Cin, Cout, H, W, pi, pl, x, (const float*)wpack, styles, z);
    if (pl.cfg == 0) launch_upconv<2, 1, 2, 2, true>(u, s);
    else launch_upconv<2, 1, 1, 4, false>(u, s);
    const int64_t rows = (int64_t)B * Cout * (2 * H + 1);
    TDGP_LAUNCH("z_gather_kernel", z_gather_kernel, dim3((unsigned)min((int64_t)65535 * 8, rows)), dim3(256), 0, s, (const float*)z, y, rows, 2 * H + 1, 2 * W + 1,
                2 * pl.G1, 2 * pl.GS, pl.ksplit, pl.zslice);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_modconv_wsq_offset(int Cout, int Cin, int k) {
    if (Cout < 1 || Cin < 1 || (k != 1 && k != 3 && k != 5)) return -1;
    return pack_info(Cout, Cin, k).wsq * (int64_t)sizeof(float);
}

TDGP_API int tdgp_demod_batch(const float* styles_all, const int64_t* meta, float* dcoef_all, int B, int num_layers, int max_cout, tdgp_stream_t stream) {
    TDGP_CHECK(styles_all && meta && dcoef_all, TDGP_EINVAL, "demod_batch: null pointer");
    TDGP_CHECK(B >= 1 && num_layers >= 1 && max_cout >= 1, TDGP_EINVAL, "demod_batch: bad shape");
    TDGP_LAUNCH("demod_kernel", demod_batch_kernel, dim3(cdiv(max_cout, 64), B, num_layers), dim3(1024), 0, (hipStream_t)stream, styles_all, meta, dcoef_all, B);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_style_affine(const float* ws, const float* A, const float* abias, const int32_t* row_meta, const float* row_scale,
                               float* styles, int B, int num_ws, int w_dim, int rows_total, tdgp_stream_t stream) {
    TDGP_CHECK(ws && A && abias && row_meta && row_scale && styles, TDGP_EINVAL, "style_affine: null pointer");
    TDGP_CHECK(B >= 1 && num_ws >= 1 && w_dim >= 1 && rows_total >= 1, TDGP_EINVAL, "style_affine: bad shape");
    const int64_t waves = (int64_t)B * rows_total;
    const float wgain = (float)(1.0 / sqrt((double)w_dim));
    TDGP_LAUNCH("style_affine_kernel", style_affine_kernel, dim3((int)cdiv64(waves, 4)), dim3(256), 0, (hipStream_t)stream, ws, A, abias, row_meta, row_scale, styles, B,
                       num_ws, w_dim, rows_total, wgain);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

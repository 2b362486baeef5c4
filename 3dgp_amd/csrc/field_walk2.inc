// field_walk2.inc -- the image walk of the field kernel as a producer / consumer pair of waves per SIMD (round 3).
//
// Same function, same arithmetic in the same order as triplane_walk_kernel (field.hip; reference: tri_plane_renderer.py:560-588,
// networks_epigraf.py:46-68) -- results are bit-identical to it and to the generic kernel.  What changes is who does what:
//
//   block = 8 waves = one 8x8-pixel patch at a time, one block per CU (persistent grid).  Waves 0..3 are PRODUCERS, waves 4..7 CONSUMERS;
//   producer w and consumer w + 4 form a pair that marches the S samples of one 4x4-pixel quadrant (with the round-robin placement of a
//   workgroup's waves they sit on the same SIMD).
//   producer : coordinate -> tap arithmetic (lane = (ray, sample), four samples at a time, into an LDS table), 24 x 16-B buffer loads per
//              16-point tile with TWO tiles of taps in flight (192 registers: a wave that never multiplies can afford them), bilinear
//              blend + plane sum as one packed fma chain, blended features g[16 points][F] written to an LDS ring in the layout the
//              MFMA B operand wants (LDS does the lane transpose that used to take FQ ds_bpermute per tile);
//   consumer : reads g of the next tile while the matrix pipe runs this one: layer 1 (v_mfma_f32_16x16x4_f32, A operands and bias
//              resident in registers), leaky ReLU, layer 2 (16-block v_mfma_f32_4x4x1); the four hidden-quarter partial sums of a point
//              are parked in LDS and added when a run of 8 samples is flushed as 128-B stores (no cross-lane shuffles in the loop).
//   The two meet through the ring and two LDS counters (tiles produced / consumed).  LDS executes a wave's instructions in order, so a
//   counter written after the data is seen after the data; the compiler is held to program order around the counters.
//
// Why: in the one-role kernel a wave alternates between a vector phase that waits on memory / LDS round trips and a matrix phase, and two
// such waves per SIMD cannot cover each other (measured r02/r03: 2900 cycles per tile against 1152 matrix + ~620 vector-issue cycles;
// 2440 with the tap loads compiled out).  Here the matrix stream of a SIMD never waits for memory, and the memory side runs ahead by up
// to NSLOT tiles.
constexpr int WALK2_SLOTS = 6;         // ring tiles per pair (4 when HID >= 128: Walk2Lds::NS)
constexpr int WALK2_SPIN = 1 << 15;    // bounded waits (~2 ms; a legitimate one lasts microseconds): a protocol bug or a stall under a debugger must
                                       // never hang the GPU -- on a timeout the wave sets the library's device-fault word (include/tdgp.h:
                                       // tdgp_device_fault) and ends; its partner times out once and ends too: the launch finishes, flagged
__device__ __forceinline__ void walk2_fault(int* word, int code) {
    if (word && lane_id() == 0) __hip_atomic_fetch_or(word, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int FQ, int MT>
struct Walk2Lds {
    static constexpr int F = FQ * 4, HID = MT * 16;
    // LDS layouts laid out against the bank map of the instruction widths that touch them (MI355X_MICROARCH.md, LDS table; modelled in
    // tools/dev/lds_conflicts.py, which reproduces round 3's measured SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.45 as 0.44):
    //   ring tile  g[16 points][F]: points in PAIRS of RP2 float4 slots, the odd point at slot RPO with its channel quads xor 2 --
    //              conflict-free for the producer's ds_write_b128 (8 lanes = 2 points x 4 quads, 32 banks) AND the consumer's ds_read_b128
    //              (16-lane groups {0-3,12-15,20-27}.., 64 banks); the second pass of F = 32 is a constant +4 slots.  Round 3's rows of
    //              F + 4 floats were 2-way conflicts both ways;
    //   tap table  [6 rows][TP slots], slot = 18 sample + ray: the address phase's ds_write_b128 (lane = ray, sample) hit 2 of 8
    //              bank slots with slot = 16 sample + ray (4-way, 32 LDS cycles per store);
    //   park       [16 rays][33] float4 as before (its flush reads stay 2-way: 4 of ~100 LDS cycles per tile; the conflict-free pitch
    //              47 does not fit the 160 KB).
    static constexpr int RP2 = 20, RPO = 12;                           // float4 slots per pair of points, offset of the odd one
    static constexpr int RT = 8 * RP2 * 4;                             // floats per ring tile
    static constexpr int TS = 18, TP = 4 * TS;                               // tap table: slots per sample, slots per row
    static constexpr int NS = (MT >= 8) ? 4 : WALK2_SLOTS;
    static constexpr int off_a0 = 0;                                   // [MT*FQ][64] layer-1 A operands (start-up only)
    static constexpr int off_a1 = off_a0 + MT * FQ * 64 * 4;           // [MT*4][64]  layer-2 A operands
    static constexpr int off_b0 = off_a1 + MT * 4 * 64 * 4;            // [HID]
    static constexpr int off_ctr = off_b0 + HID * 4;                   // per pair: {produced, consumed, -, -}
    static constexpr int ring_bytes = NS * RT * 4;                     // per pair: NS tiles of g[16][F] in the paired-row layout
    static constexpr int off_ring = off_ctr + 64;
    static constexpr int atab_bytes = 2 * 6 * TP * 16;                 // per pair: two tap tables (4 samples x 16 rays x 3 planes x {weights, offsets})
    static constexpr int off_atab = off_ring + 4 * ring_bytes;
    static constexpr int obuf_bytes = 16 * 33 * 16;                    // per pair: [16 rays][8 samples x 4 quarters (+1)] float4
    static constexpr int off_obuf = off_atab + 4 * atab_bytes;
    static constexpr int total = off_obuf + 4 * obuf_bytes;
    static_assert(total <= 160 * 1024, "walk2: LDS layout exceeds the CU's 160 KiB");
};

// float offset of (point pt, channel quad c) inside a ring tile
__device__ __forceinline__ int walk2_ring_off(int pt, int c, int RP2, int RPO) { return ((pt >> 1) * RP2 + (pt & 1) * RPO + (c ^ (2 * (pt & 1)))) * 4; }

// the counters: wave-uniform values (every lane reads / writes the same word), compared on the scalar unit
__device__ __forceinline__ int lds_peek(int* p) { return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); }
__device__ __forceinline__ void lds_poke(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#define TDGP_ORDER() asm volatile("" ::: "memory")

template <int FQ, int MT, bool TAPS>
__global__ __launch_bounds__(512, 1) void triplane_walk2_kernel(FieldParams p) {
    using L = Walk2Lds<FQ, MT>;
    constexpr int F = L::F, HID = L::HID, RT = L::RT, TP = L::TP, TS = L::TS, NS = L::NS;
    constexpr int NP = FQ / 4;                      // 16-channel passes per tile
    static_assert(FQ % 4 == 0 && FQ <= 8, "two tiles of taps must fit the register file");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* a0s = (float*)(smem + L::off_a0);
    float* a1s = (float*)(smem + L::off_a1);
    float* b0s = (float*)(smem + L::off_b0);
    const float sqrt2 = 1.41421353816986083984375f;
    for (int i = threadIdx.x; i < MT * FQ * 64; i += blockDim.x) {
        const int ln = i & 63, ms = i >> 6, mt = ms / FQ, sidx = ms % FQ;
        a0s[i] = (p.w0[(mt * 16 + (ln & 15)) * F + feat_of(sidx, ln >> 4, FQ)] * p.g0) / 3.0f;      // the plane mean's 1/3 lives in the layer-1 weights
    }
    for (int i = threadIdx.x; i < MT * 4 * 64; i += blockDim.x) {
        const int ln = i & 63, ms = i >> 6, mt = ms >> 2, r = ms & 3;
        a1s[i] = (p.w1[(ln & 3) * HID + mt * 16 + 4 * (ln >> 4) + r] * p.g1) * sqrt2;
    }
    for (int i = threadIdx.x; i < HID; i += blockDim.x) b0s[i] = p.b0[i];
    if (threadIdx.x < 16) ((int*)(smem + L::off_ctr))[threadIdx.x] = 0;
    __syncthreads();

    const int l = lane_id();
    const int wv = threadIdx.x >> 6, pair = wv & 3, role = wv >> 2;
    int* const ctr = (int*)(smem + L::off_ctr) + pair * 4;             // [0] tiles produced, [1] tiles consumed
    float* const ring = (float*)(smem + L::off_ring + pair * L::ring_bytes);
    const int S = p.S;

    // Work of a block: a patch is 8x8 pixels and pair w takes quadrant w.  (Measured, r03: one 4x4-pixel quad per patch shared by the four pairs,
    // pair w marching a quarter of the depth range so that the (x,y)-plane lines stay in the L1: correct (same bits), 3-4 % SLOWER than quadrants
    // (4.54 vs 4.38 ms): the L1 is not what the gather waits for.)
    const int PS = 8;                                   // patch side in pixels
    const int Sq = S;                                   // samples a pair marches per patch
    const int kb = 0;                                   // its first sample
    // patches of this block: ids lb, lb + nb, ... in the XCD-compact order of triplane_walk_kernel
    const int pX = (p.ray_w + PS - 1) / PS, pY = (p.ray_h + PS - 1) / PS;
    const int npatch = (int)(p.total / p.P) * pX * pY;
    const int nb = gridDim.x, per = nb / 8;
    const int lb = (nb % 8 == 0) ? (blockIdx.x % 8) * per + blockIdx.x / 8 : blockIdx.x;
    const int npl = lb < npatch ? (npatch - lb + nb - 1) / nb : 0;
    const int total = npl * Sq;                                        // tiles this pair marches
    if (total == 0) return;
    auto decode = [&](int patch, int& b, int& py, int& px) {
        if (((pX | pY) & 7) == 0) {
            const int per_img = pX * pY, r = patch % per_img, sq = r >> 6, in = r & 63;
            b = patch / per_img;
            px = (sq % (pX >> 3)) * 8 + (in & 7); py = (sq / (pX >> 3)) * 8 + (in >> 3);
        } else {
            px = patch % pX; py = (patch / pX) % pY; b = patch / (pX * pY);
        }
    };
    auto ray_of = [&](int b, int py, int px, int tpt, bool& ok) {          // pixel tpt of this pair's 4x4 quadrant -> ray index
        const int y = py * 8 + ((pair >> 1) & 1) * 4 + (tpt >> 2);
        const int x = px * 8 + (pair & 1) * 4 + (tpt & 3);
        ok = y < p.ray_h && x < p.ray_w;
        return b * (int)p.R + (ok ? y * p.ray_w + x : 0);
    };

    if (role == 0) {
        // ================================================================ producer
        // (No static priority for either role.  Measured, r03, one box, interleaved: producer at priority 3: +6 % time, consumer at 3: +8 %.)
        uint4* const atab = (uint4*)(smem + L::off_atab + pair * L::atab_bytes);      // [2][6][TP]
        const int gpt = l >> 2, gc4 = l & 3;
        const int plane_elems = p.H * p.W * F;
        const uint32_t plane_bytes = (uint32_t)plane_elems * 4u;
        // ADD_TID_ENABLE (descriptor word 3 bit 23) with stride 16: the hardware adds lane_id * 16 to every address.  The table rows are
        // biased by 1024 - 64 * ray (ray = lane >> 2), the descriptor base by -1024: lane 4 * ray + c4 lands on texel + 16 * c4 -- the
        // piece offset costs no vector instruction (12 v_add per tile otherwise).  DATA_FORMAT doubles as stride bits when ADD_TID is on: 0.
        // Measured: 4.56 -> 4.43 ms per 67 M points (B = 16, average of the two passes).
        const uint32_t tid_adj = 1024u - 64u * (uint32_t)gpt;
        // The tap loads and their waits are issued by hand (inline asm).  Reason: for loads whose results are used in the NEXT loop iteration
        // the compiler's wait-count bookkeeping gives up and waits for everything at the first use (vmcnt(0) at the loop head; reproduced
        // on a ten-line loop), so the two buffers were requested, awaited and refilled as one batch and the texture path sat idle while
        // the producer blended.  Written out, the waits are vmcnt(3 FQ) for buffer A (only B's 3 FQ = 24 refills are younger) and vmcnt(3 FQ + 3)
        // for B (A's refills and the three small loads are younger): each buffer is waited for separately and one is always in flight.
        // What this needs -- and tools/dev/check_walk2_isa.py checks in the ISA of every build -- is that the compiler never touches a tap
        // register between its load and the matching wait (it believes the value is there when the asm statement ends): no instruction
        // reads or writes them in that window.  The producer has no other vector-memory instruction the compiler knows about (the tap_idx
        // stores of the TAPS instance only make the hand-written counts wait for more, never less).
        typedef unsigned int w2_u32x4 __attribute__((ext_vector_type(4)));
        const uint64_t dbase = (uint64_t)(uintptr_t)((const char*)p.planes - 1024);
        const w2_u32x4 dsc = {(uint32_t)dbase, (uint32_t)((dbase >> 32) & 0xffffu) | (16u << 16), 0x7fffffffu, 0x00800000u};
        const int wslot = gc4 * TS + gpt;                  // table slot this lane writes: sample gc4 of the group, ray gpt
        const float sx = (float)(p.W - 1) / 2.f, sy = (float)(p.H - 1) / 2.f;
        const int gpp = Sq >> 2;                           // groups of four samples per patch and pair (S % 4 == 0, checked on the host)
        const int ngroups = npl * gpp;

        // What the address arithmetic of a group needs from memory -- origin and direction of ray gpt, the depth of sample gc4 -- is
        // requested one iteration ahead, UNCONDITIONALLY and at a fixed place of every iteration (into the same seven registers): with no
        // vector-memory instruction under a condition the compiler's wait counts for the tap buffers stay exact (vmcnt(24..27) instead of
        // the vmcnt(0) it falls back to when paths with different numbers of loads meet).
        typedef float w2_f32x3 __attribute__((ext_vector_type(3)));
        w2_f32x3 ray_o3 = {0.f, 0.f, 0.f}, ray_d3 = {0.f, 0.f, 0.f};     // the loaded vectors are kept whole until the address arithmetic reads them
        float t_grp = 0.f;
        int gray = 0;                                        // ray of the prefetched group (tap_idx rows), its validity
        bool gok = false;
        uint32_t soff_cur = 0, soff_nxt = 0, soff_n2 = 0;    // plane bases of the patches of the current group, the next one, the one after
        int pq_cached = -1;                                  // patch whose ray index / plane base are cached (the decode runs once per patch)
        uint32_t ray_voff = 0, t_voff = 0;                   // byte offsets of this lane's ray in ray_o / ray_d and of its first sample in t (per patch)
        auto prefetch_group = [&](int pi_, int gl_) {        // group gl_ of patch pi_ of this block
            if (pi_ != pq_cached) {                          // (scalar branch, no vector-memory instruction inside)
                int b, py, px;
                decode(lb + pi_ * nb, b, py, px);
                gray = ray_of(b, py, px, gpt, gok);
                soff_n2 = (uint32_t)b * 3u * plane_bytes;
                ray_voff = (uint32_t)gray * 12u;
                t_voff = ((uint32_t)gray * (uint32_t)S + (uint32_t)(kb + gc4)) * 4u;
                pq_cached = pi_;
            }
            // scalar base + 32-bit vector offset (the launcher checks that ray_o / ray_d / t stay below 4 GiB): the per-lane part is computed once per
            // patch, the group adds one scalar -- the 64-bit pointer arithmetic these three requests used to need was 9 vector instructions per pair of tiles
            const uint32_t tv = t_voff + (uint32_t)__builtin_amdgcn_readfirstlane(gl_ * 16);
            asm volatile("global_load_dwordx3 %0, %1, %2" : "=v"(ray_o3) : "v"(ray_voff), "s"(p.ray_o));
            asm volatile("global_load_dwordx3 %0, %1, %2" : "=v"(ray_d3) : "v"(ray_voff), "s"(p.ray_d));
            asm volatile("global_load_dword %0, %1, %2" : "=v"(t_grp) : "v"(tv), "s"(p.t));
        };
        // One (ray, sample) per lane: the arithmetic of triplane_walk_kernel's address_phase, step for step (tap indices bit-exact).
        auto address_phase = [&](int tb, int k0) {
            uint4* const tab = atab + tb * (6 * TP);
            const int ks = kb + k0 + gc4;
            // the three requested values become the compiler's HERE, behind the hand-written wait that covers them (a component copied
            // out of a vector that is still in flight was the one bug of this scheme: the first group of every block)
            asm volatile("" : "+v"(ray_o3), "+v"(ray_d3), "+v"(t_grp));
            const float ox = ray_o3[0], oy = ray_o3[1], oz = ray_o3[2], dxr = ray_d3[0], dyr = ray_d3[1], dzr = ray_d3[2];
            const float tt = t_grp;
            const f32x2 cxy = (f32x2){ox, oy} + (f32x2){tt, tt} * (f32x2){dxr, dyr};
            const float cz = oz + tt * dzr;
            f32x2 qxy; float qz;
            if (p.scale_is_pow2) { qxy = cxy * (f32x2){p.inv_scale, p.inv_scale}; qz = cz * p.inv_scale; }
            else { qxy = (f32x2){cxy.x / p.scale, cxy.y / p.scale}; qz = cz / p.scale; }
            const f32x2 one2 = {1.0f, 1.0f};
            const f32x2 iA = ((f32x2){qxy.x, qxy.y} + one2) * (f32x2){sx, sy};
            const f32x2 iB = ((f32x2){qxy.y, qz} + one2) * (f32x2){sx, sy};
            const float iv[4] = {iA.x, iA.y, iB.x, iB.y};
            const float lim[4] = {(float)p.W, (float)p.H, (float)p.W, (float)p.H};
            const int nn[4] = {p.W, p.H, p.W, p.H};
            f32x2 T[4];
            int i0[4], ia[4], ib[4];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const float f = floorf(iv[a]);
                const float tw = iv[a] - f;
                const f32x2 t2 = __builtin_elementwise_fma((f32x2){tw, tw}, (f32x2){-1.0f, 1.0f}, (f32x2){1.0f, 0.0f});
                const float cf = __builtin_amdgcn_fmed3f(f, -2.f, lim[a]);
                const int x0 = (int)cf;
                i0[a] = x0;
                const bool v0 = (unsigned)x0 < (unsigned)nn[a], v1 = (unsigned)(x0 + 1) < (unsigned)nn[a];
                T[a] = (f32x2){v0 ? t2.x : 0.f, v1 ? t2.y : 0.f};
                ia[a] = min(max(x0, 0), nn[a] - 1);
                ib[a] = min(max(x0 + 1, 0), nn[a] - 1);
            }
            if (TAPS) {
                if (p.tap_idx && gok) {
                    int32_t* tdst = p.tap_idx + ((int64_t)gray * S + ks) * 6;
                    tdst[0] = i0[0]; tdst[1] = i0[1]; tdst[2] = i0[0]; tdst[3] = i0[3]; tdst[4] = i0[2]; tdst[5] = i0[3];
                }
            }
            const uint32_t rowb = (uint32_t)p.W * (F * 4u);
            const int ua[3] = {0, 0, 2}, va[3] = {1, 3, 3};
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
                const f32x2 wn = T[ua[pl]] * (f32x2){T[va[pl]].x, T[va[pl]].x};
                const f32x2 ws2 = T[ua[pl]] * (f32x2){T[va[pl]].y, T[va[pl]].y};
                const uint32_t ca = (uint32_t)ia[ua[pl]] * (F * 4u) + tid_adj, cb = (uint32_t)ib[ua[pl]] * (F * 4u) + tid_adj;
                const uint32_t ra = __umul24((uint32_t)ia[va[pl]], rowb), rb = __umul24((uint32_t)ib[va[pl]], rowb);
                tab[(pl * 2 + 0) * TP + wslot] = make_uint4(__float_as_uint(wn.x), __float_as_uint(wn.y), __float_as_uint(ws2.x), __float_as_uint(ws2.y));
                tab[(pl * 2 + 1) * TP + wslot] = make_uint4(ra + ca, ra + cb, rb + ca, rb + cb);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        f32x4 tapA[3][4][FQ / 4], tapB[3][4][FQ / 4];
        // The table rows of a tile -- 3 x (4 weights) for its blend, 3 x (4 texel offsets) for the loads that refill its buffer -- are
        // requested together and ahead of their use: one LDS round trip per tile instead of two, and none of it exposed.
        // (address = one loop-invariant vector base (this lane's ray) + ONE scalar offset (table half, sample slot) + an immediate (plane, row kind): a
        //  single v_add per call.  Left to itself the compiler rebuilt the address from `tb`, `j` and the ray with 4-5 vector instructions per call --
        //  9 per tile on the issue port the matrix pipe shares.)
        const uint4* const rowbase = atab + gpt;
        auto read_rows = [&](uint4 (&r)[3], int tb, int j, int which) {                // which: 0 = weights, 1 = offsets
            const int so = __builtin_amdgcn_readfirstlane(tb * (6 * TP) + j * TS);
            const uint4* const tab = rowbase + so;
#pragma unroll
            for (int pl = 0; pl < 3; pl++) r[pl] = tab[(pl * 2 + which) * TP];
        };
        auto issue = [&](f32x4 (&T)[3][4][FQ / 4], const uint4 (&o4)[3], uint32_t soff_b) {
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
                const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane((int)(soff_b + (uint32_t)pl * plane_bytes));     // (an SGPR for the asm's "s" operand)
                const uint32_t ov[4] = {o4[pl].x, o4[pl].y, o4[pl].z, o4[pl].w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(T[pl][t][0]) : "v"(ov[t]), "s"(dsc), "s"(so));
                    if constexpr (FQ / 4 > 1) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:64" : "=v"(T[pl][t][FQ / 4 - 1]) : "v"(ov[t]), "s"(dsc), "s"(so));
                }
            }
        };
        // wait until at most NEWER vector-memory operations are outstanding, then hand the buffer to the compiler: every later use of a tap
        // register depends on one of these statements, and volatile asm statements keep their order
        auto await = [&](f32x4 (&T)[3][4][FQ / 4], auto newer) {
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(decltype(newer)::value) : "memory");
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
                if constexpr (FQ / 4 > 1)
                    asm volatile("" : "+v"(T[pl][0][0]), "+v"(T[pl][0][1]), "+v"(T[pl][1][0]), "+v"(T[pl][1][1]), "+v"(T[pl][2][0]), "+v"(T[pl][2][1]),
                                 "+v"(T[pl][3][0]), "+v"(T[pl][3][1]));
                else
                    asm volatile("" : "+v"(T[pl][0][0]), "+v"(T[pl][1][0]), "+v"(T[pl][2][0]), "+v"(T[pl][3][0]));
            }
        };
        // g[16 channels of a pass] = sum over 3 planes x 4 taps of weight * texel: ONE fma chain per channel pair in tap order 0..11 (the
        // order of triplane_walk_kernel), the NP * 2 chains of a tile interleaved so that no packed fma waits for its predecessor.
        auto blend = [&](const f32x4 (&T)[3][4][FQ / 4], const uint4 (&w4)[3], f32x2 (&g)[FQ / 2]) {
            auto tp = [&](int jt, int s) -> f32x2 { const f32x4 v = T[jt >> 2][jt & 3][s >> 1]; return (s & 1) ? (f32x2){v[2], v[3]} : (f32x2){v[0], v[1]}; };
            float w[12];
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
                w[pl * 4 + 0] = __uint_as_float(w4[pl].x); w[pl * 4 + 1] = __uint_as_float(w4[pl].y); w[pl * 4 + 2] = __uint_as_float(w4[pl].z); w[pl * 4 + 3] = __uint_as_float(w4[pl].w);
            }
#pragma unroll
            for (int s = 0; s < FQ / 2; s++) g[s] = tp(0, s) * (f32x2){w[0], w[0]};
#pragma unroll
            for (int jt = 1; jt < 12; jt++)
#pragma unroll
                for (int s = 0; s < FQ / 2; s++) g[s] = __builtin_elementwise_fma(tp(jt, s), (f32x2){w[jt], w[jt]}, g[s]);
            // pin the sums HERE: left alone, the compiler sinks the whole fma chain to its use behind the ring wait -- past the loads that
            // refill this buffer -- and then has three tiles of taps live (it spilled 129 registers doing so)
#pragma unroll
            for (int s = 0; s < FQ / 2; s++) asm volatile("" : "+v"(g[s]));
        };
        const int ring_lane = walk2_ring_off(gpt, gc4, L::RP2, L::RPO);
        int n = 0, slot = 0, seen = 0;
        auto publish = [&](const f32x2 (&g)[FQ / 2]) {
            if (n - seen >= NS) {                                        // ring full: the consumer is NS tiles behind (the common case never enters)
                int spin = 0;
                do {
                    seen = lds_peek(ctr + 1);
                    if (n - seen < NS) break;
                    __builtin_amdgcn_s_sleep(8);
                } while (++spin < WALK2_SPIN);
                // timeout: report and END THIS WAVE (the partner's own bounded wait then runs out once, ~2 ms, and it ends too).  No "stop
                // waiting" state is carried through the loop: that state (and `seen` with it) lived in vector registers and cost ~8 vector
                // instructions per tile on each side of the ring -- on an issue port the matrix pipe shares (round 5)
                if (spin >= WALK2_SPIN) { walk2_fault(p.fault, 1); asm volatile("s_endpgm"); }
            }
            float* dst = ring + slot * RT + ring_lane;
#pragma unroll
            for (int ps = 0; ps < NP; ps++) *(float4*)(dst + 16 * ps) = make_float4(g[2 * ps].x, g[2 * ps].y, g[2 * ps + 1].x, g[2 * ps + 1].y);
            TDGP_ORDER();
            n++;
            lds_poke(ctr + 0, n);
            TDGP_ORDER();
            slot = slot + 1 == NS ? 0 : slot + 1;
        };

        prefetch_group(0, 0);
        soff_cur = soff_nxt = soff_n2;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        address_phase(0, 0);
        {                                                   // group 1 of this pair's march (the next patch's first group when a patch is one group)
            const int g1 = ngroups > 1 ? 1 : 0;
            prefetch_group(g1 / gpp, g1 % gpp);
            soff_nxt = soff_n2;
        }
        {
            uint4 o0[3], o1[3];
            read_rows(o0, 0, 0, 1);
            read_rows(o1, 0, 1, 1);
            issue(tapA, o0, soff_cur);
            issue(tapB, o1, soff_cur);
        }
        int gl = 0, pi = 0;                                 // group within the patch, patch index
        // Two tiles per iteration (buffers A and B), so that a loop body holds 48 + 3 loads -- inside what the hardware's 6-bit counter and
        // the compiler's bookkeeping can express.  The sample's position in its group of four and the table half are run-time scalars.
        for (int t0 = 0; t0 < total; t0 += 2) {
            const int j0 = t0 & 3, g = t0 >> 2, tb = g & 1;
            const bool first = j0 == 0;                     // first half of a group: the next group's table is due
            const bool has_next = g + 1 < ngroups;
            // (The compiler waited for BOTH buffers at the first use of either -- vmcnt(0) at the loop head: it does not keep the order of
            // loads issued in the previous iteration apart.  Measured alternative: both blends first, both refills in one burst, hand-over
            // and address arithmetic under the flight time -- 4 % SLOWER than this order, which hands tile A to the consumer at once.)
            f32x2 gv[FQ / 2];
            // tiles t0 + 2, t0 + 3 (the refills): the second half of this group, or the first half of the next one, whose table was written
            // in the previous iteration.  The tap buffers never sit under a condition (a conditional 96-register definition costs 96
            // moves): after the last group the look-ahead re-reads its table -- harmless extra loads, once per block.
            // (integer arithmetic on purpose: a bool turned into 0 / 1 is a v_cndmask, and everything computed from it -- this table half, the row
            //  addresses below -- then runs on the vector unit)
            int hn;                                                           // has_next as 0 / 1 (asm: the compiler turns the shift back into a compare + v_cndmask)
            asm("s_lshr_b32 %0, %1, 31" : "=s"(hn) : "s"(__builtin_amdgcn_readfirstlane(g + 1 - ngroups)));
            const int tbn = tb ^ ((j0 >> 1) & hn);
            const int jn = 2 - j0;
            const uint32_t soffn = first ? soff_cur : soff_nxt;
            uint4 wA[3], oA[3], wB[3], oB[3];
            read_rows(wA, tb, j0, 0);
            read_rows(oA, tbn, jn, 1);
            __builtin_amdgcn_sched_barrier(0);
            await(tapA, std::integral_constant<int, 3 * FQ>());      // younger than A's loads: B's 3 * FQ refills
            // (sched_barrier: the loads of a buffer must not be hoisted above the blend that frees it)
            blend(tapA, wA, gv);
            __builtin_amdgcn_sched_barrier(0);
            read_rows(wB, tb, j0 + 1, 0);                    // tile B's rows travel under the hand-over / address arithmetic / loads of A
            read_rows(oB, tbn, jn + 1, 1);
            __builtin_amdgcn_sched_barrier(0);
            publish(gv);
            __builtin_amdgcn_sched_barrier(0);
            // buffer A is free here: the register-hungry address arithmetic of the NEXT group runs now, on the values requested one iteration ago
            if (first && has_next) address_phase(tb ^ 1, (gl + 1 == gpp ? 0 : gl + 1) * 4);
            __builtin_amdgcn_sched_barrier(0);
            {   // request the inputs of the group whose address arithmetic comes next: g + 2 in the second half of group g (consumed one
                // iteration from now); in a first half the request is a repeat of the previous one (nothing else may be overwritten yet).
                // Issued BEFORE A's refills: the wait for A at the next loop head then covers these three loads too.
                int gq = gl + (first ? 1 : 2), pq = pi;
                while (gq >= gpp) { gq -= gpp; pq++; }
                if (pq >= npl) { pq = npl - 1; gq = gpp - 1; }
                prefetch_group(pq, gq);
            }
            __builtin_amdgcn_sched_barrier(0);
            issue(tapA, oA, soffn);
            __builtin_amdgcn_sched_barrier(0);
            await(tapB, std::integral_constant<int, 3 * FQ + 3>());  // younger than B's loads: the three small loads and A's 3 * FQ refills
            blend(tapB, wB, gv);
            __builtin_amdgcn_sched_barrier(0);
            issue(tapB, oB, soffn);
            __builtin_amdgcn_sched_barrier(0);
            publish(gv);
            __builtin_amdgcn_sched_barrier(0);
            if (!first) {
                soff_cur = soff_nxt; soff_nxt = soff_n2;
                if (gl + 1 == gpp) { gl = 0; pi++; } else gl++;
            }
        }
        return;
    }

    // ==================================================================== consumer
    {
        float4* const obuf = (float4*)(smem + L::off_obuf + pair * L::obuf_bytes);
        const int pt = l & 15, q = l >> 4;
        float a0r[MT * FQ], a1r[MT * 4];
        f32x4 b0r[MT];
#pragma unroll
        for (int i = 0; i < MT * FQ; i++) a0r[i] = a0s[i * 64 + l];
#pragma unroll
        for (int i = 0; i < MT * 4; i++) a1r[i] = a1s[i * 64 + l];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) b0r[mt] = *(const f32x4*)(b0s + mt * 16 + 4 * q);
        const f32x4 o4init = q == 0 ? (f32x4){p.b1[0], p.b1[1], p.b1[2], p.b1[3]} : (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* const rd = ring + walk2_ring_off(pt, q, L::RP2, L::RPO);

        int n = 0, slot = 0, seen = 0, k = 0, pi = 0;
        int fray = 0;
        bool fok = false;
        auto setup_patch = [&](int i) {
            int b, py, px;
            decode(lb + i * nb, b, py, px);
            fray = ray_of(b, py, px, l >> 2, fok);          // the ray whose parked results this lane flushes
        };
        auto fetch = [&](f32x4 (&g)[NP], int want, int sl) {                 // wait until tile `want` is in the ring, then read it from slot sl
            if (seen <= want) {
                int spin = 0;
                do {
                    seen = lds_peek(ctr + 0);
                    if (seen > want) break;
                    __builtin_amdgcn_s_sleep(1);
                } while (++spin < WALK2_SPIN);
                if (spin >= WALK2_SPIN) { walk2_fault(p.fault, 2); asm volatile("s_endpgm"); }     // see publish()
            }
            TDGP_ORDER();
#pragma unroll
            for (int ps = 0; ps < NP; ps++) g[ps] = *(const f32x4*)(rd + sl * RT + 16 * ps);
        };
        // one tile: gc = its features (requested one tile ago), gn = where the next tile's are requested into
        auto step = [&](f32x4 (&gc)[NP], f32x4 (&gn)[NP]) {
            // wait for THIS tile's features (requested a whole tile ago) before any new LDS traffic is queued behind them: the compiler's
            // wait count for a value requested in the previous iteration is conservative, and placed after the new requests it would wait
            // for those as well (a full LDS round trip per tile)
#pragma unroll
            for (int ps = 0; ps < NP; ps++) asm volatile("" : "+v"(gc[ps]));
            TDGP_ORDER();
            lds_poke(ctr + 1, n + 1);                        // slot of tile n is free: its reads were issued before this store (LDS is in order)
            TDGP_ORDER();
            const int nslot = slot + 1 == NS ? 0 : slot + 1;
            if (n + 1 < total) fetch(gn, n + 1, nslot);
            f32x4 acc[MT];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = b0r[mt];
#pragma unroll
            for (int ps = 0; ps < NP; ps++) {
                const float gp[4] = {gc[ps][0], gc[ps][1], gc[ps][2], gc[ps][3]};
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0r[mt * FQ + ps * 4 + i], gp[i], acc[mt], 0, 0, 0);
            }
            // (layer 2 as four independent chains of 4x4x1 instead of two: measured, no change -- the pure consumer stays at 3.1 ms)
            f32x4 o4[2] = {o4init, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const f32x2 c02 = {0.2f, 0.2f};
                const f32x2 lo = (f32x2){acc[mt][0], acc[mt][1]} * c02, hi = (f32x2){acc[mt][2], acc[mt][3]} * c02;
                const float sc[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float h = __builtin_amdgcn_fmed3f(acc[mt][r], sc[r], 3.4028234663852886e38f);
                    o4[r & 1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a1r[mt * 4 + r], h, o4[r & 1], 0, 0, 0);
                }
            }
            const f32x2 s01 = (f32x2){o4[0][0], o4[0][1]} + (f32x2){o4[1][0], o4[1][1]}, s23 = (f32x2){o4[0][2], o4[0][3]} + (f32x2){o4[1][2], o4[1][3]};
            obuf[pt * 33 + (k & 7) * 4 + q] = make_float4(s01.x, s01.y, s23.x, s23.y);       // partial sum over this lane's quarter of the hidden units
            if ((k & 7) == 7 || k + 1 == Sq) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int k0 = k & ~7, nk = (k & 7) + 1;
                const int fr = l >> 2, j = (l & 3) * 2;
                float4 v[2];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const float4 p0 = obuf[fr * 33 + (j + e) * 4 + 0], p1 = obuf[fr * 33 + (j + e) * 4 + 1];
                    const float4 p2 = obuf[fr * 33 + (j + e) * 4 + 2], p3 = obuf[fr * 33 + (j + e) * 4 + 3];
                    // (q0 + q1) + (q2 + q3): the order of the two xor-shuffles of triplane_walk_kernel
                    v[e] = make_float4((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y), (p0.z + p1.z) + (p2.z + p3.z), (p0.w + p1.w) + (p2.w + p3.w));
                    if (p.marcher == 1) {
                        v[e].x = (1.0f / (1.0f + expf(-v[e].x))) * (1.f + 2.f * 0.001f) - 0.001f;
                        v[e].y = (1.0f / (1.0f + expf(-v[e].y))) * (1.f + 2.f * 0.001f) - 0.001f;
                        v[e].z = (1.0f / (1.0f + expf(-v[e].z))) * (1.f + 2.f * 0.001f) - 0.001f;
                    }
                }
                float4* dst = (float4*)p.rgbs + (int64_t)fray * S + kb + k0 + j;
                if (p.snoise && fok) {
                    const float* np = p.snoise + (int64_t)fray * S + kb + k0 + j;
                    if (j < nk) v[0].w = __fadd_rn(v[0].w, __fmul_rn(np[0], p.snoise_std));
                    if (j + 1 < nk) v[1].w = __fadd_rn(v[1].w, __fmul_rn(np[1], p.snoise_std));
                }
                if (fok) {
                    if (j < nk) dst[0] = v[0];
                    if (j + 1 < nk) dst[1] = v[1];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            n++;
            slot = nslot;
            if (++k == Sq) { k = 0; pi++; if (pi < npl) setup_patch(pi); }
        };
        setup_patch(0);
        f32x4 gA[NP], gB[NP];
        fetch(gA, 0, 0);
        while (n < total) {
            step(gA, gB);
            if (n < total) step(gB, gA);
        }
    }
}

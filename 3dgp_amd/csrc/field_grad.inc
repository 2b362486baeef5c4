// field_grad.inc -- what the two tri-plane field gradient kernels share: triplane_field_grad_kernel (render_grad.hip, two-layer decoders)
// and triplane_field_deep_grad_kernel (field_deep.hip, 3 and 4 layers).  Their MLP middles (stages 2-5) and their reductions differ -- the
// two-layer kernel keeps 16 bias-gradient registers per tile in the accumulator layout, the deep one sums the A operands it reads, so the
// summation orders and the last bits of d_b0 differ -- and stay in their files.  The bilinear geometry of the gradient kernels is here only.
//
// Included twice per translation unit:
//   * at namespace scope (FIELD_GRAD_STAGE undefined): the types and helpers;
//   * inside the tile loop of a kernel, with FIELD_GRAD_STAGE = 1 or 6: the statements of that stage, as text.  (Text, not functions:
//     the forward body showed that moving statements of these kernels into functions or lambdas changes register allocation and waits,
//     and the listings of both kernels are held fixed.)  A stage reads and declares plain names of the kernel it stands in:
//       reads     p (planes, coords, d_out, d_planes, d_coords, P, F, H, W, scale), gl [32 pts][FG_PITCH], hl (scratch once the MLP
//                 middle is done, >= 32 * 24 floats), l32, half, valid, gpc, b, sx, sy, fh;  stage 6 also dg transposed into gl
//       declares  stage 1: cp, q, tw_, to_, fr_, in_, gsum, acc3, dout4 (stage 6 reads tw_, to_, fr_, in_ again)
// Each stage ends with the wave-level sync that its readers need.
#ifndef FIELD_GRAD_STAGE

typedef float fg_f32x16 __attribute__((ext_vector_type(16)));
constexpr int FG_PITCH = 33;                                  // pitch of every [..][32] panel of the gradient kernels (odd: rows and columns both conflict-free)

// row of a 32x32 accumulator tile that register r of half-wave `half` holds (v_mfma_f32_32x32x2_f32), in tile mt of a [32 MT] panel
__device__ __forceinline__ int fg_row_of(int mt, int r, int half) { return mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half; }

// the lanes of a wave exchange data through LDS: make the writes visible, keep the compiler from moving accesses across
__device__ __forceinline__ void fg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

#elif FIELD_GRAD_STAGE == 1
        // ---- 1. geometry + gather: coordinates -> tap weights / offsets / fractions / in-range masks, blended features -> gl, zero beyond F
        const float* cp = p.coords + gpc * 3;
        const float q[3] = {cp[0] / p.scale, cp[1] / p.scale, cp[2] / p.scale};
        float tw_[3][4];
        int to_[3][4];
        float fr_[3][2];                                      // (tw, tn): fractional position inside the texel cell, per plane
        int in_[3];                                           // in-range mask of the four taps (bit t), per plane
        float gsum[16];
#ifdef FIELD_GRAD_ZERO_GSUM                                   // render_grad.hip asks for it: a dead store the compiler drops, but without it, at this
#pragma unroll                                                // place, the two-layer kernel's listing moves (and the deep kernel's moves with it)
        for (int c = 0; c < 16; c++) gsum[c] = 0.f;
#endif
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
        // features of the point: [pt][f], zero beyond F
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if (c < fh) gl[l32 * FG_PITCH + half * fh + c] = gsum[c];
        }
        for (int f = p.F + half; f < 32; f += 2) gl[l32 * FG_PITCH + f] = 0.f;
        const float4 dout4 = valid ? *(const float4*)(p.d_out + gpc * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        fg_wave_sync();

#elif FIELD_GRAD_STAGE == 6
        // ---- 6a. gradient w.r.t. the sample position (grid_sampler's grid gradient; what a camera is trained through, loss.py:69-83):
        //     d ix = sum_c dg_c/3 [(ne - nw) ts + (se - sw) tn],   d iy = sum_c dg_c/3 [(sw - nw) te + (se - ne) tw]
        // taps outside the plane read as zero (torch grid_sampler_2d_backward), then x (size - 1) / 2 (align_corners) and / scale.
        // lane = (point, channel half): the taps are fetched again (cache hits: this wave gathered them a moment ago).
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
                        const float* gq = gl + l32 * FG_PITCH + half * fh + 4 * c4;
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
                dq[pl == 2 ? 1 : 0] += gix * sx;                 // planes (x,y), (x,z), (y,z): width <- first coordinate
                dq[pl == 0 ? 1 : 2] += giy * sy;
            }
            if (half == 0 && valid) {
                const float k = 1.0f / (3.0f * p.scale);
                float* dc = p.d_coords + gpc * 3;
                dc[0] = dq[0] * k; dc[1] = dq[1] * k; dc[2] = dq[2] * k;
            }
        }
        // ---- 6. scatter: d_plane[tap] += w_tap * dg / 3 ------------------------------------------------------------------------
        // Transposed through LDS so that ONE atomic instruction adds the 32 channels of one tap (a 128-B line) per half-wave:
        // issued from the accumulator layout (lane = point) every instruction touched 64 different lines and the kernel ran at
        // the L2's atomic line rate (82 ms for 8.4 M points).  What bounds it now (round 4, tools/dev/ubench_atomics.hip): the chip
        // retires 10.3 G such lines per second = 0.6 lane-atomics per clock and CU -- the same for a 24-MiB and a 1.6-GiB target, with
        // or without sc1 / nt, and with every XCD kept inside its own eighth of the target -- so 12 lines per point are 1.17 ms per
        // million points whatever the access pattern; only fewer lines (an LDS window that merges the taps of neighbouring rays before
        // they leave the CU) can lower it.
        if (p.d_planes) {
            int* tab_off = (int*)hl;                             // [32 pts][12 taps] float offset into d_planes (the h / dh_pre panels are dead now)
            float* tab_w = hl + 32 * 12;
#pragma unroll
            for (int pl = 0; pl < 3; pl++)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (((pl * 4 + t) & 1) == half) {
                        tab_off[l32 * 12 + pl * 4 + t] = (int)((((int64_t)b * 3 + pl) * p.H * p.W) * p.F) + to_[pl][t];
                        tab_w[l32 * 12 + pl * 4 + t] = tw_[pl][t] / 3.0f;
                    }
            fg_wave_sync();
            for (int e2 = 0; e2 < 32 * 12 / 2; e2++) {
                const int e = 2 * e2 + half;                    // (point, tap) handled by this half-wave; lane = channel
                const float wt = tab_w[e];
                if (wt != 0.f && l32 < p.F) unsafeAtomicAdd(p.d_planes + tab_off[e] + l32, wt * gl[(e / 12) * FG_PITCH + l32]);
            }
        }
        fg_wave_sync();

#endif
#undef FIELD_GRAD_STAGE
#undef FIELD_GRAD_ZERO_GSUM

// augment.hip -- the ADA augmentation pipe (src/training/augment.py of the reference) on the device.
//
//   tdgp_augment_params    augment.py:199-268, 313-354, 393-402, 423-436: every per-sample parameter in one launch, one lane per sample.
//                          The scalars (gates, angles, scales, offsets; erfinv / exp2 correctly rounded) are the reference's fp32 ones, its
//                          order of operations kept; the 3x3 / 4x4 products run in fp64 and round once at the end -- composed in fp32 the
//                          translation column alone carried 2 ulp (4e-6 pixels), as much as the whole fp32 pipe of the reference.
//   tdgp_augment_geom      augment.py:276-305: margins, reflect pad, x2 sym6 upsampling, affine bilinear sampling, sym6 x2 downsampling, crop
//   tdgp_augment_geom_adj  its adjoint (= its gradient: given the parameters the operator is linear in the image)
//   tdgp_augment_color     augment.py:363-382, 427, 437-442: colour matrix, additive noise, cutout mask; with `transposed` its own adjoint
//
// Geometry.  With f the 12 normalised sym6 taps, m = [mx0, my0, mx1, my1] the margins and G the user-level inverse transform, the
// reference computes (one axis shown)
//   xp[p]  = x[reflect(p)]                         p in [-m0, W + m1)                       reflect pad
//   u[n]   = sum_p 2 f[5 + n - 2 p] xp[p]          n in [-2 m0, 2 (W + m1))                 upsample2d, zeros beyond xp
//   s[j]   = bilinear(u, h(j)), zeros outside u    j in [0, 2 W + 12)                       affine_grid + grid_sample, align_corners=False
//   out[o] = sum_k f[k] s[2 o + 1 + k]             o in [0, W)                              downsample2d, padding -6, flipped filter
// where, after collecting the five conjugations of augment.py:291-300, the sampling position in texels of u (counted from the unpadded
// image's first texel) is  h(j) = 2 G ((j - [W, H] - 5) / 2) + [W, H] - 1.  The margins enter only through the ranges of p and n.
// Neither xp nor u exists in memory: a warped sample is a 7 x 7 weighted sum of reflect-indexed input pixels (the two texels a bilinear
// sample touches per axis share their input taps), and the window of samples an output tile needs is staged in LDS for the separable
// down pass.  Positions h(j) and the margins are evaluated in fp64 from the fp32 matrix, so the integer decisions (floor, ceil) are those
// of exact arithmetic on the given parameters; pixel sums are fp32.
// The adjoint walks the same chain backwards with one writer per value and no atomics: the same bytes on every run.
#include "common.h"
#include <string.h>

namespace {

constexpr int NT = 12;                 // taps of the sym6 low-pass
constexpr int TILE = 16;               // output tile (forward) / input tile (adjoint)
constexpr int WIN = 2 * TILE + 10;     // warped samples (forward) / hi-res texels (adjoint) one tile needs per axis
constexpr int CC = 4;                  // channels staged together

struct AugCfg {
    float xflip, rotate90, xint, xint_max;
    float scale, rotate, aniso, xfrac, scale_std, rotate_max, aniso_std, xfrac_std;
    float brightness, contrast, lumaflip, hue, saturation, brightness_std, contrast_std, hue_max, saturation_std;
    float imgfilter, band[4], imgfilter_std;
    float noise, cutout, noise_std, cutout_size;
};
static_assert(sizeof(AugCfg) == TDGP_AUGMENT_CFG_FLOATS * sizeof(float), "AugCfg layout");

// columns of the uniform / normal draw blocks
enum { U_XFLIP_I, U_XFLIP_G, U_ROT90_I, U_ROT90_G, U_XINT_X, U_XINT_Y, U_XINT_G, U_SCALE_G, U_ROT0_T, U_ROT0_G, U_ANISO_G, U_ROT1_T, U_ROT1_G,
       U_XFRAC_G, U_BRIGHT_G, U_CONTRAST_G, U_LUMA_I, U_LUMA_G, U_HUE_T, U_HUE_G, U_SAT_G, U_FILT_G0, U_FILT_G1, U_FILT_G2, U_FILT_G3,
       U_NOISE_G, U_CUT_G, U_CUT_X, U_CUT_Y, U_COUNT };
enum { N_SCALE, N_ANISO, N_XFRAC_X, N_XFRAC_Y, N_BRIGHT, N_CONTRAST, N_SAT, N_FILT0, N_FILT1, N_FILT2, N_FILT3, N_NOISE, N_COUNT };
static_assert(U_COUNT == TDGP_AUGMENT_UNIFORMS && N_COUNT == TDGP_AUGMENT_NORMALS, "draw layout");

template <int N>
struct Mat { double m[N][N]; };

template <int N>
__device__ __forceinline__ Mat<N> eye() {
    Mat<N> r;
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) r.m[i][j] = i == j ? 1.0 : 0.0;
    return r;
}
template <int N>
__device__ __forceinline__ Mat<N> mul(const Mat<N>& a, const Mat<N>& b) {
    Mat<N> r;
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            double s = a.m[i][0] * b.m[0][j];
            for (int k = 1; k < N; k++) s = s + a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
__device__ __forceinline__ Mat<3> scale2d(double sx, double sy) { Mat<3> r = eye<3>(); r.m[0][0] = sx; r.m[1][1] = sy; return r; }
__device__ __forceinline__ Mat<3> translate2d(double tx, double ty) { Mat<3> r = eye<3>(); r.m[0][2] = tx; r.m[1][2] = ty; return r; }
__device__ __forceinline__ Mat<3> rotate2d(double t) {
    Mat<3> r = eye<3>();
    r.m[0][0] = cos(t); r.m[0][1] = sin(-t); r.m[1][0] = sin(t); r.m[1][1] = cos(t);
    return r;
}

constexpr float PI_F = 3.14159265358979323846f;
constexpr double PI_D = 3.14159265358979323846;
// exp2 of an fp32 argument, correctly rounded to fp32 (the scalar the reference holds), widened for the matrices
__device__ __forceinline__ double exp2r(float x) { return (double)(float)exp2((double)x); }

__global__ __launch_bounds__(64) void augment_params_kernel(AugCfg cfg, const float* __restrict__ p_ptr, int B, int H, int W, int num_channels,
                                                            const float* __restrict__ un, const float* __restrict__ nr, int use_q, float q,
                                                            float* __restrict__ G_out, float* __restrict__ C_out, float* __restrict__ gains,
                                                            float* __restrict__ sigma_out, float* __restrict__ cutout) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float p = p_ptr[0];
    const float* u = use_q ? nullptr : un + (int64_t)b * U_COUNT;
    const float* n = use_q ? nullptr : nr + (int64_t)b * N_COUNT;
    const float q2 = q * 2.0f - 1.0f;                              // debug_percentile * 2 - 1
    const float qe = use_q ? (float)erfinv((double)q2) : 0.0f;
    const float w = (float)W, h = (float)H;

    if (G_out) {
        Mat<3> G = eye<3>();
        if (cfg.xflip > 0) {
            float i = use_q ? floorf(q * 2.0f) : (u[U_XFLIP_G] < cfg.xflip * p ? floorf(u[U_XFLIP_I] * 2.0f) : 0.0f);
            G = mul(G, scale2d(1.0 / (1.0 - 2.0 * (double)i), 1.0));
        }
        if (cfg.rotate90 > 0) {
            float i = use_q ? floorf(q * 4.0f) : (u[U_ROT90_G] < cfg.rotate90 * p ? floorf(u[U_ROT90_I] * 4.0f) : 0.0f);
            G = mul(G, rotate2d(-((-PI_D / 2.0) * (double)i)));
        }
        if (cfg.xint > 0) {
            float tx, ty;
            if (use_q) {
                tx = ty = q2 * cfg.xint_max;
            } else {
                const bool on = u[U_XINT_G] < cfg.xint * p;
                tx = on ? (u[U_XINT_X] * 2.0f - 1.0f) * cfg.xint_max : 0.0f;
                ty = on ? (u[U_XINT_Y] * 2.0f - 1.0f) * cfg.xint_max : 0.0f;
            }
            G = mul(G, translate2d(-(double)rintf(tx * w), -(double)rintf(ty * h)));
        }
        if (cfg.scale > 0) {
            const double s = use_q ? exp2r(qe * cfg.scale_std) : (u[U_SCALE_G] < cfg.scale * p ? exp2r(n[N_SCALE] * cfg.scale_std) : 1.0f);
            G = mul(G, scale2d(1.0 / s, 1.0 / s));
        }
        float t0 = 1.0f - cfg.rotate * p;
        t0 = t0 < 0.0f ? 0.0f : (t0 > 1.0f ? 1.0f : t0);
        const float p_rot = 1.0f - sqrtf(t0);
        if (cfg.rotate > 0) {
            float t = use_q ? (q2 * PI_F) * cfg.rotate_max : (u[U_ROT0_G] < p_rot ? ((u[U_ROT0_T] * 2.0f - 1.0f) * PI_F) * cfg.rotate_max : 0.0f);
            G = mul(G, rotate2d(-(-(double)t)));
        }
        if (cfg.aniso > 0) {
            const double s = use_q ? exp2r(qe * cfg.aniso_std) : (u[U_ANISO_G] < cfg.aniso * p ? exp2r(n[N_ANISO] * cfg.aniso_std) : 1.0f);
            G = mul(G, scale2d(1.0 / s, 1.0 / (1.0 / s)));
        }
        if (cfg.rotate > 0) {
            float t = use_q ? 0.0f : (u[U_ROT1_G] < p_rot ? ((u[U_ROT1_T] * 2.0f - 1.0f) * PI_F) * cfg.rotate_max : 0.0f);
            G = mul(G, rotate2d(-(-(double)t)));
        }
        if (cfg.xfrac > 0) {
            float tx, ty;
            if (use_q) {
                tx = ty = qe * cfg.xfrac_std;
            } else {
                const bool on = u[U_XFRAC_G] < cfg.xfrac * p;
                tx = on ? n[N_XFRAC_X] * cfg.xfrac_std : 0.0f;
                ty = on ? n[N_XFRAC_Y] * cfg.xfrac_std : 0.0f;
            }
            G = mul(G, translate2d(-((double)tx * (double)w), -((double)ty * (double)h)));
        }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) G_out[(int64_t)b * 9 + i * 3 + j] = (float)G.m[i][j];
    }

    if (C_out) {
        Mat<4> C = eye<4>();
        const double v = 1.0 / 1.7320508075688772;                  // luma axis [1, 1, 1, 0] / sqrt(3)
        const double vv = v * v;
        if (cfg.brightness > 0) {
            float bb = use_q ? qe * cfg.brightness_std : (u[U_BRIGHT_G] < cfg.brightness * p ? n[N_BRIGHT] * cfg.brightness_std : 0.0f);
            Mat<4> T = eye<4>();
            T.m[0][3] = T.m[1][3] = T.m[2][3] = (double)bb;
            C = mul(T, C);
        }
        if (cfg.contrast > 0) {
            const double c = use_q ? exp2r(qe * cfg.contrast_std) : (u[U_CONTRAST_G] < cfg.contrast * p ? exp2r(n[N_CONTRAST] * cfg.contrast_std) : 1.0f);
            Mat<4> S = eye<4>();
            S.m[0][0] = S.m[1][1] = S.m[2][2] = c;
            C = mul(S, C);
        }
        if (cfg.lumaflip > 0) {
            float i = use_q ? floorf(q * 2.0f) : (u[U_LUMA_G] < cfg.lumaflip * p ? floorf(u[U_LUMA_I] * 2.0f) : 0.0f);
            Mat<4> R = eye<4>();
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++) R.m[a][c] = R.m[a][c] - (2.0 * vv) * (double)i;
            C = mul(R, C);
        }
        if (cfg.hue > 0 && num_channels > 1) {
            float t = use_q ? (q2 * PI_F) * cfg.hue_max : (u[U_HUE_G] < cfg.hue * p ? ((u[U_HUE_T] * 2.0f - 1.0f) * PI_F) * cfg.hue_max : 0.0f);
            const double s = sin((double)t), c = cos((double)t), cc = 1.0 - c;
            Mat<4> R = eye<4>();
            R.m[0][0] = vv * cc + c;     R.m[0][1] = vv * cc - v * s; R.m[0][2] = vv * cc + v * s;
            R.m[1][0] = vv * cc + v * s; R.m[1][1] = vv * cc + c;     R.m[1][2] = vv * cc - v * s;
            R.m[2][0] = vv * cc - v * s; R.m[2][1] = vv * cc + v * s; R.m[2][2] = vv * cc + c;
            C = mul(R, C);
        }
        if (cfg.saturation > 0 && num_channels > 1) {
            const double s = use_q ? exp2r(qe * cfg.saturation_std) : (u[U_SAT_G] < cfg.saturation * p ? exp2r(n[N_SAT] * cfg.saturation_std) : 1.0f);
            Mat<4> S;
            for (int a = 0; a < 4; a++)
                for (int c = 0; c < 4; c++) {
                    const double o = (a < 3 && c < 3) ? vv : 0.0;
                    S.m[a][c] = o + ((a == c ? 1.0 : 0.0) - o) * s;
                }
            C = mul(S, C);
        }
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) C_out[(int64_t)b * 16 + i * 4 + j] = (float)C.m[i][j];
    }

    if (gains) {
        const double ep[4] = {10.0 / 13.0, 1.0 / 13.0, 1.0 / 13.0, 1.0 / 13.0};
        double g[4] = {1.0, 1.0, 1.0, 1.0};
        for (int i = 0; i < 4; i++) {
            double ti;
            if (use_q) ti = cfg.band[i] > 0 ? exp2r(qe * cfg.imgfilter_std) : 1.0f;
            else ti = u[U_FILT_G0 + i] < (cfg.imgfilter * p) * cfg.band[i] ? exp2r(n[N_FILT0 + i] * cfg.imgfilter_std) : 1.0f;
            double t[4] = {1.0, 1.0, 1.0, 1.0};
            t[i] = ti;
            double s = ep[0] * (t[0] * t[0]);
            for (int k = 1; k < 4; k++) s = s + ep[k] * (t[k] * t[k]);
            s = sqrt(s);
            for (int k = 0; k < 4; k++) g[k] = g[k] * (t[k] / s);
        }
        for (int k = 0; k < 4; k++) gains[(int64_t)b * 4 + k] = (float)g[k];
    }

    if (sigma_out) {
        float s = use_q ? (float)erfinv((double)q) * cfg.noise_std : (u[U_NOISE_G] < cfg.noise * p ? fabsf(n[N_NOISE]) * cfg.noise_std : 0.0f);
        sigma_out[b] = s;
    }

    if (cutout) {
        float size = use_q ? cfg.cutout_size : (u[U_CUT_G] < cfg.cutout * p ? cfg.cutout_size : 0.0f);
        cutout[(int64_t)b * 4 + 0] = size;
        cutout[(int64_t)b * 4 + 1] = size;
        cutout[(int64_t)b * 4 + 2] = use_q ? q : u[U_CUT_X];
        cutout[(int64_t)b * 4 + 3] = use_q ? q : u[U_CUT_Y];
    }
}

// ------------------------------------------------------------------------------------------------------------------------ geometry
struct Margins { int x0, y0, x1, y1; };

// augment.py:277-287, the maximum over the whole batch, by every block for itself (4 B small products): nothing crosses to the host.
__device__ Margins block_margins(const float* __restrict__ G, int B, int H, int W, double (*red)[256]) {
    const double cx = (W - 1) * 0.5, cy = (H - 1) * 0.5;
    double m[4] = {-1e300, -1e300, -1e300, -1e300};
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* g = G + (int64_t)b * 9;
        for (int k = 0; k < 4; k++) {
            const double px = (k == 1 || k == 2) ? cx : -cx, py = (k >= 2) ? cy : -cy;
            const double x = (double)g[0] * px + (double)g[1] * py + (double)g[2];
            const double y = (double)g[3] * px + (double)g[4] * py + (double)g[5];
            m[0] = fmax(m[0], -x); m[1] = fmax(m[1], -y); m[2] = fmax(m[2], x); m[3] = fmax(m[3], y);
        }
    }
    for (int k = 0; k < 4; k++) red[k][threadIdx.x] = m[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = red[threadIdx.x][0];
        for (int i = 1; i < (int)blockDim.x; i++) v = fmax(v, red[threadIdx.x][i]);
        const bool isx = (threadIdx.x & 1) == 0;
        v = v + (6.0 - (isx ? cx : cy));                              // Hz_pad * 2 - c
        const double hi = isx ? W - 1 : H - 1;
        v = !(v > 0.0) ? 0.0 : (v > hi ? hi : v);                     // a NaN matrix pads nothing
        red[threadIdx.x][0] = ceil(v);
    }
    __syncthreads();
    Margins r{(int)red[0][0], (int)red[1][0], (int)red[2][0], (int)red[3][0]};
    __syncthreads();
    return r;
}

struct Affine { double a00, a01, a02, a10, a11, a12; };
__device__ __forceinline__ Affine load_affine(const float* __restrict__ g) {
    return Affine{(double)g[0], (double)g[1], (double)g[2], (double)g[3], (double)g[4], (double)g[5]};
}
// position of warped sample (jx, jy) in texels of the upsampled image, counted from the unpadded image's first texel
__device__ __forceinline__ void sample_pos(const Affine& A, int jx, int jy, int H, int W, double& hx, double& hy) {
    const double qx = (double)(jx - W - 5) * 0.5, qy = (double)(jy - H - 5) * 0.5;
    const double rx = A.a00 * qx + A.a01 * qy + A.a02;
    const double ry = A.a10 * qx + A.a11 * qy + A.a12;
    hx = 2.0 * rx + (double)(W - 1);
    hy = 2.0 * ry + (double)(H - 1);
}
// floor and fraction; false when the position is nowhere near the image (or not a number): the sample reads zeros
__device__ __forceinline__ bool split_pos(double h, int size, int& i0, float& fr) {
    if (!(h > -4.0 * size - 8.0 && h < 6.0 * size + 8.0)) return false;
    const double fl = floor(h);
    i0 = (int)fl;
    fr = (float)(h - fl);
    return true;
}
__device__ __forceinline__ int reflect(int p, int n) {
    p = p < 0 ? -p : p;
    p = p >= n ? 2 * (n - 1) - p : p;
    return p < 0 ? 0 : (p >= n ? n - 1 : p);                          // (only positions whose weight is zero are clamped)
}

// Weights of one warped sample on the 7 input positions p0 .. p0 + 6 of one axis: the bilinear pair of texels (i0, i0 + 1), each the
// x2 sym6 interpolation of 6 input pixels.  f2 = 2 f.
__device__ __forceinline__ void axis_weights(int i0, float fr, int m0, int m1, int size, const float* f2, int& p0, float* wgt, int* idx) {
    const int lo = -2 * m0, hi = 2 * (size + m1);
    const float wa = (i0 >= lo && i0 < hi) ? 1.0f - fr : 0.0f;
    const float wb = (i0 + 1 >= lo && i0 + 1 < hi) ? fr : 0.0f;
    const int a = i0 >> 1;                                            // floor division
    p0 = a - 3;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const int p = p0 + k;
        const int ta = 5 + i0 - 2 * p, tb = ta + 1;
        const float fa = (ta >= 0 && ta < NT) ? f2[ta] : 0.0f;
        const float fb = (tb >= 0 && tb < NT) ? f2[tb] : 0.0f;
        const bool in = p >= -m0 && p < size + m1;
        wgt[k] = in ? wa * fa + wb * fb : 0.0f;
        idx[k] = reflect(p, size);
    }
}

__global__ __launch_bounds__(256) void augment_geom_kernel(const float* __restrict__ x, const float* __restrict__ G, const float* __restrict__ f,
                                                           float* __restrict__ y, int B, int C, int H, int W, int tiles_x) {
    __shared__ double red[4][256];
    __shared__ float s[CC][WIN][WIN + 1];
    __shared__ float tmp[CC][TILE][WIN + 1];
    __shared__ float fs[NT], f2[NT];
    const int b = blockIdx.y;
    const int oy0 = (blockIdx.x / tiles_x) * TILE, ox0 = (blockIdx.x % tiles_x) * TILE;
    if (threadIdx.x < NT) { fs[threadIdx.x] = f[threadIdx.x]; f2[threadIdx.x] = f[threadIdx.x] * 2.0f; }
    const Margins m = block_margins(G, B, H, W, red);                 // (syncs: fs / f2 are visible after it)
    const Affine A = load_affine(G + (int64_t)b * 9);
    const int64_t plane = (int64_t)H * W;
    for (int c0 = 0; c0 < C; c0 += CC) {
        const int nc = min(CC, C - c0);
        const float* xb = x + ((int64_t)b * C + c0) * plane;
        for (int e = threadIdx.x; e < WIN * WIN; e += blockDim.x) {
            const int wy = e / WIN, wx = e % WIN;
            const int jy = 2 * oy0 + 1 + wy, jx = 2 * ox0 + 1 + wx;
            float acc[CC] = {0.0f, 0.0f, 0.0f, 0.0f};
            double hx, hy;
            int ix0, iy0;
            float frx, fry;
            sample_pos(A, jx, jy, H, W, hx, hy);
            if (jy <= 2 * H + 10 && jx <= 2 * W + 10 && split_pos(hx, W, ix0, frx) && split_pos(hy, H, iy0, fry)) {
                float wxv[7], wyv[7];
                int pxv[7], pyv[7], p0;
                axis_weights(ix0, frx, m.x0, m.x1, W, f2, p0, wxv, pxv);
                axis_weights(iy0, fry, m.y0, m.y1, H, f2, p0, wyv, pyv);
#pragma unroll
                for (int ky = 0; ky < 7; ky++) {
                    if (wyv[ky] == 0.0f) continue;
                    const float* row = xb + (int64_t)pyv[ky] * W;
                    for (int c = 0; c < nc; c++) {
                        const float* r = row + c * plane;
                        float t = 0.0f;
#pragma unroll
                        for (int kx = 0; kx < 7; kx++) t = fmaf_(wxv[kx], r[pxv[kx]], t);
                        acc[c] = fmaf_(wyv[ky], t, acc[c]);
                    }
                }
            }
            for (int c = 0; c < CC; c++) s[c][wy][wx] = acc[c];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < CC * TILE * WIN; e += blockDim.x) {       // down pass, rows
            const int wx = e % WIN, oy = (e / WIN) % TILE, c = e / (WIN * TILE);
            float t = 0.0f;
#pragma unroll
            for (int k = 0; k < NT; k++) t = fmaf_(fs[k], s[c][2 * oy + k][wx], t);
            tmp[c][oy][wx] = t;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < CC * TILE * TILE; e += blockDim.x) {      // down pass, columns
            const int ox = e % TILE, oy = (e / TILE) % TILE, c = e / (TILE * TILE);
            if (c < nc && oy0 + oy < H && ox0 + ox < W) {
                float t = 0.0f;
#pragma unroll
                for (int k = 0; k < NT; k++) t = fmaf_(fs[k], tmp[c][oy][2 * ox + k], t);
                y[((int64_t)b * C + c0 + c) * plane + (int64_t)(oy0 + oy) * W + ox0 + ox] = t;
            }
        }
        __syncthreads();
    }
}

// Adjoint, step 1: the transposed down pass.  gs [B*C, 2H+12, 2W+12]: gs[j] = sum_o f[j - 1 - 2 o] dy[o] per axis (rows / columns 0 and
// 2 H + 11 / 2 W + 11, which the forward pass never reads, come out as zeros).
__global__ __launch_bounds__(256) void augment_down_adj_kernel(const float* __restrict__ dy, const float* __restrict__ f, float* __restrict__ gs,
                                                               int64_t planes, int H, int W) {
    const int SH = 2 * H + 12, SW = 2 * W + 12;
    const int64_t total = planes * SH * SW;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int jx = (int)(e % SW), jy = (int)((e / SW) % SH);
        const int64_t pl = e / ((int64_t)SW * SH);
        const float* d = dy + pl * H * W;
        // o with 0 <= j - 1 - 2 o <= 11
        const int oy_lo = max(0, (jy - 12 + 1) >> 1), oy_hi = min(H - 1, (jy - 1) >> 1);
        const int ox_lo = max(0, (jx - 12 + 1) >> 1), ox_hi = min(W - 1, (jx - 1) >> 1);
        float acc = 0.0f;
        if (jy >= 1 && jx >= 1) {
            for (int oy = oy_lo; oy <= oy_hi; oy++) {
                float t = 0.0f;
                for (int ox = ox_lo; ox <= ox_hi; ox++) t = fmaf_(f[jx - 1 - 2 * ox], d[(int64_t)oy * W + ox], t);
                acc = fmaf_(f[jy - 1 - 2 * oy], t, acc);
            }
        }
        gs[e] = acc;
    }
}

// Adjoint, step 2: per tile of input pixels and per reflection image of the tile (the pixel itself, its mirror image left / above of the
// frame, its mirror image right / below), the window of hi-res texels the image's up-filter reaches is staged in LDS -- each texel gathers
// the warped samples whose bilinear footprint covers it: for an affine map those are the integer points inside the pre-image of the
// texel's 2 x 2 neighbourhood, found by walking that parallelogram's bounding box -- then the transposed up-filter is applied separably.
__global__ __launch_bounds__(256) void augment_geom_adj_kernel(const float* __restrict__ gs, const float* __restrict__ G, const float* __restrict__ f,
                                                               float* __restrict__ dx, int B, int C, int H, int W, int tiles_x) {
    __shared__ double red[4][256];
    __shared__ float gu[CC][WIN][WIN + 1];
    __shared__ float tmp[CC][WIN][TILE + 1];
    __shared__ float f2[NT];
    const int b = blockIdx.y;
    const int iy0 = (blockIdx.x / tiles_x) * TILE, ix0 = (blockIdx.x % tiles_x) * TILE;
    if (threadIdx.x < NT) f2[threadIdx.x] = f[threadIdx.x] * 2.0f;
    const Margins m = block_margins(G, B, H, W, red);
    const Affine A = load_affine(G + (int64_t)b * 9);
    const int SH = 2 * H + 12, SW = 2 * W + 12;
    // inverse of the linear part, for the candidate boxes; a singular (or non-finite) map walks every sample
    const double det = A.a00 * A.a11 - A.a01 * A.a10;
    const bool invertible = fabs(det) > 1e-30 && fabs(det) < 1e30;
    const double i00 = A.a11 / det, i01 = -A.a01 / det, i10 = -A.a10 / det, i11 = A.a00 / det;
    const double ex = fabs(i00) + fabs(i01) + 1e-6, ey = fabs(i10) + fabs(i11) + 1e-6;
    // h = L (j - [W, H] - 5) + 2 t + [W, H] - 1
    const double cxo = 2.0 * A.a02 + (double)(W - 1), cyo = 2.0 * A.a12 + (double)(H - 1);
    const int ty = threadIdx.x / TILE, tx = threadIdx.x % TILE;       // the pixel this lane owns
    const int py = iy0 + ty, px = ix0 + tx;
    const int64_t plane = (int64_t)H * W, splane = (int64_t)SH * SW;

    for (int c0 = 0; c0 < C; c0 += CC) {
        const int nc = min(CC, C - c0);
        const float* gb = gs + ((int64_t)b * C + c0) * splane;
        float acc[CC] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int ry = 0; ry < 3; ry++) {
            // pixels of the tile this image exists for: [lo, hi]
            const int ylo = ry == 0 ? 0 : (ry == 1 ? 1 : H - 1 - m.y1), yhi = ry == 0 ? H - 1 : (ry == 1 ? m.y0 : H - 2);
            if (max(ylo, iy0) > min(yhi, iy0 + TILE - 1)) continue;
            const int pminy = ry == 0 ? iy0 : (ry == 1 ? -(iy0 + TILE - 1) : 2 * (H - 1) - (iy0 + TILE - 1));
            for (int rx = 0; rx < 3; rx++) {
                const int xlo = rx == 0 ? 0 : (rx == 1 ? 1 : W - 1 - m.x1), xhi = rx == 0 ? W - 1 : (rx == 1 ? m.x0 : W - 2);
                if (max(xlo, ix0) > min(xhi, ix0 + TILE - 1)) continue;
                const int pminx = rx == 0 ? ix0 : (rx == 1 ? -(ix0 + TILE - 1) : 2 * (W - 1) - (ix0 + TILE - 1));
                const int nby = 2 * pminy - 5, nbx = 2 * pminx - 5;
                for (int e = threadIdx.x; e < WIN * WIN; e += blockDim.x) {
                    const int wy = e / WIN, wx = e % WIN;
                    const int ny = nby + wy, nx = nbx + wx;
                    float a[CC] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (ny >= -2 * m.y0 && ny < 2 * (H + m.y1) && nx >= -2 * m.x0 && nx < 2 * (W + m.x1)) {
                        int jx_lo = 1, jx_hi = 2 * W + 10, jy_lo = 1, jy_hi = 2 * H + 10;
                        if (invertible) {
                            const double ux = (double)nx - cxo, uy = (double)ny - cyo;
                            const double jcx = i00 * ux + i01 * uy + (double)(W + 5), jcy = i10 * ux + i11 * uy + (double)(H + 5);
                            const double lx = floor(jcx - ex) - 1.0, hxx = ceil(jcx + ex) + 1.0;
                            const double ly = floor(jcy - ey) - 1.0, hyy = ceil(jcy + ey) + 1.0;
                            // (comparisons written so that a NaN or an out-of-range box leaves the full range)
                            if (lx > (double)jx_lo) jx_lo = lx < (double)(jx_hi + 1) ? (int)lx : jx_hi + 1;
                            if (hxx < (double)jx_hi) jx_hi = hxx > 0.0 ? (int)hxx : 0;
                            if (ly > (double)jy_lo) jy_lo = ly < (double)(jy_hi + 1) ? (int)ly : jy_hi + 1;
                            if (hyy < (double)jy_hi) jy_hi = hyy > 0.0 ? (int)hyy : 0;
                        }
                        for (int jy = jy_lo; jy <= jy_hi; jy++)
                            for (int jx = jx_lo; jx <= jx_hi; jx++) {
                                double hx, hy;
                                int sx0, sy0;
                                float frx, fry;
                                sample_pos(A, jx, jy, H, W, hx, hy);
                                if (!split_pos(hx, W, sx0, frx) || !split_pos(hy, H, sy0, fry)) continue;
                                const float wxx = sx0 == nx ? 1.0f - frx : (sx0 + 1 == nx ? frx : 0.0f);
                                const float wyy = sy0 == ny ? 1.0f - fry : (sy0 + 1 == ny ? fry : 0.0f);
                                const float wgt = wxx * wyy;
                                if (wgt == 0.0f) continue;
                                const float* g = gb + (int64_t)jy * SW + jx;
                                for (int c = 0; c < nc; c++) a[c] = fmaf_(wgt, g[c * splane], a[c]);
                            }
                    }
                    for (int c = 0; c < CC; c++) gu[c][wy][wx] = a[c];
                }
                __syncthreads();
                for (int e = threadIdx.x; e < CC * WIN * TILE; e += blockDim.x) {       // transposed up-filter along x
                    const int sp = e % TILE, wy = (e / TILE) % WIN, c = e / (TILE * WIN);
                    float t = 0.0f;
#pragma unroll
                    for (int k = 0; k < NT; k++) t = fmaf_(f2[k], gu[c][wy][2 * sp + k], t);
                    tmp[c][wy][sp] = t;
                }
                __syncthreads();
                if (py >= max(ylo, 0) && py <= min(yhi, H - 1) && px >= max(xlo, 0) && px <= min(xhi, W - 1)) {
                    const int spy = ry == 0 ? ty : TILE - 1 - ty, spx = rx == 0 ? tx : TILE - 1 - tx;
                    for (int c = 0; c < nc; c++) {
                        float t = 0.0f;
#pragma unroll
                        for (int k = 0; k < NT; k++) t = fmaf_(f2[k], tmp[c][2 * spy + k][spx], t);
                        acc[c] = acc[c] + t;
                    }
                }
                __syncthreads();
            }
        }
        if (py < H && px < W)
            for (int c = 0; c < nc; c++) dx[((int64_t)b * C + c0 + c) * plane + (int64_t)py * W + px] = acc[c];
    }
}

// ------------------------------------------------------------------------------------------------------------------------ colour
// y = mask * (M x[:ncc] + bias + sigma * noise); channels >= ncc take no matrix.  M = C[:3,:3] (transposed for the adjoint), bias = C[:3,3];
// one colour channel: the scalar forms of augment.py:376-378.
__global__ __launch_bounds__(256) void augment_color_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ Cm,
                                                            int transposed, int use_bias, const float* __restrict__ noise,
                                                            const float* __restrict__ sigma, const float* __restrict__ cutout, int B, int C, int H,
                                                            int W, int ncc) {
    const int64_t plane = (int64_t)H * W, total = (int64_t)B * plane;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(e / plane);
        const int64_t pix = e - (int64_t)b * plane;
        const int py = (int)(pix / W), px = (int)(pix - (int64_t)py * W);
        const float* xp = x + (int64_t)b * C * plane + pix;
        float* yp = y + (int64_t)b * C * plane + pix;
        float mask = 1.0f;
        if (cutout) {
            const float* ct = cutout + (int64_t)b * 4;
            const bool mx = fabsf(((float)px + 0.5f) / (float)W - ct[2]) >= ct[0] / 2.0f;
            const bool my = fabsf(((float)py + 0.5f) / (float)H - ct[3]) >= ct[1] / 2.0f;
            mask = (mx || my) ? 1.0f : 0.0f;
        }
        const float sg = noise ? sigma[b] : 0.0f;
        float v[3] = {0.0f, 0.0f, 0.0f};
        int c = 0;
        if (Cm && ncc == 3) {
            const float* M = Cm + (int64_t)b * 16;
            const float x0 = xp[0], x1 = xp[plane], x2 = xp[2 * plane];
            for (int r = 0; r < 3; r++) {
                const float m0 = transposed ? M[0 * 4 + r] : M[r * 4 + 0], m1 = transposed ? M[1 * 4 + r] : M[r * 4 + 1],
                            m2 = transposed ? M[2 * 4 + r] : M[r * 4 + 2];
                float t = (m0 * x0 + m1 * x1) + m2 * x2;
                if (use_bias) t = t + M[r * 4 + 3];
                v[r] = t;
            }
            c = 3;
        } else if (Cm && ncc == 1) {
            const float* M = Cm + (int64_t)b * 16;
            float col[4];
            for (int k = 0; k < 4; k++) col[k] = ((M[0 * 4 + k] + M[1 * 4 + k]) + M[2 * 4 + k]) / 3.0f;     // C[:, :3, :].mean(dim=1)
            float t = xp[0] * ((col[0] + col[1]) + col[2]);
            if (use_bias) t = t + col[3];
            v[0] = t;
            c = 1;
        }
        for (int k = 0; k < C; k++) {
            float t = k < c ? v[k] : xp[(int64_t)k * plane];
            if (noise) t = t + noise[(int64_t)b * C * plane + (int64_t)k * plane + pix] * sg;
            yp[(int64_t)k * plane] = t * mask;
        }
    }
}

}  // namespace

TDGP_API int tdgp_augment_params(const float* cfg, const float* p, int B, int H, int W, int num_channels, const float* uniforms,
                                 const float* normals, int use_percentile, float percentile, float* G_inv, float* Cmat, float* gains,
                                 float* noise_sigma, float* cutout, tdgp_stream_t stream) {
    TDGP_CHECK(cfg && p, TDGP_EINVAL, "augment_params: null pointer");
    TDGP_CHECK(B >= 1 && H >= 1 && W >= 1 && num_channels >= 1, TDGP_EINVAL, "augment_params: bad shape");
    TDGP_CHECK(use_percentile || (uniforms && normals), TDGP_EINVAL, "augment_params: draws needed without a percentile");
    AugCfg c;
    memcpy(&c, cfg, sizeof(c));
    TDGP_LAUNCH("augment_params_kernel", augment_params_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, c, p, B, H, W, num_channels,
                uniforms, normals, use_percentile ? 1 : 0, percentile, G_inv, Cmat, gains, noise_sigma, cutout);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

static int geom_shape_ok(int B, int C, int H, int W) {
    return B >= 1 && B <= 65535 && C >= 1 && H >= 2 && W >= 2 && H <= 8192 && W <= 8192 && (double)B * C * (2.0 * H + 12) * (2.0 * W + 12) < 2.0e18;
}

TDGP_API int tdgp_augment_geom(const float* x, const float* G_inv, const float* f, float* y, int B, int C, int H, int W, tdgp_stream_t stream) {
    TDGP_CHECK(x && G_inv && f && y, TDGP_EINVAL, "augment_geom: null pointer");
    TDGP_CHECK(geom_shape_ok(B, C, H, W), TDGP_EINVAL, "augment_geom: bad shape (2 <= H, W <= 8192, B <= 65535)");
    const int tx = cdiv(W, TILE), ty = cdiv(H, TILE);
    TDGP_LAUNCH("augment_geom_kernel", augment_geom_kernel, dim3(tx * ty, B), dim3(256), 0, (hipStream_t)stream, x, G_inv, f, y, B, C, H, W, tx);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_augment_geom_adj_workspace_bytes(int B, int C, int H, int W) {
    if (!geom_shape_ok(B, C, H, W)) return -1;
    return (int64_t)B * C * (2 * (int64_t)H + 12) * (2 * (int64_t)W + 12) * (int64_t)sizeof(float);
}

TDGP_API int tdgp_augment_geom_adj(const float* dy, const float* G_inv, const float* f, float* dx, int B, int C, int H, int W, void* workspace,
                                   int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(dy && G_inv && f && dx && workspace, TDGP_EINVAL, "augment_geom_adj: null pointer");
    TDGP_CHECK(geom_shape_ok(B, C, H, W), TDGP_EINVAL, "augment_geom_adj: bad shape (2 <= H, W <= 8192, B <= 65535)");
    TDGP_CHECK(workspace_bytes >= tdgp_augment_geom_adj_workspace_bytes(B, C, H, W), TDGP_EINVAL, "augment_geom_adj: workspace too small");
    TDGP_CHECK(((uintptr_t)workspace & 3) == 0, TDGP_EINVAL, "augment_geom_adj: workspace must be 4-byte aligned");
    float* gs = (float*)workspace;
    const int64_t total = (int64_t)B * C * (2 * (int64_t)H + 12) * (2 * (int64_t)W + 12);
    const int blocks = (int)min((int64_t)65536, cdiv64(total, 256));
    TDGP_LAUNCH("augment_down_adj_kernel", augment_down_adj_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, f, gs, (int64_t)B * C, H, W);
    TDGP_LAUNCH_CHECK();
    const int tx = cdiv(W, TILE), ty = cdiv(H, TILE);
    TDGP_LAUNCH("augment_geom_adj_kernel", augment_geom_adj_kernel, dim3(tx * ty, B), dim3(256), 0, (hipStream_t)stream, gs, G_inv, f, dx, B, C, H, W,
                tx);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_augment_color(const float* x, float* y, const float* Cmat, int transposed, int use_bias, const float* noise, const float* noise_sigma,
                                const float* cutout, int B, int C, int H, int W, int num_color_channels, tdgp_stream_t stream) {
    TDGP_CHECK(x && y, TDGP_EINVAL, "augment_color: null pointer");
    TDGP_CHECK(B >= 1 && C >= 1 && H >= 1 && W >= 1 && (double)B * C * H * W < 9.0e18 && (int64_t)H * W < ((int64_t)1 << 31), TDGP_EINVAL,
               "augment_color: bad shape");
    TDGP_CHECK(!Cmat || ((num_color_channels == 3 || num_color_channels == 1) && num_color_channels <= C), TDGP_EINVAL,
               "augment_color: image must be RGB (3 colour channels) or L (1 colour channel)");
    TDGP_CHECK(!noise || noise_sigma, TDGP_EINVAL, "augment_color: noise needs noise_sigma");
    const int64_t total = (int64_t)B * H * W;
    const int blocks = (int)min((int64_t)65536, cdiv64(total, 256));
    TDGP_LAUNCH("augment_color_kernel", augment_color_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, Cmat, transposed ? 1 : 0,
                use_bias ? 1 : 0, noise, noise_sigma, cutout, B, C, H, W, num_color_channels);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

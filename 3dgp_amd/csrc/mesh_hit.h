// mesh_hit.h -- what a hit of a mesh frame needs from its triangle, one body each: the triangle's frame, the face normal (tdgp_mesh_resolve),
// the interpolated vertex colour (tdgp_mesh_resolve), the interpolated vertex normal (tdgp_mesh_interp_normals) and the texture fetch
// (tdgp_mesh_sample_texture).  The one-sample kernels (mesh_raster.hip, mesh_surface.hip, mesh_texture.hip) and the fused multisample
// resolve (tdgp_mesh_resolve_ms, mesh_raster.hip) compile this text, so a sample is shaded with the bits a ray is.  The arithmetic is the
// one include/tdgp.h writes out under those entry points: double where stated, every operation rounded once in the order written.
#pragma once
#include "common.h"
#include "mesh_bary.h"

// v0 and the legs a = v1 - v0, b = v2 - v0 of the triangle with (checked) vertex indices idx, widened
__device__ __forceinline__ void mesh_tri_frame(const float* __restrict__ verts, const int (&idx)[3], double (&a)[3], double (&b)[3], double (&v0)[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        v0[c] = (double)verts[(int64_t)idx[0] * 3 + c];
        a[c] = (double)verts[(int64_t)idx[1] * 3 + c] - v0[c];
        b[c] = (double)verts[(int64_t)idx[2] * 3 + c] - v0[c];
    }
}

// the unit normal of the stored winding; a triangle of no (or unbounded) area faces the ray: tdgp_iso_shade's own fallback
__device__ __forceinline__ void mesh_face_normal(const double (&a)[3], const double (&b)[3], const float (&d)[3], float (&n)[3]) {
    const double g[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double gq = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    if (gq > 0.0 && gq < (double)__builtin_inff()) {
        const double r = sqrt(gq);
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = (float)(g[c] / r);
    } else {
        const float dn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = (-d[c]) / dn;
    }
}

// one value per vertex (rgb [V,3]) at the weights w of mesh_bary_weights
__device__ __forceinline__ void mesh_vertex_colour(const double (&w)[3], const int (&idx)[3], const float* __restrict__ vertex_rgb, float (&col)[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double c0 = (double)vertex_rgb[(int64_t)idx[0] * 3 + c], c1 = (double)vertex_rgb[(int64_t)idx[1] * 3 + c];
        const double c2 = (double)vertex_rgb[(int64_t)idx[2] * 3 + c];
        col[c] = (float)((w[0] * c0 + w[1] * c1) + w[2] * c2);
    }
}

// the vertex normals at the weights w, normalised -> false (n untouched: the face normal stays) when they cancel or overflow
__device__ __forceinline__ bool mesh_vertex_normal(const double (&w)[3], const int (&idx)[3], const float* __restrict__ vnormal, float (&n)[3]) {
    double m[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double n0 = (double)vnormal[(int64_t)idx[0] * 3 + c], n1 = (double)vnormal[(int64_t)idx[1] * 3 + c];
        const double n2 = (double)vnormal[(int64_t)idx[2] * 3 + c];
        m[c] = (w[0] * n0 + w[1] * n1) + w[2] * n2;
    }
    const double q = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    if (!(q > 0.0 && q < (double)__builtin_inff())) return false;
    const double r = sqrt(q);
#pragma unroll
    for (int c = 0; c < 3; c++) n[c] = (float)(m[c] / r);
    return true;
}

// a tile coordinate brought into [0, S - 1] before it is turned into an index (a NaN goes to 0)
__device__ __forceinline__ double tile_clamp(double x, double hi) {
    if (!(x >= 0.0)) x = 0.0;
    if (x > hi) x = hi;
    return x;
}

// the texture of triangle k (checked: 0 <= k < T) at the weights w: image uint8 [H,W,3], the atlas of n texels with r tiles per row
__device__ __forceinline__ void mesh_texture_fetch(const double (&w)[3], int k, const uint8_t* __restrict__ image, int n, int r, int W, int filter,
                                                   float (&out)[3]) {
    const int S = n + 2;
    const double m = (double)(n - 1), hi = (double)(S - 1);
    const double u = w[1] * m, v = w[2] * m;
    const bool upper = (k & 1) != 0;
    const double tx = tile_clamp(upper ? hi - u : u, hi), ty = tile_clamp(upper ? hi - v : v, hi);
    const int tile = k >> 1;
    const int trow = tile / r;
    const int64_t X0 = (int64_t)(tile - trow * r) * S, Y0 = (int64_t)trow * S;
    const uint8_t* base = image + (Y0 * W + X0) * 3;
    if (filter == 0) {
        const int x0 = (int)rint(tx), y0 = (int)rint(ty);
        const uint8_t* t00 = base + ((int64_t)y0 * W + x0) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = (float)((double)t00[c] / 255.0);
    } else {
        const double fx0 = floor(tx), fy0 = floor(ty);
        const double fx = tx - fx0, fy = ty - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int x1 = min(x0 + 1, S - 1), y1 = min(y0 + 1, S - 1);
        const double gx = 1.0 - fx, gy = 1.0 - fy;
        const double w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
        const uint8_t* t00 = base + ((int64_t)y0 * W + x0) * 3;
        const uint8_t* t10 = base + ((int64_t)y0 * W + x1) * 3;
        const uint8_t* t01 = base + ((int64_t)y1 * W + x0) * 3;
        const uint8_t* t11 = base + ((int64_t)y1 * W + x1) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++)
            out[c] = (float)(((w00 * (double)t00[c] + w10 * (double)t10[c]) + (w01 * (double)t01[c] + w11 * (double)t11[c])) / 255.0);
    }
}

// the layout of tdgp.h from (T, n): -> false when (r, W, H) are not the atlas of T triangles at n texels
inline bool atlas_is(int64_t T, int n, int r, int W, int H) {
    const int64_t S = n + 2, P = (T + 1) / 2;
    int64_t rr = 0;
    while (rr * rr < P) rr++;
    const int64_t rows = rr == 0 ? 0 : (P + rr - 1) / rr;
    return (int64_t)r == rr && (int64_t)W == rr * S && (int64_t)H == rows * S;
}

// mesh_bary.h -- the barycentric weights of a hit point on its triangle, shared by tdgp_mesh_resolve (vertex colours, mesh_raster.hip) and
// tdgp_mesh_interp_normals (vertex normals, mesh_surface.hip) so that both interpolate with the same bits.  The arithmetic is the one
// include/tdgp.h writes out under tdgp_mesh_resolve: double throughout, every operation rounded once in the order written.
#pragma once
#include "common.h"

// a = v1 - v0, b = v2 - v0, v0 and the hit x (fp32, widened by the caller) -> w[0..2], the weights of vertices 0, 1, 2
__device__ __forceinline__ void mesh_bary_weights(const double (&a)[3], const double (&b)[3], const double (&v0)[3], const float (&x)[3], double (&w)[3]) {
    const double e[3] = {(double)x[0] - v0[0], (double)x[1] - v0[1], (double)x[2] - v0[2]};
    const double d11 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], d12 = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const double d22 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double e1 = (e[0] * a[0] + e[1] * a[1]) + e[2] * a[2], e2 = (e[0] * b[0] + e[1] * b[1]) + e[2] * b[2];
    const double den = d11 * d22 - d12 * d12;
    double b1 = (d22 * e1 - d12 * e2) / den, b2 = (d11 * e2 - d12 * e1) / den;
    if (!(b1 >= 0.0)) b1 = 0.0;                                 // a NaN (a needle: den == 0) is taken to vertex 0
    if (!(b2 >= 0.0)) b2 = 0.0;
    const double sum = b1 + b2;
    if (sum > 1.0) { b1 = b1 / sum; b2 = b2 / sum; }
    w[0] = (1.0 - b1) - b2;
    w[1] = b1;
    w[2] = b2;
}

// shade.h -- the shade of a hit from its unit normal on, shared by the shape frames (iso_surface.hip: normal from the density stencil) and the
// mesh frames (mesh_raster.hip: face normal from the resolve pass).  Arithmetic contract (include/tdgp.h): every fp32
// operation rounded once in the order written, `/` and sqrtf correctly rounded, ordered comparisons (a NaN compares false).
#pragma once
#include "common.h"

namespace {

struct ShadeParams {
    int mode, has_light;                             // mode 0 shaded albedo, 1 normals, 2 colour; no light = a headlight along -d
    float light[3], ambient, albedo[3], background[3];
};

// `light` may be null (headlight); the entry points have checked mode and the other pointers
inline ShadeParams shade_params(int mode, const float* light, float ambient, const float* albedo, const float* background) {
    ShadeParams q;
    q.mode = mode; q.has_light = light ? 1 : 0; q.ambient = ambient;
    for (int c = 0; c < 3; c++) { q.light[c] = light ? light[c] : 0.0f; q.albedo[c] = albedo[c]; q.background[c] = background[c]; }
    return q;
}

__device__ __forceinline__ float ray_norm(const float (&d)[3]) { return sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); }

// out = the shade of a hit with unit normal n seen along d.  colour(c) is the kernel's own source of channel c of the mode-2 colour, asked
// in mode 2 only; it is clamped to [0, 1] here with a NaN taken to 0.
template <class Colour>
__device__ __forceinline__ void shade_hit(const ShadeParams q, const float (&n)[3], const float (&d)[3], Colour colour, float (&out)[3]) {
    const float dn = ray_norm(d);
    float l[3];
#pragma unroll
    for (int c = 0; c < 3; c++) l[c] = q.has_light ? q.light[c] : (-d[c]) / dn;
    float cs = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
    if (!(cs > 0.0f)) cs = 0.0f;
    const float v = q.ambient + (1.0f - q.ambient) * cs;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (q.mode == 0) {
            out[c] = (q.albedo[c] * v) * 2.0f - 1.0f;
        } else if (q.mode == 1) {
            out[c] = n[c];
        } else {
            float k = colour(c);
            k = !(k > 0.0f) ? 0.0f : k;
            k = k > 1.0f ? 1.0f : k;
            out[c] = (k * v) * 2.0f - 1.0f;
        }
    }
}

}  // namespace

// mesh_raster.hip -- mesh frames: the indexed mesh `geometry.marching_cubes` leaves on the device, seen from the cameras (mesh.py:
// render_mesh_views).  Marching-cubes triangles of a 256^3 grid seen at 256^2 are smaller than a pixel, so this is a visibility-buffer
// rasteriser with one triangle per lane, not a tiled one:
//   tdgp_mesh_visibility (per camera x triangle: 64-bit atomic min of (depth bits, triangle) per covered pixel)
//   -> tdgp_mesh_resolve (per ray: hit depth, face normal, colour, the 7 stencil points of tdgp_iso_locate) -> tdgp_mesh_shade.
// Arithmetic contract (include/tdgp.h): every fp operation rounded once in the order written (-ffp-contract=off), `/` and
// sqrt correctly rounded, ordered comparisons, coverage decided in exact int64 arithmetic on coordinates snapped to 1/256 pixel.  The
// only atomic is an unsigned 64-bit minimum, whose result does not depend on the order of its operands: the same bytes on every run and under
// every permutation of the triangles.  A numpy restatement reproduces all three bit for bit (tests/mesh_raster_reference.py).
#include "common.h"
#include "shade.h"
#include "mesh_bary.h"

namespace {

constexpr int SUB = 8;                               // sub-pixel bits of the snapped screen coordinates
constexpr double SUB_SCALE = 256.0;
constexpr double COORD_LIMIT = 1073741824.0;         // 2^30 sub-pixel units: beyond it a triangle is dropped (the int64 edge functions stay exact)
constexpr int WAVE_BBOX = 8;                         // a bbox wider or taller than this many pixels is rasterised by the whole wave

struct TriSetup {
    int X[3], Y[3];                                  // snapped screen coordinates, |.| <= 2^30
    double iz[3];                                    // 1 / depth of the vertices along the camera axis
    int64_t area;                                    // |twice the signed area| in sub-pixel units squared
    int sign, k, cam, c0, r0, bw, bh;                // orientation, triangle, camera, first column / row and size of the clamped bbox
};

__device__ __forceinline__ void raster_pixel(const TriSetup& s, int col, int row, const float* __restrict__ c2w, const float* __restrict__ ray_d, int h,
                                             int w, unsigned long long* __restrict__ vis) {
    const int64_t px = (int64_t)col << SUB, py = (int64_t)row << SUB;
    int64_t e[3];
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {                    // edge i runs from vertex i+1 to vertex i+2, opposite vertex i
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        const int64_t dx = (int64_t)s.sign * ((int64_t)s.X[b] - s.X[a]), dy = (int64_t)s.sign * ((int64_t)s.Y[b] - s.Y[a]);
        e[i] = dx * (py - s.Y[a]) - dy * (px - s.X[a]);
        const bool top_left = dy < 0 || (dy == 0 && dx > 0);
        in = in && (e[i] > 0 || (e[i] == 0 && top_left));
    }
    if (!in) return;
    const double q = ((double)e[0] * s.iz[0] + (double)e[1] * s.iz[1]) + (double)e[2] * s.iz[2];
    const double depth = (double)s.area / q;
    const int64_t ray = ((int64_t)s.cam * h + row) * w + col;
    const float* m = c2w + (int64_t)s.cam * 16;
    const float* d = ray_d + ray * 3;
    const double df = ((double)d[0] * (double)(-m[2]) + (double)d[1] * (double)(-m[6])) + (double)d[2] * (double)(-m[10]);
    const float t = (float)(depth / df);
    if (!(t > 0.0f && t < __builtin_inff())) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)(uint32_t)s.k;
    atomicMin(vis + ray, key);
}

__global__ __launch_bounds__(256) void mesh_visibility_kernel(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t T,
                                                              const float* __restrict__ c2w, const float* __restrict__ focal,
                                                              const float* __restrict__ ray_d, int C, int h, int w, float near_, int cull,
                                                              unsigned long long* __restrict__ vis) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    TriSetup s;
    bool live = gid < (int64_t)C * T;
    s.cam = live ? (int)(gid / T) : 0;
    s.k = live ? (int)(gid - (int64_t)s.cam * T) : 0;
    s.sign = 0; s.area = 0; s.c0 = s.r0 = 0; s.bw = s.bh = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) { s.X[i] = s.Y[i] = 0; s.iz[i] = 0.0; }
    if (live) {
        int idx[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            idx[i] = triangles[(int64_t)s.k * 3 + i];
            live = live && idx[i] >= 0 && (int64_t)idx[i] < V;
        }
        if (live) {
            const float* m = c2w + (int64_t)s.cam * 16;
            const double fc = (double)focal[s.cam], near_d = (double)near_;
            const double hw = (double)(w - 1) * 0.5, hh = (double)(h - 1) * 0.5;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float* v = vertices + (int64_t)idx[i] * 3;
                const double p0 = (double)v[0] - (double)m[3], p1 = (double)v[1] - (double)m[7], p2 = (double)v[2] - (double)m[11];
                const double xc = (p0 * (double)m[0] + p1 * (double)m[4]) + p2 * (double)m[8];
                const double yc = (p0 * (double)m[1] + p1 * (double)m[5]) + p2 * (double)m[9];
                const double zc = (p0 * (double)(-m[2]) + p1 * (double)(-m[6])) + p2 * (double)(-m[10]);
                if (!(zc >= near_d)) { live = false; continue; }
                const double fx = ((((xc * fc) / zc) + 1.0) * hw) * SUB_SCALE;
                const double fy = ((1.0 - ((yc * fc) / zc)) * hh) * SUB_SCALE;
                if (!(fabs(fx) < COORD_LIMIT && fabs(fy) < COORD_LIMIT)) { live = false; continue; }
                s.X[i] = (int)rint(fx);
                s.Y[i] = (int)rint(fy);
                s.iz[i] = 1.0 / zc;
            }
        }
        if (live) {
            const int64_t area2 = ((int64_t)s.X[1] - s.X[0]) * ((int64_t)s.Y[2] - s.Y[0]) - ((int64_t)s.Y[1] - s.Y[0]) * ((int64_t)s.X[2] - s.X[0]);
            // the screen's y points down: a triangle whose stored winding is counter-clockwise as the camera sees it (its normal faces the camera) has area2 < 0
            if (area2 == 0 || (cull == 1 && area2 > 0) || (cull == 2 && area2 < 0)) live = false;
            s.sign = area2 < 0 ? -1 : 1;
            s.area = area2 < 0 ? -area2 : area2;
            const int xmin = min(s.X[0], min(s.X[1], s.X[2])), xmax = max(s.X[0], max(s.X[1], s.X[2]));
            const int ymin = min(s.Y[0], min(s.Y[1], s.Y[2])), ymax = max(s.Y[0], max(s.Y[1], s.Y[2]));
            const int c0 = max(0, (int)(((int64_t)xmin + ((1 << SUB) - 1)) >> SUB)), c1 = min(w - 1, xmax >> SUB);
            const int r0 = max(0, (int)(((int64_t)ymin + ((1 << SUB) - 1)) >> SUB)), r1 = min(h - 1, ymax >> SUB);
            if (c0 > c1 || r0 > r1) live = false;
            s.c0 = c0; s.r0 = r0; s.bw = c1 - c0 + 1; s.bh = r1 - r0 + 1;
        }
    }
    const bool big = live && (s.bw > WAVE_BBOX || s.bh > WAVE_BBOX);
    if (live && !big) {
        for (int r = 0; r < s.bh; r++)
            for (int c = 0; c < s.bw; c++) raster_pixel(s, s.c0 + c, s.r0 + r, c2w, ray_d, h, w, vis);
    }
    // hand-over: every lane of the wave reaches this loop; triangles with a large bbox are taken one at a time, 64 pixels of the bbox per step
    unsigned long long mask = __ballot(big);
    const int lane = lane_id();
    while (mask) {
        const int src = __ffsll(mask) - 1;
        mask &= mask - 1;
        TriSetup b;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            b.X[i] = __shfl(s.X[i], src, 64);
            b.Y[i] = __shfl(s.Y[i], src, 64);
            b.iz[i] = shfl_f64(s.iz[i], src);
        }
        b.area = (int64_t)(((uint64_t)(uint32_t)__shfl((int)(s.area >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(s.area & 0xffffffff), src, 64));
        b.sign = __shfl(s.sign, src, 64);
        b.k = __shfl(s.k, src, 64);
        b.cam = __shfl(s.cam, src, 64);
        b.c0 = __shfl(s.c0, src, 64);
        b.r0 = __shfl(s.r0, src, 64);
        b.bw = __shfl(s.bw, src, 64);
        b.bh = __shfl(s.bh, src, 64);
        const int n = b.bw * b.bh;                                     // <= h * w < 2^28
        for (int i = lane; i < n; i += 64) {
            const int r = i / b.bw;
            raster_pixel(b, b.c0 + (i - r * b.bw), b.r0 + r, c2w, ray_d, h, w, vis);
        }
    }
}

__global__ __launch_bounds__(256) void mesh_resolve_kernel(const unsigned long long* __restrict__ vis, const float* __restrict__ vertices, int64_t V,
                                                           const int32_t* __restrict__ triangles, int64_t T, const float* __restrict__ ray_o,
                                                           const float* __restrict__ ray_d, int64_t rays, float step, float t_miss,
                                                           const float* __restrict__ vertex_rgb, float* __restrict__ t_hit, int32_t* __restrict__ status,
                                                           int32_t* __restrict__ tri, float* __restrict__ normal, float* __restrict__ colour,
                                                           float* __restrict__ points) {
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= rays) return;
    const unsigned long long key = vis[ray];
    const float o[3] = {ray_o[ray * 3 + 0], ray_o[ray * 3 + 1], ray_o[ray * 3 + 2]};
    const float d[3] = {ray_d[ray * 3 + 0], ray_d[ray * 3 + 1], ray_d[ray * 3 + 2]};
    int k = (int)(uint32_t)(key & 0xffffffffull);
    bool hit = key != ~0ull && k >= 0 && (int64_t)k < T;
    int idx[3] = {0, 0, 0};
    if (hit) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            idx[i] = triangles[(int64_t)k * 3 + i];
            hit = hit && idx[i] >= 0 && (int64_t)idx[i] < V;       // a key that names a bad triangle (never written by tdgp_mesh_visibility) is a miss
        }
    }
    const float th = hit ? __uint_as_float((uint32_t)(key >> 32)) : t_miss;
    float n[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f}, x[3];
#pragma unroll
    for (int c = 0; c < 3; c++) x[c] = o[c] + d[c] * th;
    if (hit) {
        double a[3], b[3], v0[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v0[c] = (double)vertices[(int64_t)idx[0] * 3 + c];
            a[c] = (double)vertices[(int64_t)idx[1] * 3 + c] - v0[c];
            b[c] = (double)vertices[(int64_t)idx[2] * 3 + c] - v0[c];
        }
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
        if (colour) {
            double bw[3];
            mesh_bary_weights(a, b, v0, x, bw);                         // shared with tdgp_mesh_interp_normals (mesh_bary.h)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double c0 = (double)vertex_rgb[(int64_t)idx[0] * 3 + c], c1 = (double)vertex_rgb[(int64_t)idx[1] * 3 + c];
                const double c2 = (double)vertex_rgb[(int64_t)idx[2] * 3 + c];
                col[c] = (float)((bw[0] * c0 + bw[1] * c1) + bw[2] * c2);
            }
        }
    }
    t_hit[ray] = th;
    status[ray] = hit ? 1 : 0;
    tri[ray] = hit ? k : -1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        normal[ray * 3 + c] = n[c];
        if (colour) colour[ray * 3 + c] = col[c];
    }
#pragma unroll
    for (int p = 0; p < 21; p++) {
        const int m = p / 3, c = p - 3 * m;
        float y = x[c];
        if (m >= 1 && ((m - 1) >> 1) == c) y = (m & 1) ? y + step : y - step;
        points[ray * 21 + p] = y;
    }
}

// ShadeParams under the name the kernel's symbol has carried since the first mesh frames
struct MeshShadeParams : ShadeParams {};

__global__ __launch_bounds__(256) void mesh_shade_kernel(const float* __restrict__ normal, const int32_t* __restrict__ status, const float* __restrict__ ray_d,
                                                         const float* __restrict__ colour, int64_t rays, MeshShadeParams q, float* __restrict__ rgb) {
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= rays) return;
    float out[3];
    if (status[ray] == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = q.background[c];
    } else {
        const float d[3] = {ray_d[ray * 3 + 0], ray_d[ray * 3 + 1], ray_d[ray * 3 + 2]};
        const float n[3] = {normal[ray * 3 + 0], normal[ray * 3 + 1], normal[ray * 3 + 2]};
        // the colour is already in [0, 1] (mesh.vertex_colours); it may be null outside mode 2
        shade_hit(q, n, d, [&](int c) { return colour[ray * 3 + c]; }, out);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[ray * 3 + c] = out[c];
}

const int64_t MESH_RAYS_MAX = (int64_t)1 << 30;       // C * h * w
const int64_t MESH_WORK_MAX = (int64_t)1 << 38;       // C * T: one lane each, 256 per block, a valid grid

}  // namespace

TDGP_API int tdgp_mesh_visibility(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* c2w, const float* focal,
                                  const float* ray_d, int C, int h, int w, float near_, int cull, uint64_t* vis, tdgp_stream_t stream) {
    TDGP_CHECK(c2w && focal && ray_d && vis, TDGP_EINVAL, "mesh_visibility: null pointer");
    TDGP_CHECK((vertices || V == 0) && (triangles || T == 0), TDGP_EINVAL, "mesh_visibility: null mesh pointer");
    TDGP_CHECK(V >= 0 && V <= 2147483647ll && T >= 0 && T <= 2147483647ll, TDGP_EINVAL, "mesh_visibility: V and T must lie in [0, 2^31 - 1]");
    TDGP_CHECK(C >= 0 && h >= 2 && w >= 2 && h <= 16384 && w <= 16384, TDGP_EINVAL, "mesh_visibility: need C >= 0 and 2 <= h, w <= 16384 (got C=%d, h=%d, w=%d)", C, h, w);
    TDGP_CHECK((int64_t)C * h * w <= MESH_RAYS_MAX && (int64_t)C * T <= MESH_WORK_MAX, TDGP_EINVAL, "mesh_visibility: too many rays or camera x triangle pairs for one call");
    TDGP_CHECK(near_ > 0.0f && near_ < __builtin_inff(), TDGP_EINVAL, "mesh_visibility: near must be positive and finite");
    TDGP_CHECK(cull >= 0 && cull <= 2, TDGP_EINVAL, "mesh_visibility: cull must be 0 (none), 1 (back) or 2 (front), got %d", cull);
    if (C == 0) return TDGP_OK;
    const int64_t rays = (int64_t)C * h * w;
    if (hipMemsetAsync(vis, 0xff, (size_t)rays * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) {
        tdgp_set_error("mesh_visibility: clearing the visibility buffer failed");
        return TDGP_ELAUNCH;
    }
    if (T == 0) return TDGP_OK;
    TDGP_LAUNCH("mesh_visibility_kernel", mesh_visibility_kernel, dim3((unsigned)cdiv64((int64_t)C * T, 256)), dim3(256), 0, (hipStream_t)stream, vertices, V,
                triangles, T, c2w, focal, ray_d, C, h, w, near_, cull, (unsigned long long*)vis);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_resolve(const uint64_t* vis, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* ray_o,
                               const float* ray_d, int64_t rays, float step, float t_miss, const float* vertex_rgb, float* t_hit, int32_t* status,
                               int32_t* tri, float* normal, float* colour, float* points, tdgp_stream_t stream) {
    TDGP_CHECK(vis && ray_o && ray_d && t_hit && status && tri && normal && points, TDGP_EINVAL, "mesh_resolve: null pointer");
    TDGP_CHECK((vertices || V == 0) && (triangles || T == 0), TDGP_EINVAL, "mesh_resolve: null mesh pointer");
    TDGP_CHECK((vertex_rgb == nullptr) == (colour == nullptr), TDGP_EINVAL, "mesh_resolve: vertex_rgb and colour come together");
    TDGP_CHECK(V >= 0 && V <= 2147483647ll && T >= 0 && T <= 2147483647ll, TDGP_EINVAL, "mesh_resolve: V and T must lie in [0, 2^31 - 1]");
    TDGP_CHECK(rays >= 0 && rays <= MESH_RAYS_MAX, TDGP_EINVAL, "mesh_resolve: bad ray count");
    if (rays == 0) return TDGP_OK;
    TDGP_LAUNCH("mesh_resolve_kernel", mesh_resolve_kernel, dim3((unsigned)cdiv64(rays, 256)), dim3(256), 0, (hipStream_t)stream,
                (const unsigned long long*)vis, vertices, V, triangles, T, ray_o, ray_d, rays, step, t_miss, vertex_rgb, t_hit, status, tri, normal, colour, points);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_shade(const float* normal, const int32_t* status, const float* ray_d, const float* colour, int64_t rays, int mode, const float* light,
                             float ambient, const float* albedo, const float* background, float* rgb, tdgp_stream_t stream) {
    TDGP_CHECK(normal && status && ray_d && albedo && background && rgb, TDGP_EINVAL, "mesh_shade: null pointer");
    TDGP_CHECK(rays >= 0 && rays <= MESH_RAYS_MAX, TDGP_EINVAL, "mesh_shade: bad shape");
    TDGP_CHECK(mode >= 0 && mode <= 2, TDGP_EINVAL, "mesh_shade: mode must be 0 (shaded), 1 (normals) or 2 (colour), got %d", mode);
    TDGP_CHECK(mode != 2 || colour, TDGP_EINVAL, "mesh_shade: mode 2 (colour) needs the colour tdgp_mesh_resolve wrote");
    if (rays == 0) return TDGP_OK;
    const MeshShadeParams q{shade_params(mode, light, ambient, albedo, background)};
    TDGP_LAUNCH("mesh_shade_kernel", mesh_shade_kernel, dim3((unsigned)cdiv64(rays, 256)), dim3(256), 0, (hipStream_t)stream, normal, status, ray_d, colour, rays, q, rgb);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

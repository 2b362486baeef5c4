// mesh_raster.hip -- mesh frames: the indexed mesh `geometry.marching_cubes` leaves on the device, seen from the cameras (mesh.py:
// render_mesh_views).  Marching-cubes triangles of a 256^3 grid seen at 256^2 are smaller than a pixel, so this is a visibility-buffer
// rasteriser with one triangle per lane, not a tiled one:
//   tdgp_mesh_visibility (per camera x triangle: 64-bit atomic min of (depth bits, triangle) per covered pixel)
//   -> tdgp_mesh_resolve (per ray: hit depth, face normal, colour, the 7 stencil points of tdgp_iso_locate) -> tdgp_mesh_shade.
// Arithmetic contract (include/tdgp.h): every fp operation rounded once in the order written (-ffp-contract=off), `/` and
// sqrt correctly rounded, ordered comparisons, coverage decided in exact int64 arithmetic on coordinates snapped to 1/256 pixel.  The
// only atomic is an unsigned 64-bit minimum, whose result does not depend on the order of its operands: the same bytes on every run and under
// every permutation of the triangles.  A numpy restatement reproduces all three bit for bit (tests/mesh_raster_reference.py).
// Multisampled frames: tdgp_mesh_visibility_ms (the same setup once per triangle, one key per covered sample of the 4- or
// 16-sample pattern, the sample's ray from its position) -> tdgp_mesh_resolve_ms (per sample: resolve, normal, colour and shade with the
// per-hit bodies of mesh_hit.h / shade.h that the one-sample kernels compile too; per pixel: mean colour, coverage, nearest hit).  Same
// contract, restated in tests/mesh_msaa_reference.py.
#include "common.h"
#include "shade.h"
#include "mesh_hit.h"

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

// The candidate positions of a triangle with screen box [xmin, xmax] x [ymin, ymax], as a box of lattice indices clamped to the frame.
//   S = 1:  the pixel centres, (256 c, 256 r).
//   S = 16: the samples of all pixels form one regular lattice, (64 c - 96, 64 r - 96) with c in [0, 4w), r in [0, 4h).
//   S = 4:  lattice row r in [0, 4h) holds sample r % 4 of pixel row r / 4, at y = 64 r - 96 and x = 256 c + ox(r % 4), c in [0, w): the columns
//           are those of the pixels with any sample position in the box.
template <int S>
__device__ __forceinline__ void sample_box(int xmin, int xmax, int ymin, int ymax, int h, int w, int& c0, int& c1, int& r0, int& r1) {
    if constexpr (S == 1) {
        c0 = max(0, (int)(((int64_t)xmin + ((1 << SUB) - 1)) >> SUB)); c1 = min(w - 1, xmax >> SUB);
        r0 = max(0, (int)(((int64_t)ymin + ((1 << SUB) - 1)) >> SUB)); r1 = min(h - 1, ymax >> SUB);
    } else {
        r0 = max(0, (int)(((int64_t)ymin + 96 + 63) >> 6)); r1 = min(4 * h - 1, (int)(((int64_t)ymax + 96) >> 6));
        if constexpr (S == 16) {
            c0 = max(0, (int)(((int64_t)xmin + 96 + 63) >> 6)); c1 = min(4 * w - 1, (int)(((int64_t)xmax + 96) >> 6));
        } else {
            c0 = max(0, (int)(((int64_t)xmin - 96 + 255) >> SUB)); c1 = min(w - 1, (int)(((int64_t)xmax + 96) >> SUB));
        }
    }
}

// (camera, triangle) number gid -> its setup; false when there is nothing to draw.  S: the sample pattern whose candidate box is kept (1: the
// pixel centres).
template <int S>
__device__ __forceinline__ bool tri_setup(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t T,
                                          const float* __restrict__ c2w, const float* __restrict__ focal, int C, int h, int w, float near_, int cull, int64_t gid,
                                          TriSetup& s) {
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
            int c0, c1, r0, r1;
            sample_box<S>(xmin, xmax, ymin, ymax, h, w, c0, c1, r0, r1);
            if (c0 > c1 || r0 > r1) live = false;
            s.c0 = c0; s.r0 = r0; s.bw = c1 - c0 + 1; s.bh = r1 - r0 + 1;
        }
    }
    return live;
}

// the setup of lane src, in every lane of the wave
__device__ __forceinline__ TriSetup tri_broadcast(const TriSetup& s, int src) {
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
    return b;
}

// the three edge functions at the position (px, py), in sub-pixel units; edge i runs from vertex i+1 to vertex i+2, opposite vertex i
struct Edges {
    int64_t dx[3], dy[3], e[3];
};

__device__ __forceinline__ Edges edges_at(const TriSetup& s, int64_t px, int64_t py) {
    Edges g;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        g.dx[i] = (int64_t)s.sign * ((int64_t)s.X[b] - s.X[a]);
        g.dy[i] = (int64_t)s.sign * ((int64_t)s.Y[b] - s.Y[a]);
        g.e[i] = g.dx[i] * (py - s.Y[a]) - g.dy[i] * (px - s.X[a]);
    }
    return g;
}

// the top-left rule on edge values e of the edges g: a position on an edge shared by two triangles belongs to exactly one of them
__device__ __forceinline__ bool edges_cover(const Edges& g, const int64_t (&e)[3]) {
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const bool top_left = g.dy[i] < 0 || (g.dy[i] == 0 && g.dx[i] > 0);
        in = in && (e[i] > 0 || (e[i] == 0 && top_left));
    }
    return in;
}

// the perspective-correct camera depth where the edge functions are e
__device__ __forceinline__ double edges_depth(const TriSetup& s, const int64_t (&e)[3]) {
    const double q = ((double)e[0] * s.iz[0] + (double)e[1] * s.iz[1]) + (double)e[2] * s.iz[2];
    return (double)s.area / q;
}

__device__ __forceinline__ unsigned long long vis_key(float t, int k) {
    return ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)(uint32_t)k;
}

__device__ __forceinline__ void raster_pixel(const TriSetup& s, int col, int row, const float* __restrict__ c2w, const float* __restrict__ ray_d, int h,
                                             int w, unsigned long long* __restrict__ vis) {
    const Edges g = edges_at(s, (int64_t)col << SUB, (int64_t)row << SUB);
    if (!edges_cover(g, g.e)) return;
    const double depth = edges_depth(s, g.e);
    const int64_t ray = ((int64_t)s.cam * h + row) * w + col;
    const float* m = c2w + (int64_t)s.cam * 16;
    const float* d = ray_d + ray * 3;
    const double df = ((double)d[0] * (double)(-m[2]) + (double)d[1] * (double)(-m[6])) + (double)d[2] * (double)(-m[10]);
    const float t = (float)(depth / df);
    if (!(t > 0.0f && t < __builtin_inff())) return;
    atomicMin(vis + ray, vis_key(t, s.k));
}

__global__ __launch_bounds__(256) void mesh_visibility_kernel(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t T,
                                                              const float* __restrict__ c2w, const float* __restrict__ focal,
                                                              const float* __restrict__ ray_d, int C, int h, int w, float near_, int cull,
                                                              unsigned long long* __restrict__ vis) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    TriSetup s;
    const bool live = tri_setup<1>(vertices, V, triangles, T, c2w, focal, C, h, w, near_, cull, gid, s);
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
        const TriSetup b = tri_broadcast(s, src);
        const int n = b.bw * b.bh;                                     // <= h * w < 2^28
        for (int i = lane; i < n; i += 64) {
            const int r = i / b.bw;
            raster_pixel(b, b.c0 + (i - r * b.bw), b.r0 + r, c2w, ray_d, h, w, vis);
        }
    }
}

// ---- multisampled coverage ----------------------------------------------------------------------------------------------------------------
// Sample j of a pixel sits at its centre + (ox, oy) sub-pixel units, x to the right and y down.  4: a rotated grid; 16: the 4 x 4 grid, row-major.
template <int S> __device__ __forceinline__ int ms_ox(int j) { return S == 16 ? -96 + 64 * (j & 3) : (j == 0 ? -32 : j == 1 ? 96 : j == 2 ? -96 : 32); }
template <int S> __device__ __forceinline__ int ms_oy(int j) { return S == 16 ? -96 + 64 * (j >> 2) : -96 + 64 * j; }

// The ray through the screen position (sx, sy), in the camera's frame: (u, v, 1) / len along right / up / forward -- the projection of
// tri_setup inverted.  A point at camera depth z on it has the ray parameter z * len.
__device__ __forceinline__ void ms_sample_ray(int sx, int sy, int h, int w, double fc, double& u, double& v, double& len) {
    const double hw = (double)(w - 1) * 0.5, hh = (double)(h - 1) * 0.5;
    u = ((double)sx / (SUB_SCALE * hw) - 1.0) / fc;
    v = (1.0 - (double)sy / (SUB_SCALE * hh)) / fc;
    len = sqrt((u * u + v * v) + 1.0);
}

// the candidate (c, r) of sample_box<S>: which sample of which pixel it is and where it sits
struct Candidate {
    int row, col, j, sx, sy;
};

template <int S>
__device__ __forceinline__ Candidate candidate_at(int c, int r) {
    Candidate p;
    const int q = r & 3;
    p.row = r >> 2;
    p.col = S == 16 ? c >> 2 : c;
    p.j = S == 16 ? q * 4 + (c & 3) : q;
    p.sx = (p.col << SUB) + ms_ox<S>(p.j);
    p.sy = (p.row << SUB) + ms_oy<S>(p.j);
    return p;
}

// the triangle's key at a candidate it covers (g: its edge functions there)
template <int S>
__device__ __forceinline__ void emit_sample(const TriSetup& s, const Candidate& p, const Edges& g, double fc, int h, int w, unsigned long long* __restrict__ vis) {
    const double depth = edges_depth(s, g.e);
    double u, v, len;
    ms_sample_ray(p.sx, p.sy, h, w, fc, u, v, len);
    const float t = (float)(depth * len);
    if (!(t > 0.0f && t < __builtin_inff())) return;
    atomicMin(vis + (((int64_t)s.cam * h + p.row) * w + p.col) * S + p.j, vis_key(t, s.k));
}

template <int S>
__device__ __forceinline__ void raster_sample(const TriSetup& s, int c, int r, double fc, int h, int w, unsigned long long* __restrict__ vis) {
    const Candidate p = candidate_at<S>(c, r);
    const Edges g = edges_at(s, p.sx, p.sy);
    if (edges_cover(g, g.e)) emit_sample<S>(s, p, g, fc, h, w, vis);
}

template <int S>
__global__ __launch_bounds__(256) void mesh_visibility_ms_kernel(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t T,
                                                                 const float* __restrict__ c2w, const float* __restrict__ focal, int C, int h, int w,
                                                                 float near_, int cull, unsigned long long* __restrict__ vis) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    TriSetup s;
    const bool live = tri_setup<S>(vertices, V, triangles, T, c2w, focal, C, h, w, near_, cull, gid, s);
    const bool big = live && (s.bw > WAVE_BBOX || s.bh > WAVE_BBOX);     // in candidates: the work a lane keeps is that of mesh_visibility_kernel
    if (live && !big) {
        // The integer cover tests first, the covered candidates of the box (at most 8 x 8) as a bit mask; then the double arithmetic of a key
        // for the set bits alone: the lanes of a wave diverge on coverage, and a wave pays for the longest list, not for the largest box.
        unsigned long long covered = 0;
        for (int r = 0; r < s.bh; r++)
            for (int c = 0; c < s.bw; c++) {
                const Candidate p = candidate_at<S>(s.c0 + c, s.r0 + r);
                const Edges g = edges_at(s, p.sx, p.sy);
                if (edges_cover(g, g.e)) covered |= 1ull << (r * s.bw + c);
            }
        const double fc = (double)focal[s.cam];
        while (covered) {
            const int i = __ffsll(covered) - 1;
            covered &= covered - 1;
            const int r = i / s.bw;
            const Candidate p = candidate_at<S>(s.c0 + (i - r * s.bw), s.r0 + r);
            emit_sample<S>(s, p, edges_at(s, p.sx, p.sy), fc, h, w, vis);
        }
    }
    unsigned long long mask = __ballot(big);         // the hand-over of mesh_visibility_kernel, 64 candidates of the box per step
    const int lane = lane_id();
    while (mask) {
        const int src = __ffsll(mask) - 1;
        mask &= mask - 1;
        const TriSetup b = tri_broadcast(s, src);
        const double fc = (double)focal[b.cam];
        const int n = b.bw * b.bh;                   // <= 16 * h * w <= 2^30 (checked by the entry point)
        for (int i = lane; i < n; i += 64) {
            const int r = i / b.bw;
            raster_sample<S>(b, b.c0 + (i - r * b.bw), b.r0 + r, fc, h, w, vis);
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
        mesh_tri_frame(vertices, idx, a, b, v0);                        // the per-hit bodies are shared with tdgp_mesh_resolve_ms (mesh_hit.h)
        mesh_face_normal(a, b, d, n);
        if (colour) {
            double bw[3];
            mesh_bary_weights(a, b, v0, x, bw);                         // shared with tdgp_mesh_interp_normals (mesh_bary.h)
            mesh_vertex_colour(bw, idx, vertex_rgb, col);
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

// What the fused resolve reads besides the keys: the optional per-vertex normals and colours, the optional texture and its atlas
struct MeshSurface {
    const float* vertex_normal;                      // [V,3] or null: face normals
    const float* vertex_rgb;                         // [V,3] or null
    const uint8_t* image;                            // [H,W,3] or null; mode 2 reads exactly one of vertex_rgb and image
    int n, r, W, filter;
};

// One lane per sample, the S samples of a pixel in S neighbouring lanes of one wave: every lane resolves and shades its own key, then the
// pixel's lanes add the S colours in sample order and agree on the nearest hit.  There are no per-sample buffers.
template <int S>
__global__ __launch_bounds__(256) void mesh_resolve_ms_kernel(const unsigned long long* __restrict__ vis, const float* __restrict__ vertices, int64_t V,
                                                              const int32_t* __restrict__ triangles, int64_t T, const float* __restrict__ c2w,
                                                              const float* __restrict__ focal, int64_t pixels, int h, int w, float t_miss, MeshSurface f,
                                                              MeshShadeParams q, float* __restrict__ rgb, float* __restrict__ coverage,
                                                              int32_t* __restrict__ status, float* __restrict__ depth, int32_t* __restrict__ tri,
                                                              float* __restrict__ normal) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t pixel = gid / S;
    const int j = (int)(gid - pixel * S);
    const bool live = pixel < pixels;                // 256 is a multiple of S: the lanes of a pixel are live together
    const unsigned long long key = live ? vis[gid] : ~0ull;
    const int k = (int)(uint32_t)(key & 0xffffffffull);
    bool hit = key != ~0ull && k >= 0 && (int64_t)k < T;
    int idx[3] = {0, 0, 0};
    if (hit) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            idx[i] = triangles[(int64_t)k * 3 + i];
            hit = hit && idx[i] >= 0 && (int64_t)idx[i] < V;       // a key that names a bad triangle (never written by tdgp_mesh_visibility_ms) is a miss
        }
    }
    const float th = hit ? __uint_as_float((uint32_t)(key >> 32)) : t_miss;
    float n[3] = {0.0f, 0.0f, 0.0f}, out[3] = {q.background[0], q.background[1], q.background[2]};
    if (hit) {
        const int R = h * w;
        const int cam = (int)(pixel / R);
        const int p = (int)(pixel - (int64_t)cam * R);
        const int row = p / w, col = p - row * w;
        const float* m = c2w + (int64_t)cam * 16;
        double u, v, len;
        ms_sample_ray((col << SUB) + ms_ox<S>(j), (row << SUB) + ms_oy<S>(j), h, w, (double)focal[cam], u, v, len);
        float d[3], x[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            d[c] = (float)(((u * (double)m[c * 4 + 0] + v * (double)m[c * 4 + 1]) + (double)(-m[c * 4 + 2])) / len);
            x[c] = m[c * 4 + 3] + d[c] * th;
        }
        double a[3], b[3], v0[3], bw[3];
        mesh_tri_frame(vertices, idx, a, b, v0);
        mesh_face_normal(a, b, d, n);
        float col3[3] = {0.0f, 0.0f, 0.0f};
        if (f.vertex_normal || q.mode == 2) {
            mesh_bary_weights(a, b, v0, x, bw);
            if (f.vertex_normal) mesh_vertex_normal(bw, idx, f.vertex_normal, n);
            if (q.mode == 2) {
                if (f.vertex_rgb) mesh_vertex_colour(bw, idx, f.vertex_rgb, col3);
                else mesh_texture_fetch(bw, k, f.image, f.n, f.r, f.W, f.filter, col3);
            }
        }
        shade_hit(q, n, d, [&](int c) { return col3[c]; }, out);
    }
    // the pixel's S lanes, in sample order
    const int base = lane_id() & ~(S - 1);
    double sum[3] = {0.0, 0.0, 0.0};
    int hits = 0, best = -1;
    float best_t = 0.0f;
#pragma unroll
    for (int i = 0; i < S; i++) {
#pragma unroll
        for (int c = 0; c < 3; c++) sum[c] = sum[c] + (double)__shfl(out[c], base + i, 64);
        const int hi = __shfl(hit ? 1 : 0, base + i, 64);
        const float ti = __shfl(th, base + i, 64);
        if (hi && (best < 0 || ti < best_t)) { best = i; best_t = ti; }
        hits += hi;
    }
    if (!live) return;
    if (j == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) rgb[pixel * 3 + c] = (float)(sum[c] / (double)S);
        coverage[pixel] = (float)hits / (float)S;
        status[pixel] = hits > 0 ? 1 : 0;
    }
    if (j == (best < 0 ? 0 : best)) {                // the nearest hit writes its own depth, triangle and normal; sample 0 writes a miss
        depth[pixel] = th;
        tri[pixel] = hit ? k : -1;
#pragma unroll
        for (int c = 0; c < 3; c++) normal[pixel * 3 + c] = n[c];
    }
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

TDGP_API int tdgp_mesh_visibility_ms(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* c2w, const float* focal, int C,
                                     int h, int w, int samples, float near_, int cull, uint64_t* vis, tdgp_stream_t stream) {
    TDGP_CHECK(c2w && focal && vis, TDGP_EINVAL, "mesh_visibility_ms: null pointer");
    TDGP_CHECK((vertices || V == 0) && (triangles || T == 0), TDGP_EINVAL, "mesh_visibility_ms: null mesh pointer");
    TDGP_CHECK(V >= 0 && V <= 2147483647ll && T >= 0 && T <= 2147483647ll, TDGP_EINVAL, "mesh_visibility_ms: V and T must lie in [0, 2^31 - 1]");
    TDGP_CHECK(samples == 4 || samples == 16, TDGP_EINVAL, "mesh_visibility_ms: samples must be 4 or 16, got %d", samples);
    TDGP_CHECK(C >= 0 && h >= 2 && w >= 2 && h <= 16384 && w <= 16384, TDGP_EINVAL, "mesh_visibility_ms: need C >= 0 and 2 <= h, w <= 16384 (got C=%d, h=%d, w=%d)", C, h, w);
    TDGP_CHECK((int64_t)C * h * w * samples <= MESH_RAYS_MAX && (int64_t)C * T <= MESH_WORK_MAX, TDGP_EINVAL,
               "mesh_visibility_ms: too many samples or camera x triangle pairs for one call");
    TDGP_CHECK(near_ > 0.0f && near_ < __builtin_inff(), TDGP_EINVAL, "mesh_visibility_ms: near must be positive and finite");
    TDGP_CHECK(cull >= 0 && cull <= 2, TDGP_EINVAL, "mesh_visibility_ms: cull must be 0 (none), 1 (back) or 2 (front), got %d", cull);
    if (C == 0) return TDGP_OK;
    const int64_t keys = (int64_t)C * h * w * samples;
    if (hipMemsetAsync(vis, 0xff, (size_t)keys * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) {
        tdgp_set_error("mesh_visibility_ms: clearing the visibility buffer failed");
        return TDGP_ELAUNCH;
    }
    if (T == 0) return TDGP_OK;
    const dim3 grid((unsigned)cdiv64((int64_t)C * T, 256));
    if (samples == 4) {
        TDGP_LAUNCH("mesh_visibility_ms_kernel<4>", mesh_visibility_ms_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, vertices, V, triangles, T, c2w, focal, C, h,
                    w, near_, cull, (unsigned long long*)vis);
    } else {
        TDGP_LAUNCH("mesh_visibility_ms_kernel<16>", mesh_visibility_ms_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, vertices, V, triangles, T, c2w, focal, C,
                    h, w, near_, cull, (unsigned long long*)vis);
    }
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_resolve_ms(const uint64_t* vis, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* c2w,
                                  const float* focal, int C, int h, int w, int samples, float t_miss, const float* vertex_normal, const float* vertex_rgb,
                                  const uint8_t* image, int n, int r, int W, int H, int filter, int mode, const float* light, float ambient,
                                  const float* albedo, const float* background, float* rgb, float* coverage, int32_t* status, float* depth, int32_t* tri,
                                  float* normal, tdgp_stream_t stream) {
    TDGP_CHECK(vis && c2w && focal && albedo && background && rgb && coverage && status && depth && tri && normal, TDGP_EINVAL, "mesh_resolve_ms: null pointer");
    TDGP_CHECK((vertices || V == 0) && (triangles || T == 0), TDGP_EINVAL, "mesh_resolve_ms: null mesh pointer");
    TDGP_CHECK(V >= 0 && V <= 2147483647ll && T >= 0 && T <= 2147483647ll, TDGP_EINVAL, "mesh_resolve_ms: V and T must lie in [0, 2^31 - 1]");
    TDGP_CHECK(samples == 4 || samples == 16, TDGP_EINVAL, "mesh_resolve_ms: samples must be 4 or 16, got %d", samples);
    TDGP_CHECK(C >= 0 && h >= 2 && w >= 2 && h <= 16384 && w <= 16384, TDGP_EINVAL, "mesh_resolve_ms: need C >= 0 and 2 <= h, w <= 16384 (got C=%d, h=%d, w=%d)", C, h, w);
    TDGP_CHECK((int64_t)C * h * w * samples <= MESH_RAYS_MAX, TDGP_EINVAL, "mesh_resolve_ms: too many samples for one call");
    TDGP_CHECK(mode >= 0 && mode <= 2, TDGP_EINVAL, "mesh_resolve_ms: mode must be 0 (shaded), 1 (normals) or 2 (colour), got %d", mode);
    TDGP_CHECK(!(vertex_rgb && image), TDGP_EINVAL, "mesh_resolve_ms: the colour comes from vertex_rgb or from the texture, not both");
    TDGP_CHECK(mode != 2 || vertex_rgb || image || T == 0, TDGP_EINVAL, "mesh_resolve_ms: mode 2 (colour) needs vertex_rgb or a texture");
    if (image) {
        TDGP_CHECK(filter == 0 || filter == 1, TDGP_EINVAL, "mesh_resolve_ms: filter must be 0 (nearest) or 1 (bilinear), got %d", filter);
        TDGP_CHECK(n >= 2 && n <= 64 && r >= 0 && W >= 0 && H >= 0 && W <= 16384 && H <= 16384 && atlas_is(T, n, r, W, H), TDGP_EINVAL,
                   "mesh_resolve_ms: (texels %d, tiles_per_row %d, width %d, height %d) is not an atlas of %lld triangles", n, r, W, H, (long long)T);
    }
    if (C == 0) return TDGP_OK;
    const int64_t pixels = (int64_t)C * h * w;
    const MeshSurface f{vertex_normal, vertex_rgb, image, n, r, W, filter};
    const MeshShadeParams q{shade_params(mode, light, ambient, albedo, background)};
    const dim3 grid((unsigned)cdiv64(pixels * samples, 256));
    if (samples == 4) {
        TDGP_LAUNCH("mesh_resolve_ms_kernel<4>", mesh_resolve_ms_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)vis, vertices, V,
                    triangles, T, c2w, focal, pixels, h, w, t_miss, f, q, rgb, coverage, status, depth, tri, normal);
    } else {
        TDGP_LAUNCH("mesh_resolve_ms_kernel<16>", mesh_resolve_ms_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)vis, vertices, V,
                    triangles, T, c2w, focal, pixels, h, w, t_miss, f, q, rgb, coverage, status, depth, tri, normal);
    }
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// mesh_distance.hip -- how far one mesh is from another (contract in include/tdgp.h, restated line by line in
// tests/mesh_distance_reference.py): a uniform grid over the triangles, the closest point of the mesh per query point, surface samples and
// the area-weighted statistics of their distances (maximum = the sampled Hausdorff distance, mean, RMS).
//
//   prepare_kernel                                             per triangle: valid?, its fp32 box, its area in double
//   grid_count_kernel -> md_sums / md_scan -> grid_emit_kernel (cell, triangle) pairs in triangle order; the caller sorts them by cell (stable)
//   cell_start_kernel                                          cell_start [cells + 1] from the sorted keys: every entry written by exactly one lane
//   closest_kernel                                             one lane per point: shells of cells round the point's own, or the plain scan
//   sample_count_kernel -> md_sums / md_scan -> sample_emit_kernel
//   reduce_partials_kernel -> reduce_final_kernel              sums in double in ONE fixed order, the maximum with the lowest index
//
// Every distance is the same pure function of (point, triangle) in double, every operation rounded once (-ffp-contract=off), and the minimum
// over triangles breaks ties by the triangle index -- so the walk through the grid and the scan over all triangles return the same bits as
// long as the walk never skips the minimiser.  Positions come from scans, never from atomics: the same bytes on every run.  One-wave blocks
// for the walk: it is a data-dependent gather, and neighbouring sample points are neighbours in space.
#include "common.h"
#include "device_scan.h"

namespace {

constexpr int MD_BLOCK = 256;
constexpr int MD_WALK_BLOCK = 64;
constexpr int64_t MD_WS_HEAD = 64;                 // bytes in front of the block sums / partials: totals
constexpr int64_t MD_N_MAX = (int64_t)INT32_MAX;   // triangles, points, pairs, samples: int32 indices
constexpr int64_t MD_CELLS_MAX = 1ll << 24;
constexpr int MD_K_MAX = 64;
constexpr int MD_REDUCE_FIELDS = 3;

struct MdGrid {
    double lo[3];
    double cell;
    int n[3];
};

struct MdMesh {
    const float* verts;
    const int32_t* tris;
    int64_t T, V;
};

__device__ __forceinline__ double md_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void md_cross(const double (&a)[3], const double (&b)[3], double (&n)[3]) {
    n[0] = a[1] * b[2] - a[2] * b[1];
    n[1] = a[2] * b[0] - a[0] * b[2];
    n[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void md_sub(const double (&a)[3], const double (&b)[3], double (&r)[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = a[c] - b[c];
}

__device__ __forceinline__ bool md_finite(float x) { return fabsf(x) < __builtin_inff(); }

// the indices of triangle t, checked: three distinct ones inside [0, V)
__device__ __forceinline__ bool md_indices(const MdMesh& m, int64_t t, int (&idx)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) idx[i] = m.tris[t * 3 + i];
    if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0 || idx[0] >= m.V || idx[1] >= m.V || idx[2] >= m.V) return false;
    return idx[0] != idx[1] && idx[1] != idx[2] && idx[0] != idx[2];
}

__device__ __forceinline__ void md_load(const MdMesh& m, const int (&idx)[3], double (&p)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) p[i][c] = (double)m.verts[(int64_t)idx[i] * 3 + c];
}

// the closest point of segment (x, y) to p: a strictly smaller squared distance replaces the running one
__device__ __forceinline__ void md_edge(const double (&p)[3], const double (&x)[3], const double (&y)[3], double& d2, double (&q)[3]) {
    double e[3], px[3], r[3], d[3];
    md_sub(y, x, e);
    md_sub(p, x, px);
    const double ee = md_dot(e, e);
    double t = 0.0;
    if (ee != 0.0) {
        t = md_dot(px, e) / ee;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        r[c] = x[c] + t * e[c];
        d[c] = p[c] - r[c];
    }
    const double dd = md_dot(d, d);
    if (dd < d2) {
        d2 = dd;
#pragma unroll
        for (int c = 0; c < 3; c++) q[c] = r[c];
    }
}

// squared distance of p to triangle (a, b, c) and the closest point (include/tdgp.h: the face case, else the three edges in order)
__device__ __forceinline__ double md_point_triangle(const double (&p)[3], const double (&a)[3], const double (&b)[3], const double (&c)[3], double (&q)[3]) {
    double ab[3], ac[3], ap[3], n[3];
    md_sub(b, a, ab);
    md_sub(c, a, ac);
    md_sub(p, a, ap);
    md_cross(ab, ac, n);
    const double nn = md_dot(n, n);
    if (nn > 0.0) {
        double bc[3], bp[3], ca[3], cp[3], x[3];
        md_sub(c, b, bc);
        md_sub(p, b, bp);
        md_cross(bc, bp, x);
        const double s0 = md_dot(x, n);
        md_sub(a, c, ca);
        md_sub(p, c, cp);
        md_cross(ca, cp, x);
        const double s1 = md_dot(x, n);
        md_cross(ab, ap, x);
        const double s2 = md_dot(x, n);
        if (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) {
            const double s = md_dot(ap, n);
            const double f = s / nn;
#pragma unroll
            for (int k = 0; k < 3; k++) q[k] = p[k] - n[k] * f;
            return s * s / nn;
        }
    }
    double d2 = (double)__builtin_inff();
    md_edge(p, a, b, d2, q);
    md_edge(p, b, c, d2, q);
    md_edge(p, c, a, d2, q);
    return d2;
}

// floor((x - lo) / cell) clamped into [0, n - 1]; every operation in double
__device__ __forceinline__ int md_cell(double x, double lo, double cell, int n) {
    const double v = floor((x - lo) / cell);
    if (!(v > 0.0)) return 0;
    return v >= (double)(n - 1) ? n - 1 : (int)v;
}

__global__ __launch_bounds__(1024) void md_scan_kernel(uint32_t* __restrict__ block_sums, int64_t nb, int64_t* __restrict__ total) {
    scan_block_sums<1>(block_sums, nb, total);
}

__global__ __launch_bounds__(MD_BLOCK) void md_sums_kernel(const int32_t* __restrict__ counts, int64_t n, uint32_t* __restrict__ sums) {
    __shared__ int sm[MD_BLOCK / 64];
    const int64_t i = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<MD_BLOCK>(i < n ? counts[i] : 0, sm, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = (uint32_t)total;
}

// ---- triangles: valid, box, area -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MD_BLOCK) void prepare_kernel(MdMesh m, uint8_t* __restrict__ valid, float* __restrict__ box, double* __restrict__ area) {
    const int64_t t = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (t >= m.T) return;
    int idx[3];
    bool ok = md_indices(m, t, idx);
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    double ar = 0.0;
    if (ok) {
        float f[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                f[i][c] = m.verts[(int64_t)idx[i] * 3 + c];
                ok = ok && md_finite(f[i][c]);
            }
        if (ok) {
            double p[3][3], ab[3], ac[3], n[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                lo[c] = fminf(fminf(f[0][c], f[1][c]), f[2][c]);
                hi[c] = fmaxf(fmaxf(f[0][c], f[1][c]), f[2][c]);
#pragma unroll
                for (int i = 0; i < 3; i++) p[i][c] = (double)f[i][c];
            }
            md_sub(p[1], p[0], ab);
            md_sub(p[2], p[0], ac);
            md_cross(ab, ac, n);
            ar = 0.5 * sqrt(md_dot(n, n));
        }
    }
    valid[t] = ok ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        box[t * 6 + c] = ok ? lo[c] : 0.f;
        box[t * 6 + 3 + c] = ok ? hi[c] : 0.f;
    }
    area[t] = ok ? ar : 0.0;
}

// ---- the grid ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void md_cell_range(const float* __restrict__ box, int64_t t, const MdGrid& g, int (&c0)[3], int (&c1)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c0[k] = md_cell((double)box[t * 6 + k], g.lo[k], g.cell, g.n[k]);
        c1[k] = md_cell((double)box[t * 6 + 3 + k], g.lo[k], g.cell, g.n[k]);
        if (c1[k] < c0[k]) c1[k] = c0[k];
    }
}

__global__ __launch_bounds__(MD_BLOCK) void grid_count_kernel(const float* __restrict__ box, const uint8_t* __restrict__ valid, int64_t T, MdGrid g,
                                                              int32_t* __restrict__ counts) {
    const int64_t t = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (t >= T) return;
    int n = 0;
    if (valid[t]) {
        int c0[3], c1[3];
        md_cell_range(box, t, g, c0, c1);
        n = (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);       // <= the cells of the grid <= 2^24
    }
    counts[t] = n;
}

__global__ __launch_bounds__(MD_BLOCK) void grid_emit_kernel(const float* __restrict__ box, const int32_t* __restrict__ counts, int64_t T, MdGrid g,
                                                             const uint32_t* __restrict__ sums, int32_t* __restrict__ pair_cell, int32_t* __restrict__ pair_tri,
                                                             int64_t P) {
    __shared__ int sm[MD_BLOCK / 64];
    const int64_t t = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    const int n = t < T ? counts[t] : 0;
    int total;
    int64_t at = (int64_t)sums[blockIdx.x] + block_excl_scan<MD_BLOCK>(n, sm, total);
    if (n <= 0) return;
    int c0[3], c1[3];
    md_cell_range(box, t, g, c0, c1);
    const int64_t end = min(at + n, P);
    for (int z = c0[2]; z <= c1[2]; z++)
        for (int y = c0[1]; y <= c1[1]; y++)
            for (int x = c0[0]; x <= c1[0]; x++) {
                if (at >= end) return;
                pair_cell[at] = (z * g.n[1] + y) * g.n[0] + x;
                pair_tri[at] = (int32_t)t;
                at++;
            }
}

// lane i of [0, P]: the cells after the one before pair i up to pair i's own start at i (the last lane: up to `cells`)
__global__ __launch_bounds__(MD_BLOCK) void cell_start_kernel(const int32_t* __restrict__ key, int64_t P, int64_t cells, int32_t* __restrict__ cell_start) {
    const int64_t i = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (i > P) return;
    int64_t prev = i == 0 ? -1 : (int64_t)key[i - 1];
    int64_t cur = i == P ? cells : (int64_t)key[i];
    prev = prev < -1 ? -1 : (prev > cells ? cells : prev);
    cur = cur > cells ? cells : cur;
    for (int64_t c = prev + 1; c <= cur; c++) cell_start[c] = (int32_t)i;
}

// ---- closest points ------------------------------------------------------------------------------------------------------------------------
struct MdBest {
    double d2;
    int tri;
};

__device__ __forceinline__ void md_try(const MdMesh& m, const double (&p)[3], int64_t t, MdBest& best) {
    int idx[3];
    if (t < 0 || t >= m.T || !md_indices(m, t, idx)) return;
    double v[3][3], q[3];
    md_load(m, idx, v);
    const double d2 = md_point_triangle(p, v[0], v[1], v[2], q);
    if (d2 < best.d2 || (d2 == best.d2 && (int)t < best.tri)) {
        best.d2 = d2;
        best.tri = (int)t;
    }
}

__global__ __launch_bounds__(MD_WALK_BLOCK) void closest_kernel(const float* __restrict__ points, int64_t N, MdMesh m, const uint8_t* __restrict__ valid, MdGrid g,
                                                                const int32_t* __restrict__ cell_start, const int32_t* __restrict__ pair_tri, int64_t P,
                                                                int brute_force, double* __restrict__ sqdist, float* __restrict__ distance,
                                                                int32_t* __restrict__ triangle, float* __restrict__ closest, int32_t* __restrict__ evals) {
    const int64_t i = blockIdx.x * (int64_t)MD_WALK_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float nanf_ = __builtin_nanf("");
    const float f[3] = {points[i * 3 + 0], points[i * 3 + 1], points[i * 3 + 2]};
    MdBest best = {(double)__builtin_inff(), INT32_MAX};
    int count = 0;
    if (!(md_finite(f[0]) && md_finite(f[1]) && md_finite(f[2]))) {
        sqdist[i] = (double)nanf_;
        distance[i] = nanf_;
        triangle[i] = -1;
#pragma unroll
        for (int c = 0; c < 3; c++) closest[i * 3 + c] = nanf_;
        if (evals) evals[i] = 0;
        return;
    }
    const double p[3] = {(double)f[0], (double)f[1], (double)f[2]};
    if (brute_force) {
        for (int64_t t = 0; t < m.T; t++) {
            if (!valid[t]) continue;
            md_try(m, p, t, best);
            count++;
        }
    } else if (P > 0) {
        int c[3];
        double a[3];                                                   // the point in the grid's frame; cell planes sit at m * cell, an exact product
        int rmax = 1;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            c[k] = md_cell(p[k], g.lo[k], g.cell, g.n[k]);
            a[k] = p[k] - g.lo[k];
            rmax = g.n[k] > rmax ? g.n[k] : rmax;
        }
        for (int r = 0; r < rmax; r++) {                               // at r = max(n_k) - 1 the block covers the grid: the loop cannot run on
            const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.n[2] - 1);
            const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
            const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.n[0] - 1);
            for (int z = z0; z <= z1; z++)
                for (int y = y0; y <= y1; y++) {
                    const bool whole = (z - c[2] == r) || (c[2] - z == r) || (y - c[1] == r) || (c[1] - y == r);
                    const int step = whole || r == 0 ? 1 : 2 * r;          // an inner row of the shell: its two ends only
                    for (int x = whole ? x0 : c[0] - r; x <= (whole ? x1 : c[0] + r); x += step) {
                        if (x < x0 || x > x1) continue;
                        const int64_t cell = ((int64_t)z * g.n[1] + y) * g.n[0] + x;
                        int64_t s = cell_start[cell], e = cell_start[cell + 1];
                        s = s < 0 ? 0 : (s > P ? P : s);
                        e = e < s ? s : (e > P ? P : e);
                        for (int64_t j = s; j < e; j++) {
                            md_try(m, p, pair_tri[j], best);
                            count++;
                        }
                    }
                }
            // a triangle not yet seen lies wholly beyond one of the block's open sides: the smallest of their distances bounds it from below
            double lb = (double)__builtin_inff();
            bool open = false;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (c[k] - r > 0) {
                    const double mc = (double)(c[k] - r) * g.cell;
                    const double d = (a[k] - mc) - (fabs(a[k]) + mc) * 0x1p-48;
                    lb = fmin(lb, d > 0.0 ? d : 0.0);
                    open = true;
                }
                if (c[k] + r < g.n[k] - 1) {
                    const double mc = (double)(c[k] + r + 1) * g.cell;
                    const double d = (mc - a[k]) - (fabs(a[k]) + mc) * 0x1p-48;
                    lb = fmin(lb, d > 0.0 ? d : 0.0);
                    open = true;
                }
            }
            if (!open) break;
            if ((lb * lb) * (1.0 - 0x1p-40) > best.d2) break;
        }
    }
    if (evals) evals[i] = count;
    if (best.tri == INT32_MAX) {                                       // no valid triangle
        sqdist[i] = (double)__builtin_inff();
        distance[i] = __builtin_inff();
        triangle[i] = -1;
#pragma unroll
        for (int k = 0; k < 3; k++) closest[i * 3 + k] = nanf_;
        return;
    }
    int idx[3];
    double v[3][3], q[3] = {0.0, 0.0, 0.0};
    md_indices(m, best.tri, idx);
    md_load(m, idx, v);
    const double d2 = md_point_triangle(p, v[0], v[1], v[2], q);          // the winner once more: the same bits, and its closest point
    sqdist[i] = d2;
    distance[i] = (float)sqrt(d2);
    triangle[i] = best.tri;
#pragma unroll
    for (int k = 0; k < 3; k++) closest[i * 3 + k] = (float)q[k];
}

// ---- surface samples -----------------------------------------------------------------------------------------------------------------------
// k = clamp(ceil(longest edge / spacing), 1, 64) of a valid triangle
__device__ __forceinline__ int md_subdivisions(const double (&p)[3][3], double spacing) {
    double e[3];
    md_sub(p[1], p[0], e);
    double l2 = md_dot(e, e);
    md_sub(p[2], p[1], e);
    l2 = fmax(l2, md_dot(e, e));
    md_sub(p[0], p[2], e);
    l2 = fmax(l2, md_dot(e, e));
    const double k = ceil(sqrt(l2) / spacing);
    return !(k > 1.0) ? 1 : (k >= (double)MD_K_MAX ? MD_K_MAX : (int)k);
}

__global__ __launch_bounds__(MD_BLOCK) void sample_count_kernel(MdMesh m, const uint8_t* __restrict__ valid, double spacing, int32_t* __restrict__ counts) {
    const int64_t t = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    if (t >= m.T) return;
    int n = 0, idx[3];
    if (valid[t] && md_indices(m, t, idx)) {
        double p[3][3];
        md_load(m, idx, p);
        const int k = md_subdivisions(p, spacing);
        n = k * k + 3;
    }
    counts[t] = n;
}

__global__ __launch_bounds__(MD_BLOCK) void sample_emit_kernel(MdMesh m, const int32_t* __restrict__ counts, double spacing, const uint32_t* __restrict__ sums,
                                                               float* __restrict__ points, double* __restrict__ weight, int32_t* __restrict__ triangle, int64_t S) {
    __shared__ int sm[MD_BLOCK / 64];
    const int64_t t = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    const int n = t < m.T ? counts[t] : 0;
    int total, idx[3];
    int64_t at = (int64_t)sums[blockIdx.x] + block_excl_scan<MD_BLOCK>(n, sm, total);
    if (n <= 0 || !md_indices(m, t, idx)) return;
    double p[3][3], ab[3], ac[3], nrm[3];
    md_load(m, idx, p);
    const int k = md_subdivisions(p, spacing);
    if (k * k + 3 != n || at + n > S) return;                          // counts and spacing belong together; writes never pass S
    md_sub(p[1], p[0], ab);
    md_sub(p[2], p[0], ac);
    md_cross(ab, ac, nrm);
    const double w = (0.5 * sqrt(md_dot(nrm, nrm))) / (double)(k * k);
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int c = 0; c < 3; c++) points[at * 3 + c] = m.verts[(int64_t)idx[i] * 3 + c];
        weight[at] = 0.0;
        triangle[at] = (int32_t)t;
        at++;
    }
    for (int pass = 0; pass < 2; pass++) {                             // upright sub-triangles, then inverted ones
        const double third = pass == 0 ? 1.0 / 3.0 : 2.0 / 3.0;
        for (int i = 0; i + pass < k; i++)
            for (int j = 0; i + j + pass < k; j++) {
                const double u = ((double)i + third) / (double)k, v = ((double)j + third) / (double)k;
#pragma unroll
                for (int c = 0; c < 3; c++) points[at * 3 + c] = (float)((p[0][c] + u * ab[c]) + v * ac[c]);
                weight[at] = w;
                triangle[at] = (int32_t)t;
                at++;
            }
    }
}

// ---- statistics ----------------------------------------------------------------------------------------------------------------------------
// sum over the block's 256 slots as a tree: slot i takes slot i + s for s = 128, 64, ... 1; the maximum with the lowest index alongside
struct MdAcc {
    double s[MD_REDUCE_FIELDS];
    float mx;
    int64_t arg;
};

__device__ __forceinline__ void md_block_tree(MdAcc& a, double (*sh)[MD_BLOCK], float* shm, int64_t* sha) {
    const int t = threadIdx.x;
#pragma unroll
    for (int f = 0; f < MD_REDUCE_FIELDS; f++) sh[f][t] = a.s[f];
    shm[t] = a.mx;
    sha[t] = a.arg;
    __syncthreads();
    for (int s = MD_BLOCK / 2; s >= 1; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int f = 0; f < MD_REDUCE_FIELDS; f++) sh[f][t] = sh[f][t] + sh[f][t + s];
            const float om = shm[t + s];
            const int64_t oa = sha[t + s];
            if (oa >= 0 && (sha[t] < 0 || om > shm[t] || (om == shm[t] && oa < sha[t]))) {
                shm[t] = om;
                sha[t] = oa;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int f = 0; f < MD_REDUCE_FIELDS; f++) a.s[f] = sh[f][0];
    a.mx = shm[0];
    a.arg = sha[0];
}

struct MdPartial {
    double s[MD_REDUCE_FIELDS];
    double mx;
    int64_t arg;
};

__global__ __launch_bounds__(MD_BLOCK) void reduce_partials_kernel(const double* __restrict__ weight, const float* __restrict__ distance, int64_t N,
                                                                   MdPartial* __restrict__ partials) {
    __shared__ double sh[MD_REDUCE_FIELDS][MD_BLOCK];
    __shared__ float shm[MD_BLOCK];
    __shared__ int64_t sha[MD_BLOCK];
    const int64_t i = blockIdx.x * (int64_t)MD_BLOCK + threadIdx.x;
    MdAcc a = {{0.0, 0.0, 0.0}, 0.f, -1};
    if (i < N) {
        const double w = weight[i];
        a.s[0] = w;
        if (distance) {
            const float d = distance[i];
            const double dd = (double)d;
            a.s[1] = w * dd;
            a.s[2] = w * (dd * dd);
            if (d == d) {                                              // a NaN never is the maximum
                a.mx = d;
                a.arg = i;
            }
        }
    }
    md_block_tree(a, sh, shm, sha);
    if (threadIdx.x == 0) {
        MdPartial o;
#pragma unroll
        for (int f = 0; f < MD_REDUCE_FIELDS; f++) o.s[f] = a.s[f];
        o.mx = (double)a.mx;
        o.arg = a.arg;
        partials[blockIdx.x] = o;
    }
}

// ONE block: thread t adds partials t, t + 256, ... in that order, then the same tree
__global__ __launch_bounds__(MD_BLOCK) void reduce_final_kernel(const MdPartial* __restrict__ partials, int64_t nb, MdPartial* __restrict__ out) {
    __shared__ double sh[MD_REDUCE_FIELDS][MD_BLOCK];
    __shared__ float shm[MD_BLOCK];
    __shared__ int64_t sha[MD_BLOCK];
    MdAcc a = {{0.0, 0.0, 0.0}, 0.f, -1};
    for (int64_t b = threadIdx.x; b < nb; b += MD_BLOCK) {
        const MdPartial o = partials[b];
#pragma unroll
        for (int f = 0; f < MD_REDUCE_FIELDS; f++) a.s[f] = a.s[f] + o.s[f];
        const float om = (float)o.mx;
        if (o.arg >= 0 && (a.arg < 0 || om > a.mx || (om == a.mx && o.arg < a.arg))) {
            a.mx = om;
            a.arg = o.arg;
        }
    }
    md_block_tree(a, sh, shm, sha);
    if (threadIdx.x == 0) {
        MdPartial o;
#pragma unroll
        for (int f = 0; f < MD_REDUCE_FIELDS; f++) o.s[f] = a.s[f];
        o.mx = (double)a.mx;
        o.arg = a.arg;
        out[0] = o;
    }
}

static_assert(sizeof(MdPartial) == 40, "five 8-byte fields");

int md_grid_args(const char* who, const float* lo, float cell, const int* dims, MdGrid& g) {
    TDGP_CHECK(lo && dims, TDGP_EINVAL, "%s: null pointer", who);
    TDGP_CHECK(cell > 0.f, TDGP_EINVAL, "%s: cell must be greater than 0 (got %g)", who, (double)cell);
    int64_t cells = 1;
    for (int k = 0; k < 3; k++) {
        TDGP_CHECK(lo[k] - lo[k] == 0.f, TDGP_EINVAL, "%s: the box must be finite", who);
        TDGP_CHECK(dims[k] >= 1 && (int64_t)dims[k] <= MD_CELLS_MAX, TDGP_EINVAL, "%s: every grid dimension must lie in [1, 2^24] (got %d)", who, dims[k]);
        g.lo[k] = (double)lo[k];
        g.n[k] = dims[k];
        cells *= dims[k];
        TDGP_CHECK(cells <= MD_CELLS_MAX, TDGP_EINVAL, "%s: the grid has more than 2^24 cells", who);
    }
    g.cell = (double)cell;
    return 0;
}

int md_scan(const int32_t* counts, int64_t n, void* workspace, hipStream_t s) {
    const int64_t nb = cdiv64(n, MD_BLOCK);
    uint32_t* sums = (uint32_t*)((char*)workspace + MD_WS_HEAD);
    TDGP_LAUNCH("md_sums_kernel", md_sums_kernel, dim3((unsigned)nb), dim3(MD_BLOCK), 0, s, counts, n, sums);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("md_scan_kernel", md_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, (int64_t*)workspace);
    TDGP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

#define MD_T_CHECK(who, T) TDGP_CHECK((T) >= 0 && (T) <= MD_N_MAX, TDGP_EINVAL, "%s: need 0 <= T <= 2^31 - 1 (got %lld)", who, (long long)(T))

TDGP_API int tdgp_mesh_distance_prepare(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, uint8_t* valid, float* box, double* area,
                                        tdgp_stream_t stream) {
    MD_T_CHECK("mesh_distance_prepare", T);
    TDGP_CHECK(V >= 0 && V <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_prepare: need 0 <= V <= 2^31 - 1 (got %lld)", (long long)V);
    if (T == 0) return 0;
    TDGP_CHECK((vertices || V == 0) && triangles && valid && box && area, TDGP_EINVAL, "mesh_distance_prepare: null pointer");
    const MdMesh m = {vertices, triangles, T, V};
    TDGP_LAUNCH("md_prepare_kernel", prepare_kernel, dim3((unsigned)cdiv64(T, MD_BLOCK)), dim3(MD_BLOCK), 0, (hipStream_t)stream, m, valid, box, area);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int tdgp_mesh_distance_grid_count(const float* box, const uint8_t* valid, int64_t T, const float* lo, float cell, const int* dims, int32_t* counts,
                                           tdgp_stream_t stream) {
    MD_T_CHECK("mesh_distance_grid_count", T);
    MdGrid g;
    if (int rc = md_grid_args("mesh_distance_grid_count", lo, cell, dims, g)) return rc;
    if (T == 0) return 0;
    TDGP_CHECK(box && valid && counts, TDGP_EINVAL, "mesh_distance_grid_count: null pointer");
    TDGP_LAUNCH("md_grid_count_kernel", grid_count_kernel, dim3((unsigned)cdiv64(T, MD_BLOCK)), dim3(MD_BLOCK), 0, (hipStream_t)stream, box, valid, T, g, counts);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int64_t tdgp_mesh_distance_scan_workspace_bytes(int64_t T) {
    if (T < 0 || T > MD_N_MAX) return -1;
    return MD_WS_HEAD + align64(cdiv64(T, MD_BLOCK) * (int64_t)sizeof(uint32_t));
}

#define MD_WS_CHECK(who, T)                                                                                                          \
    do {                                                                                                                             \
        TDGP_CHECK(workspace, TDGP_EINVAL, "%s: null workspace", who);                                                              \
        TDGP_CHECK(workspace_bytes >= tdgp_mesh_distance_scan_workspace_bytes(T), TDGP_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, \
                   (long long)workspace_bytes, (long long)tdgp_mesh_distance_scan_workspace_bytes(T));                              \
    } while (0)

TDGP_API int tdgp_mesh_distance_grid_emit(const float* box, const int32_t* counts, int64_t T, const float* lo, float cell, const int* dims, void* workspace,
                                          int64_t workspace_bytes, int32_t* pair_cell, int32_t* pair_triangle, int64_t P, tdgp_stream_t stream) {
    MD_T_CHECK("mesh_distance_grid_emit", T);
    TDGP_CHECK(P >= 0 && P <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_grid_emit: need 0 <= P <= 2^31 - 1 (got %lld)", (long long)P);
    MdGrid g;
    if (int rc = md_grid_args("mesh_distance_grid_emit", lo, cell, dims, g)) return rc;
    if (T == 0 || P == 0) return 0;
    MD_WS_CHECK("mesh_distance_grid_emit", T);
    TDGP_CHECK(box && counts && pair_cell && pair_triangle, TDGP_EINVAL, "mesh_distance_grid_emit: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = md_scan(counts, T, workspace, s)) return rc;
    TDGP_LAUNCH("md_grid_emit_kernel", grid_emit_kernel, dim3((unsigned)cdiv64(T, MD_BLOCK)), dim3(MD_BLOCK), 0, s, box, counts, T, g,
                (const uint32_t*)((char*)workspace + MD_WS_HEAD), pair_cell, pair_triangle, P);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int tdgp_mesh_distance_cell_start(const int32_t* sorted_cell, int64_t P, int64_t cells, int32_t* cell_start, tdgp_stream_t stream) {
    TDGP_CHECK(P >= 0 && P <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_cell_start: need 0 <= P <= 2^31 - 1 (got %lld)", (long long)P);
    TDGP_CHECK(cells >= 1 && cells <= MD_CELLS_MAX, TDGP_EINVAL, "mesh_distance_cell_start: need 1 <= cells <= 2^24 (got %lld)", (long long)cells);
    TDGP_CHECK((sorted_cell || P == 0) && cell_start, TDGP_EINVAL, "mesh_distance_cell_start: null pointer");
    TDGP_LAUNCH("md_cell_start_kernel", cell_start_kernel, dim3((unsigned)cdiv64(P + 1, MD_BLOCK)), dim3(MD_BLOCK), 0, (hipStream_t)stream, sorted_cell, P, cells,
                cell_start);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int tdgp_mesh_distance_closest(const float* points, int64_t N, const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const uint8_t* valid,
                                        const float* lo, float cell, const int* dims, const int32_t* cell_start, const int32_t* pair_triangle, int64_t P,
                                        int brute_force, double* sqdist, float* distance, int32_t* triangle, float* closest, int32_t* evaluated,
                                        tdgp_stream_t stream) {
    TDGP_CHECK(N >= 0 && N <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_closest: need 0 <= N <= 2^31 - 1 (got %lld)", (long long)N);
    MD_T_CHECK("mesh_distance_closest", T);
    TDGP_CHECK(V >= 0 && V <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_closest: need 0 <= V <= 2^31 - 1 (got %lld)", (long long)V);
    TDGP_CHECK(P >= 0 && P <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_closest: need 0 <= P <= 2^31 - 1 (got %lld)", (long long)P);
    TDGP_CHECK(brute_force == 0 || brute_force == 1, TDGP_EINVAL, "mesh_distance_closest: brute_force must be 0 or 1");
    MdGrid g;
    if (int rc = md_grid_args("mesh_distance_closest", lo, cell, dims, g)) return rc;
    if (N == 0) return 0;
    TDGP_CHECK(points && sqdist && distance && triangle && closest, TDGP_EINVAL, "mesh_distance_closest: null pointer");
    TDGP_CHECK(T == 0 || (triangles && valid && (vertices || V == 0)), TDGP_EINVAL, "mesh_distance_closest: null pointer");
    TDGP_CHECK(brute_force || P == 0 || (cell_start && pair_triangle), TDGP_EINVAL, "mesh_distance_closest: null pointer");
    const MdMesh m = {vertices, triangles, T, V};
    TDGP_LAUNCH("md_closest_kernel", closest_kernel, dim3((unsigned)cdiv64(N, MD_WALK_BLOCK)), dim3(MD_WALK_BLOCK), 0, (hipStream_t)stream, points, N, m, valid, g,
                cell_start, pair_triangle, P, brute_force, sqdist, distance, triangle, closest, evaluated);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int tdgp_mesh_distance_sample_count(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const uint8_t* valid, float spacing,
                                             int32_t* counts, tdgp_stream_t stream) {
    MD_T_CHECK("mesh_distance_sample_count", T);
    TDGP_CHECK(V >= 0 && V <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_sample_count: need 0 <= V <= 2^31 - 1 (got %lld)", (long long)V);
    TDGP_CHECK(spacing > 0.f && spacing - spacing == 0.f, TDGP_EINVAL, "mesh_distance_sample_count: spacing must be positive and finite (got %g)", (double)spacing);
    if (T == 0) return 0;
    TDGP_CHECK((vertices || V == 0) && triangles && valid && counts, TDGP_EINVAL, "mesh_distance_sample_count: null pointer");
    const MdMesh m = {vertices, triangles, T, V};
    TDGP_LAUNCH("md_sample_count_kernel", sample_count_kernel, dim3((unsigned)cdiv64(T, MD_BLOCK)), dim3(MD_BLOCK), 0, (hipStream_t)stream, m, valid,
                (double)spacing, counts);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int tdgp_mesh_distance_sample_emit(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const int32_t* counts, float spacing,
                                            void* workspace, int64_t workspace_bytes, float* points, double* weight, int32_t* triangle, int64_t S,
                                            tdgp_stream_t stream) {
    MD_T_CHECK("mesh_distance_sample_emit", T);
    TDGP_CHECK(V >= 0 && V <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_sample_emit: need 0 <= V <= 2^31 - 1 (got %lld)", (long long)V);
    TDGP_CHECK(S >= 0 && S <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_sample_emit: need 0 <= S <= 2^31 - 1 (got %lld)", (long long)S);
    TDGP_CHECK(spacing > 0.f && spacing - spacing == 0.f, TDGP_EINVAL, "mesh_distance_sample_emit: spacing must be positive and finite (got %g)", (double)spacing);
    if (T == 0 || S == 0) return 0;
    MD_WS_CHECK("mesh_distance_sample_emit", T);
    TDGP_CHECK(vertices && triangles && counts && points && weight && triangle, TDGP_EINVAL, "mesh_distance_sample_emit: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = md_scan(counts, T, workspace, s)) return rc;
    const MdMesh m = {vertices, triangles, T, V};
    TDGP_LAUNCH("md_sample_emit_kernel", sample_emit_kernel, dim3((unsigned)cdiv64(T, MD_BLOCK)), dim3(MD_BLOCK), 0, s, m, counts, (double)spacing,
                (const uint32_t*)((char*)workspace + MD_WS_HEAD), points, weight, triangle, S);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int64_t tdgp_mesh_distance_reduce_workspace_bytes(int64_t N) {
    if (N < 0 || N > MD_N_MAX) return -1;
    return MD_WS_HEAD + align64(cdiv64(N, MD_BLOCK) * (int64_t)sizeof(MdPartial));
}

TDGP_API int tdgp_mesh_distance_reduce(const double* weight, const float* distance, int64_t N, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(N >= 0 && N <= MD_N_MAX, TDGP_EINVAL, "mesh_distance_reduce: need 0 <= N <= 2^31 - 1 (got %lld)", (long long)N);
    TDGP_CHECK(workspace, TDGP_EINVAL, "mesh_distance_reduce: null workspace");
    TDGP_CHECK(workspace_bytes >= tdgp_mesh_distance_reduce_workspace_bytes(N), TDGP_EWORKSPACE, "mesh_distance_reduce: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)tdgp_mesh_distance_reduce_workspace_bytes(N));
    TDGP_CHECK(weight || N == 0, TDGP_EINVAL, "mesh_distance_reduce: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = cdiv64(N, MD_BLOCK);
    MdPartial* partials = (MdPartial*)((char*)workspace + MD_WS_HEAD);
    if (nb > 0) {
        TDGP_LAUNCH("md_reduce_partials_kernel", reduce_partials_kernel, dim3((unsigned)nb), dim3(MD_BLOCK), 0, s, weight, distance, N, partials);
        TDGP_LAUNCH_CHECK();
    }
    TDGP_LAUNCH("md_reduce_final_kernel", reduce_final_kernel, dim3(1), dim3(MD_BLOCK), 0, s, (const MdPartial*)partials, nb, (MdPartial*)workspace);
    TDGP_LAUNCH_CHECK();
    return 0;
}

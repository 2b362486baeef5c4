// mesh_rays.hip -- what a ray hits on a mesh (contract in include/tdgp.h, restated line by line in
// tests/mesh_rays_reference.py): first hit or any hit of arbitrary rays against the triangle grid of mesh_distance.hip, and ambient occlusion.
//
//   cast_kernel   one lane per ray: the slabs of the grid along the ray's major axis, or the plain scan; first hit, or any hit (the flag only)
//   ao_kernel     one lane per (point, direction): the same walk in any-hit mode, the unoccluded lanes of a point counted with one ballot
//
// The ray-triangle function is one pure function of (ray, triangle) in double, every operation rounded once (-ffp-contract=off): the
// translate / shear / scale form of Woop, Benthin and Wald (2013), in which the sheared coordinates of a vertex depend on that vertex and the
// ray alone -- the edge function of a shared edge is the same bits up to sign in both of its triangles, so no ray passes between them.  The
// hit is the accepted triangle with the smallest t, ties to the smallest triangle index: the walk returns the bits of the scan as long as it
// never skips the minimiser.  No LDS, no matrix pipe, no atomics: fp64 VALU work and dependent gathers, one-wave blocks as closest_kernel.
#include "common.h"

namespace {

constexpr int MR_BLOCK = 64;
constexpr int64_t MR_N_MAX = (int64_t)INT32_MAX;
constexpr int64_t MR_CELLS_MAX = 1ll << 24;
constexpr int MR_TABLES_MAX = 64;

struct MrGrid {
    double lo[3];
    double cell;
    int n[3];
};

struct MrMesh {
    const float* verts;
    const int32_t* tris;
    int64_t T, V;
};

struct MrLists {
    const int32_t* cell_start;
    const int32_t* pair_tri;
    int64_t P;
};

// the ray in its own frame: axes (kx, ky, kz), origin permuted into them, the shear and the scale
struct MrRay {
    double ox, oy, oz;
    double Sx, Sy, Sz;
    int kx, ky, kz;
};

struct MrHit {
    double t, U, V, W, det;
};

struct MrBest {
    double t;
    int tri;
};

__device__ __forceinline__ bool mr_finite(float x) { return fabsf(x) < __builtin_inff(); }
__device__ __forceinline__ bool mr_finite(double x) { return fabs(x) < (double)__builtin_inff(); }

// component k of (v0, v1, v2) without an indexed register array
template <typename X>
__device__ __forceinline__ X mr_sel(X v0, X v1, X v2, int k) {
    return k == 0 ? v0 : (k == 1 ? v1 : v2);
}

__device__ __forceinline__ void mr_setup(const double (&o)[3], const double (&d)[3], MrRay& r) {
    int kz = 0;
    double m = fabs(d[0]);
    if (fabs(d[1]) > m) {
        kz = 1;
        m = fabs(d[1]);
    }
    if (fabs(d[2]) > m) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    const double dz = mr_sel(d[0], d[1], d[2], kz);
    if (dz < 0.0) {
        const int s = kx;
        kx = ky;
        ky = s;
    }
    r.kx = kx;
    r.ky = ky;
    r.kz = kz;
    r.Sx = mr_sel(d[0], d[1], d[2], kx) / dz;
    r.Sy = mr_sel(d[0], d[1], d[2], ky) / dz;
    r.Sz = 1.0 / dz;
    r.ox = mr_sel(o[0], o[1], o[2], kx);
    r.oy = mr_sel(o[0], o[1], o[2], ky);
    r.oz = mr_sel(o[0], o[1], o[2], kz);
}

// include/tdgp.h, THE RAY AND THE TRIANGLE: accepted iff t_min <= t <= t_max
__device__ __forceinline__ bool mr_test(const MrRay& r, const float (&f)[3][3], double t_min, double t_max, MrHit& h) {
    double x[3], y[3], z[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double px = (double)mr_sel(f[i][0], f[i][1], f[i][2], r.kx) - r.ox;
        const double py = (double)mr_sel(f[i][0], f[i][1], f[i][2], r.ky) - r.oy;
        z[i] = (double)mr_sel(f[i][0], f[i][1], f[i][2], r.kz) - r.oz;
        x[i] = px - r.Sx * z[i];
        y[i] = py - r.Sy * z[i];
    }
    h.U = x[2] * y[1] - y[2] * x[1];
    h.V = x[0] * y[2] - y[0] * x[2];
    h.W = x[1] * y[0] - y[1] * x[0];
    if ((h.U < 0.0 || h.V < 0.0 || h.W < 0.0) && (h.U > 0.0 || h.V > 0.0 || h.W > 0.0)) return false;
    h.det = (h.U + h.V) + h.W;
    if (h.det == 0.0) return false;
    h.t = ((h.U * (r.Sz * z[0]) + h.V * (r.Sz * z[1])) + h.W * (r.Sz * z[2])) / h.det;
    return h.t >= t_min && h.t <= t_max;
}

// the indices of triangle t, checked, and its nine coordinates
__device__ __forceinline__ bool mr_load(const MrMesh& m, int64_t t, float (&f)[3][3]) {
    if (t < 0 || t >= m.T) return false;
    int idx[3];
#pragma unroll
    for (int i = 0; i < 3; i++) idx[i] = m.tris[t * 3 + i];
    if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0 || idx[0] >= m.V || idx[1] >= m.V || idx[2] >= m.V) return false;
    if (idx[0] == idx[1] || idx[1] == idx[2] || idx[0] == idx[2]) return false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) f[i][c] = m.verts[(int64_t)idx[i] * 3 + c];
    return true;
}

__device__ __forceinline__ bool mr_try(const MrMesh& m, const MrRay& r, double t_min, double t_max, int64_t t, MrBest& best) {
    float f[3][3];
    if (!mr_load(m, t, f)) return false;
    MrHit h;
    if (!mr_test(r, f, t_min, t_max, h)) return false;
    if (h.t < best.t || (h.t == best.t && (int)t < best.tri)) {
        best.t = h.t;
        best.tri = (int)t;
    }
    return true;
}

// floor(v / cell) clamped into [0, n - 1]: v is a coordinate in the grid's frame (lo already taken off)
__device__ __forceinline__ int mr_cell(double v, double cell, int n) {
    const double c = floor(v / cell);
    if (!(c > 0.0)) return 0;
    return c >= (double)(n - 1) ? n - 1 : (int)c;
}

// the list of one cell; true when any_hit and a triangle was accepted
__device__ __forceinline__ bool mr_list(const MrMesh& m, const MrLists& l, const MrRay& r, double t_min, double t_max, int64_t cell, bool any_hit, MrBest& best,
                                        int& count) {
    int64_t s = l.cell_start[cell], e = l.cell_start[cell + 1];
    s = s < 0 ? 0 : (s > l.P ? l.P : s);
    e = e < s ? s : (e > l.P ? l.P : e);
    for (int64_t j = s; j < e; j++) {
        count++;
        if (mr_try(m, r, t_min, t_max, l.pair_tri[j], best) && any_hit) return true;
    }
    return false;
}

// include/tdgp.h, THE WALK.  Conservative: every cell within `slack` of the ray's part inside the window is visited until the entry of the
// next slab lies beyond the running minimum.  Returns true when any_hit and a triangle was accepted.
__device__ __forceinline__ bool mr_walk(const MrMesh& m, const MrGrid& g, const MrLists& l, const MrRay& r, const double (&o)[3], const double (&d)[3],
                                        double t_min, double t_max, bool any_hit, MrBest& best, int& count) {
    if (l.P <= 0) return false;
    if ((int64_t)g.n[0] * g.n[1] * g.n[2] == 1) return mr_list(m, l, r, t_min, t_max, 0, any_hit, best, count);
    const double cell = g.cell;
    // the grid in the ray's axes: index 2 is the major axis
    const int k[3] = {r.kx, r.ky, r.kz};
    double a[3], dd[3], top[3];
    int n[3];
    int64_t stride[3];
    double mag = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double lo = mr_sel(g.lo[0], g.lo[1], g.lo[2], k[c]), oc = mr_sel(o[0], o[1], o[2], k[c]);
        n[c] = mr_sel(g.n[0], g.n[1], g.n[2], k[c]);
        stride[c] = mr_sel((int64_t)1, (int64_t)g.n[0], (int64_t)g.n[0] * g.n[1], k[c]);
        dd[c] = mr_sel(d[0], d[1], d[2], k[c]);
        a[c] = oc - lo;
        top[c] = (double)n[c] * cell;
        mag = mag + ((fabs(oc) + fabs(lo)) + top[c]);
    }
    const double slack = mag * 0x1p-48;
    double t0 = t_min, t1 = t_max;
#pragma unroll
    for (int c = 0; c < 3; c++) {                                      // the window inside the box, the box grown by the slack
        const double p0 = -slack, p1 = top[c] + slack;
        if (dd[c] == 0.0) {
            if (!(a[c] >= p0 && a[c] <= p1)) return false;
        } else {
            const double ta = (p0 - a[c]) / dd[c], tb = (p1 - a[c]) / dd[c];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        }
    }
    if (!(t0 <= t1)) return false;
    const bool up = dd[2] > 0.0;
    const double z0 = a[2] + t0 * dd[2], z1 = a[2] + t1 * dd[2];
    int s = mr_cell(up ? z0 - slack : z0 + slack, cell, n[2]);
    const int last = mr_cell(up ? z1 + slack : z1 - slack, cell, n[2]);
    for (int it = 0; it < n[2] && s >= 0 && s < n[2]; it++) {         // at most n slabs: the loop cannot run on
        const double ta = (((double)s * cell - slack) - a[2]) * r.Sz, tb = (((double)(s + 1) * cell + slack) - a[2]) * r.Sz;
        const double te = fmax(fmin(ta, tb), t0), tx = fmin(fmax(ta, tb), t1);
        if (te > best.t) break;                                        // nothing from this slab on can come before the running minimum
        if (te <= tx) {
            const double xa = a[0] + te * dd[0], xb = a[0] + tx * dd[0], ya = a[1] + te * dd[1], yb = a[1] + tx * dd[1];
            const int x0 = mr_cell(fmin(xa, xb) - slack, cell, n[0]), x1 = mr_cell(fmax(xa, xb) + slack, cell, n[0]);
            const int y0 = mr_cell(fmin(ya, yb) - slack, cell, n[1]), y1 = mr_cell(fmax(ya, yb) + slack, cell, n[1]);
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++)
                    if (mr_list(m, l, r, t_min, t_max, (int64_t)s * stride[2] + (int64_t)y * stride[1] + (int64_t)x * stride[0], any_hit, best, count)) return true;
        }
        if (s == last) break;
        s += up ? 1 : -1;
    }
    return false;
}

__device__ __forceinline__ bool mr_scan(const MrMesh& m, const uint8_t* __restrict__ valid, const MrRay& r, double t_min, double t_max, bool any_hit, MrBest& best,
                                        int& count) {
    for (int64_t t = 0; t < m.T; t++) {
        if (!valid[t]) continue;
        count++;
        if (mr_try(m, r, t_min, t_max, t, best) && any_hit) return true;
    }
    return false;
}

__global__ __launch_bounds__(MR_BLOCK) void cast_kernel(const float* __restrict__ origins, const float* __restrict__ directions, int64_t N, double t_min, double t_max,
                                                        MrMesh m, const uint8_t* __restrict__ valid, MrGrid g, MrLists l, int brute_force, int any_hit,
                                                        double* __restrict__ t_out, float* __restrict__ depth, int32_t* __restrict__ triangle, float* __restrict__ bary,
                                                        int8_t* __restrict__ side, uint8_t* __restrict__ hit, int32_t* __restrict__ evals) {
    const int64_t i = blockIdx.x * (int64_t)MR_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float nanf_ = __builtin_nanf("");
    float fo[3], fd[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        fo[c] = origins[i * 3 + c];
        fd[c] = directions[i * 3 + c];
        ok = ok && mr_finite(fo[c]) && mr_finite(fd[c]);
    }
    ok = ok && !(fd[0] == 0.f && fd[1] == 0.f && fd[2] == 0.f);
    MrBest best = {(double)__builtin_inff(), INT32_MAX};
    int count = 0;
    bool found = false;
    MrRay r;
    if (ok) {
        const double o[3] = {(double)fo[0], (double)fo[1], (double)fo[2]}, d[3] = {(double)fd[0], (double)fd[1], (double)fd[2]};
        mr_setup(o, d, r);
        found = brute_force ? mr_scan(m, valid, r, t_min, t_max, any_hit != 0, best, count) : mr_walk(m, g, l, r, o, d, t_min, t_max, any_hit != 0, best, count);
    }
    if (evals) evals[i] = count;
    if (any_hit) {
        hit[i] = found ? 1 : 0;
        return;
    }
    float f[3][3];
    if (!ok || best.tri == INT32_MAX || !mr_load(m, best.tri, f)) {    // a bad ray: NaN; a miss: +inf
        t_out[i] = ok ? (double)__builtin_inff() : (double)nanf_;
        depth[i] = ok ? __builtin_inff() : nanf_;
        triangle[i] = -1;
        bary[i * 2 + 0] = nanf_;
        bary[i * 2 + 1] = nanf_;
        side[i] = 0;
        return;
    }
    MrHit h;
    mr_test(r, f, t_min, t_max, h);                                    // the winner once more: the same bits
    t_out[i] = h.t;
    depth[i] = (float)h.t;
    triangle[i] = best.tri;
    bary[i * 2 + 0] = (float)(h.V / h.det);
    bary[i * 2 + 1] = (float)(h.W / h.det);
    side[i] = h.det > 0.0 ? 1 : -1;
}

// one lane per (point, direction); R lanes of a wave share a point
__global__ __launch_bounds__(MR_BLOCK) void ao_kernel(const float* __restrict__ points, const float* __restrict__ normals, int64_t N, const float* __restrict__ tables,
                                                      int log2K, int R, double bias, double radius, MrMesh m, MrGrid g, MrLists l, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const int64_t lane_id = blockIdx.x * (int64_t)MR_BLOCK + lane;
    const int64_t i = lane_id / R;
    const int k = (int)(lane_id - i * R);
    const bool live = i < N;
    bool ok = live, open = false;
    if (live) {
        float fp[3], fn[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            fp[c] = points[i * 3 + c];
            fn[c] = normals[i * 3 + c];
            ok = ok && mr_finite(fp[c]) && mr_finite(fn[c]);
        }
        ok = ok && !(fn[0] == 0.f && fn[1] == 0.f && fn[2] == 0.f);
        if (ok) {
            const uint32_t table = log2K == 0 ? 0u : ((uint32_t)i * 2654435761u) >> (32 - log2K);
            const float* w = tables + ((int64_t)table * R + k) * 3;
            const double wx = (double)w[0], wy = (double)w[1], wz = (double)w[2];
            const double n0 = (double)fn[0], n1 = (double)fn[1], n2 = (double)fn[2];
            const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            const double nx = n0 / len, ny = n1 / len, nz = n2 / len;
            const double sg = nz >= 0.0 ? 1.0 : -1.0;                   // Duff et al. (2017): no branch on the frame itself
            const double a = -1.0 / (sg + nz);
            const double b = (nx * ny) * a;
            const double T[3] = {1.0 + ((sg * nx) * nx) * a, sg * b, (-sg) * nx};
            const double B[3] = {b, sg + (ny * ny) * a, -ny};
            const double Nn[3] = {nx, ny, nz};
            double o[3], d[3];
            bool fine = true;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                d[c] = (wx * T[c] + wy * B[c]) + wz * Nn[c];
                o[c] = (double)fp[c] + bias * Nn[c];
                fine = fine && mr_finite(d[c]) && mr_finite(o[c]);
            }
            fine = fine && !(d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0);
            open = true;
            if (fine) {                                                // (a direction that is not a ray occludes nothing)
                MrRay r;
                MrBest best = {(double)__builtin_inff(), INT32_MAX};
                int count = 0;
                mr_setup(o, d, r);
                open = !mr_walk(m, g, l, r, o, d, 0.0, radius, true, best, count);
            }
        }
    }
    const unsigned long long mask = __ballot(open);                    // all 64 lanes arrive here
    if (live && k == 0) {
        const int base = lane - lane % R;                              // R divides 64: a point's lanes never straddle a wave
        const unsigned long long group = R == 64 ? ~0ull : ((1ull << R) - 1ull);
        const int free_ = __popcll((mask >> base) & group);
        out[i] = ok ? (float)free_ / (float)R : __builtin_nanf("");
    }
}

int mr_grid_args(const char* who, const float* lo, float cell, const int* dims, MrGrid& g) {
    TDGP_CHECK(lo && dims, TDGP_EINVAL, "%s: null pointer", who);
    TDGP_CHECK(cell > 0.f, TDGP_EINVAL, "%s: cell must be greater than 0 (got %g)", who, (double)cell);
    int64_t cells = 1;
    for (int k = 0; k < 3; k++) {
        TDGP_CHECK(lo[k] - lo[k] == 0.f, TDGP_EINVAL, "%s: the box must be finite", who);
        TDGP_CHECK(dims[k] >= 1 && (int64_t)dims[k] <= MR_CELLS_MAX, TDGP_EINVAL, "%s: every grid dimension must lie in [1, 2^24] (got %d)", who, dims[k]);
        g.lo[k] = (double)lo[k];
        g.n[k] = dims[k];
        cells *= dims[k];
        TDGP_CHECK(cells <= MR_CELLS_MAX, TDGP_EINVAL, "%s: the grid has more than 2^24 cells", who);
    }
    TDGP_CHECK(cells == 1 || cell - cell == 0.f, TDGP_EINVAL, "%s: a grid of more than one cell needs a finite cell", who);
    g.cell = (double)cell;
    return 0;
}

#define MR_SIZE_CHECK(who, name, x) TDGP_CHECK((x) >= 0 && (x) <= MR_N_MAX, TDGP_EINVAL, "%s: need 0 <= %s <= 2^31 - 1 (got %lld)", who, name, (long long)(x))

}  // namespace

TDGP_API int tdgp_mesh_rays_cast(const float* origins, const float* directions, int64_t N, double t_min, double t_max, const float* vertices, const int32_t* triangles,
                                 int64_t T, int64_t V, const uint8_t* valid, const float* lo, float cell, const int* dims, const int32_t* cell_start,
                                 const int32_t* pair_triangle, int64_t P, int brute_force, int any_hit, double* t, float* depth, int32_t* triangle, float* bary,
                                 int8_t* side, uint8_t* hit, int32_t* evaluated, tdgp_stream_t stream) {
    MR_SIZE_CHECK("mesh_rays_cast", "N", N);
    MR_SIZE_CHECK("mesh_rays_cast", "T", T);
    MR_SIZE_CHECK("mesh_rays_cast", "V", V);
    MR_SIZE_CHECK("mesh_rays_cast", "P", P);
    TDGP_CHECK(brute_force == 0 || brute_force == 1, TDGP_EINVAL, "mesh_rays_cast: brute_force must be 0 or 1");
    TDGP_CHECK(any_hit == 0 || any_hit == 1, TDGP_EINVAL, "mesh_rays_cast: any_hit must be 0 or 1");
    TDGP_CHECK(t_min - t_min == 0.0 && t_max == t_max && t_min <= t_max, TDGP_EINVAL, "mesh_rays_cast: need a finite t_min <= t_max (got %g, %g)", t_min, t_max);
    MrGrid g;
    if (int rc = mr_grid_args("mesh_rays_cast", lo, cell, dims, g)) return rc;
    if (N == 0) return 0;
    TDGP_CHECK(origins && directions, TDGP_EINVAL, "mesh_rays_cast: null pointer");
    TDGP_CHECK(any_hit ? hit != nullptr : (t && depth && triangle && bary && side), TDGP_EINVAL, "mesh_rays_cast: null pointer");
    TDGP_CHECK(T == 0 || (triangles && valid && (vertices || V == 0)), TDGP_EINVAL, "mesh_rays_cast: null pointer");
    TDGP_CHECK(brute_force || P == 0 || (cell_start && pair_triangle), TDGP_EINVAL, "mesh_rays_cast: null pointer");
    const MrMesh m = {vertices, triangles, T, V};
    const MrLists l = {cell_start, pair_triangle, P};
    TDGP_LAUNCH("mr_cast_kernel", cast_kernel, dim3((unsigned)cdiv64(N, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, origins, directions, N, t_min, t_max, m, valid,
                g, l, brute_force, any_hit, t, depth, triangle, bary, side, hit, evaluated);
    TDGP_LAUNCH_CHECK();
    return 0;
}

TDGP_API int tdgp_mesh_rays_ao(const float* points, const float* normals, int64_t N, const float* tables, int K, int R, float bias, float radius, const float* vertices,
                               const int32_t* triangles, int64_t T, int64_t V, const float* lo, float cell, const int* dims, const int32_t* cell_start,
                               const int32_t* pair_triangle, int64_t P, float* occlusion, tdgp_stream_t stream) {
    MR_SIZE_CHECK("mesh_rays_ao", "N", N);
    MR_SIZE_CHECK("mesh_rays_ao", "T", T);
    MR_SIZE_CHECK("mesh_rays_ao", "V", V);
    MR_SIZE_CHECK("mesh_rays_ao", "P", P);
    TDGP_CHECK(R == 16 || R == 32 || R == 64, TDGP_EINVAL, "mesh_rays_ao: R must be 16, 32 or 64 (got %d)", R);
    TDGP_CHECK(K >= 1 && K <= MR_TABLES_MAX && (K & (K - 1)) == 0, TDGP_EINVAL, "mesh_rays_ao: K must be a power of two in [1, 64] (got %d)", K);
    TDGP_CHECK(bias >= 0.f && bias - bias == 0.f, TDGP_EINVAL, "mesh_rays_ao: bias must be finite and not negative (got %g)", (double)bias);
    TDGP_CHECK(radius > 0.f, TDGP_EINVAL, "mesh_rays_ao: radius must be greater than 0 (got %g)", (double)radius);
    MrGrid g;
    if (int rc = mr_grid_args("mesh_rays_ao", lo, cell, dims, g)) return rc;
    if (N == 0) return 0;
    TDGP_CHECK(points && normals && tables && occlusion, TDGP_EINVAL, "mesh_rays_ao: null pointer");
    TDGP_CHECK(P == 0 || (triangles && cell_start && pair_triangle && (vertices || V == 0)), TDGP_EINVAL, "mesh_rays_ao: null pointer");
    int log2K = 0;
    while ((1 << log2K) < K) log2K++;
    const MrMesh m = {vertices, triangles, T, V};
    const MrLists l = {cell_start, pair_triangle, P};
    TDGP_LAUNCH("mr_ao_kernel", ao_kernel, dim3((unsigned)cdiv64(N * R, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, points, normals, N, tables, log2K, R,
                (double)bias, (double)radius, m, g, l, occlusion);
    TDGP_LAUNCH_CHECK();
    return 0;
}

// mesh_simplify.hip -- vertex clustering on a uniform grid with each cluster's representative placed by its error quadric (Rossignac-Borrel
// 1993; Lindstrom 2000), for the indexed mesh marching cubes leaves on the device (contract in include/tdgp.h).
//
// Replaces (host / third-party for the reference's users): trimesh / MeshLab decimation on a host copy of the mesh that
// scripts/extract_geometry.py builds.  Nothing here has a counterpart inside the reference itself.
//
//   cluster_keys_kernel       one lane per vertex (three 4-byte loads of one 12-byte record): its cell as one int64 key, -1 outside the lattice
//   [the caller sorts the keys, stable: grouping is plumbing]
//   ci_sums_kernel -> sp_scan_kernel -> ci_apply_kernel   heads of the runs of equal keys, their ranks by scan (device_scan.h): dense ids in
//                             ascending key, start and key per cluster, cluster per vertex -- no atomics
//   tri_relabel_kernel        one lane per triangle: its clusters, and the triple rotated to its smallest index first (or -1 when it collapses)
//   [the caller sorts the rotated triples, stable]
//   tri_keep_kernel           one lane per sorted position: a surviving triangle is kept unless its predecessor holds the same triple
//   tk_sums_kernel -> sp_scan_kernel -> tri_emit_kernel   count, scan, emit: survivors in input order
//   place_kernel              one lane per cluster: the mean of its members in `order`, the quadric of its corners in corner-table order, a fixed
//                             3x3 Jacobi, the placement -- all sequential in double, every operation rounded once (-ffp-contract=off)
//   attr_kernel               one lane per (cluster, channel): the mean of an attribute over the members
// Neighbouring lanes of place_kernel hold neighbouring cells (ids ascend with the key, x fastest), so their gathers share lines.  No float
// atomics, no kernel waits for another workgroup; the only integer atomics are those of tdgp_mesh_corner_table, which the caller runs on the
// relabelled triangles.
#include "common.h"
#include "device_scan.h"
#include "quadric_solve.h"

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_PLACE_BLOCK = 64;            // one wave per block: 20 000 clusters of a few hundred corners each spread over every CU, not over 80
constexpr int64_t SP_WS_HEAD = 64;            // bytes in front of the block sums: the total as one int64
constexpr int64_t SP_T_MAX = 715827882ll;     // 3 T <= 2^31 - 1
constexpr int64_t SP_V_MAX = (int64_t)INT32_MAX - 1;
constexpr int64_t SP_K_HALF = 1ll << 20;      // cell indices lie in [-2^20, 2^20)
constexpr int SP_K_BITS = 21;

struct Cell3 {
    double cell[3], origin[3];
};

__global__ __launch_bounds__(1024) void sp_scan_kernel(uint32_t* __restrict__ block_sums, int64_t nb, int64_t* __restrict__ total) {
    scan_block_sums<1>(block_sums, nb, total);
}

// ---- cells -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_BLOCK) void cluster_keys_kernel(const float* __restrict__ verts, int64_t V, Cell3 g, int64_t* __restrict__ key) {
    const int64_t v = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    if (v >= V) return;
    int64_t k[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double q = floor(((double)verts[v * 3 + c] - g.origin[c]) / g.cell[c]);
        ok = ok && q >= -(double)SP_K_HALF && q < (double)SP_K_HALF;           // false for NaN
        k[c] = ok ? (int64_t)q + SP_K_HALF : 0;
    }
    key[v] = ok ? (((k[2] << SP_K_BITS) + k[1]) << SP_K_BITS) + k[0] : -1;      // (kz * 2^21 + ky) * 2^21 + kx of the biased indices: < 2^63
}

__device__ __forceinline__ int ci_head(const int64_t* __restrict__ skey, int64_t i, int64_t V) {
    if (i >= V) return 0;
    const int64_t k = skey[i];
    return (k >= 0 && (i == 0 || skey[i - 1] != k)) ? 1 : 0;
}

__global__ __launch_bounds__(SP_BLOCK) void ci_sums_kernel(const int64_t* __restrict__ skey, int64_t V, uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t i = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<SP_BLOCK>(ci_head(skey, i, V), sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(SP_BLOCK) void ci_apply_kernel(const int64_t* __restrict__ skey, const int32_t* __restrict__ order, int64_t V,
                                                            const uint32_t* __restrict__ block_offs, int32_t* __restrict__ cluster,
                                                            int32_t* __restrict__ start, int64_t* __restrict__ ckey) {
    __shared__ int sm[4];
    const int64_t i = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    const int head = ci_head(skey, i, V);
    int total;
    const int64_t before = (int64_t)block_offs[blockIdx.x] + block_excl_scan<SP_BLOCK>(head, sm, total);
    if (i >= V) return;
    const int64_t k = skey[i];
    const int64_t id = before + head - 1;          // the run this position lies in; -1 in front of the first head (keys of -1 sort first)
    if (head) {
        start[id] = (int32_t)i;
        ckey[id] = k;
    }
    const int v = order[i];
    if (v >= 0 && v < V) cluster[v] = k >= 0 ? (int32_t)id : -1;
    if (i == V - 1) start[before + head] = (int32_t)V;
}

// ---- triangles ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_BLOCK) void tri_relabel_kernel(const int32_t* __restrict__ tris, int64_t T, int64_t V, const int32_t* __restrict__ cluster,
                                                               int32_t* __restrict__ ct, int32_t* __restrict__ canon) {
    const int64_t t = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    if (t >= T) return;
    int c[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int v = tris[t * 3 + i];
        c[i] = (v >= 0 && v < V) ? cluster[v] : -1;              // an index outside [0, V) is never dereferenced
        c[i] = c[i] < 0 ? -1 : c[i];
    }
    const bool in_range = tris[t * 3] >= 0 && tris[t * 3] < V && tris[t * 3 + 1] >= 0 && tris[t * 3 + 1] < V && tris[t * 3 + 2] >= 0 && tris[t * 3 + 2] < V;
#pragma unroll
    for (int i = 0; i < 3; i++) ct[t * 3 + i] = in_range ? c[i] : -1;        // a skipped triangle names no cluster at all
    const bool live = in_range && c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
    int r[3] = {-1, -1, -1};
    if (live) {
        const int s = (c[0] < c[1] && c[0] < c[2]) ? 0 : (c[1] < c[2] ? 1 : 2);
        r[0] = c[s];
        r[1] = c[(s + 1) % 3];
        r[2] = c[(s + 2) % 3];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) canon[t * 3 + i] = r[i];
}

__global__ __launch_bounds__(SP_BLOCK) void tri_keep_kernel(const int32_t* __restrict__ canon, const int32_t* __restrict__ perm, int64_t T,
                                                            uint8_t* __restrict__ keep) {
    const int64_t i = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    if (i >= T) return;
    const int64_t t = perm ? (int64_t)perm[i] : i;
    if (t < 0 || t >= T) return;
    const int a = canon[t * 3 + 0], b = canon[t * 3 + 1], c = canon[t * 3 + 2];
    if (a < 0) return;                                           // collapsed or dropped: keep[t] stays 0
    bool dup = false;
    if (perm && i > 0) {
        const int64_t p = perm[i - 1];
        dup = p >= 0 && p < T && canon[p * 3 + 0] == a && canon[p * 3 + 1] == b && canon[p * 3 + 2] == c;
    }
    keep[t] = dup ? 0 : 1;
}

__global__ __launch_bounds__(SP_BLOCK) void tk_sums_kernel(const uint8_t* __restrict__ keep, int64_t T, uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t t = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<SP_BLOCK>(t < T && keep[t] != 0 ? 1 : 0, sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(SP_BLOCK) void tri_emit_kernel(const int32_t* __restrict__ ct, int64_t T, const uint8_t* __restrict__ keep,
                                                            const uint32_t* __restrict__ block_offs, int32_t* __restrict__ out, int64_t T_out,
                                                            int32_t* __restrict__ tri_map) {
    __shared__ int sm[4];
    const int64_t t = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    const int k = t < T && keep[t] != 0 ? 1 : 0;
    int total;
    const int64_t pos = (int64_t)block_offs[blockIdx.x] + block_excl_scan<SP_BLOCK>(k, sm, total);
    if (!k || pos >= T_out) return;
#pragma unroll
    for (int i = 0; i < 3; i++) out[pos * 3 + i] = ct[t * 3 + i];
    tri_map[pos] = (int32_t)t;
}

// ---- placement ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_PLACE_BLOCK) void place_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ start, const int64_t* __restrict__ ckey, int64_t C, Cell3 g,
                                                         const int32_t* __restrict__ tris, int64_t T, const int32_t* __restrict__ cstart,
                                                         const int32_t* __restrict__ ccorner, int quadric, double rank_tol,
                                                         float* __restrict__ out) {
    const int64_t cl = blockIdx.x * (int64_t)SP_PLACE_BLOCK + threadIdx.x;
    if (cl >= C) return;
    const int64_t key = ckey[cl];
    const int64_t mask = (1ll << SP_K_BITS) - 1;
    double centre[3];
    {
        const int64_t k[3] = {(key & mask) - SP_K_HALF, ((key >> SP_K_BITS) & mask) - SP_K_HALF, ((key >> (2 * SP_K_BITS)) & mask) - SP_K_HALF};
#pragma unroll
        for (int c = 0; c < 3; c++) centre[c] = g.origin[c] + ((double)k[c] + 0.5) * g.cell[c];
    }
    // the mean of the members, in `order`
    int64_t s0 = start[cl], e0 = start[cl + 1];
    s0 = s0 < 0 ? 0 : (s0 > V ? V : s0);
    e0 = e0 < s0 ? s0 : (e0 > V ? V : e0);
    double m[3] = {0.0, 0.0, 0.0};
    int64_t members = 0;
    for (int64_t j = s0; j < e0; j++) {
        const int v = order[j];
        if (v < 0 || v >= V) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) m[c] = m[c] + ((double)verts[(int64_t)v * 3 + c] - centre[c]);
        members++;
    }
    if (members > 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) m[c] = m[c] / (double)members;
    }
    double x[3] = {m[0], m[1], m[2]};
    if (quadric) {
        int64_t n = cstart[C];
        n = n < 0 ? 0 : (n > 3 * T ? 3 * T : n);
        int64_t cs = cstart[cl], ce = cstart[cl + 1];
        cs = cs < 0 ? 0 : (cs > n ? n : cs);
        ce = ce < cs ? cs : (ce > n ? n : ce);
        double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        double bv[3] = {0.0, 0.0, 0.0};
        int64_t corners = 0;
        for (int64_t j = cs; j < ce; j++) {
            const int cid = ccorner[j];
            if (cid < 0 || cid >= 3 * T) continue;
            const int64_t t = cid / 3;
            const int i0 = tris[t * 3 + 0], i1 = tris[t * 3 + 1], i2 = tris[t * 3 + 2];
            if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) continue;
            double a[3], e1[3], e2[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                a[c] = (double)verts[(int64_t)i0 * 3 + c] - centre[c];
                e1[c] = ((double)verts[(int64_t)i1 * 3 + c] - centre[c]) - a[c];
                e2[c] = ((double)verts[(int64_t)i2 * 3 + c] - centre[c]) - a[c];
            }
            const double nn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double d = -((nn[0] * a[0] + nn[1] * a[1]) + nn[2] * a[2]);
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = r; c < 3; c++) A[r][c] = A[r][c] + nn[r] * nn[c];
                bv[r] = bv[r] + nn[r] * d;
            }
            corners++;
        }
        if (corners > 0) {
            A[1][0] = A[0][1];
            A[2][0] = A[0][2];
            A[2][1] = A[1][2];
            quadric_minimise(A, bv, m, rank_tol, x);         // quadric_solve.h: the Jacobi mesh_decimate.hip shares
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double half = g.cell[c] * 0.5;
                ok = ok && x[c] >= -half && x[c] <= half;        // false for NaN; +-inf lies outside
            }
            if (!ok) {                                           // Lindstrom's fallback
#pragma unroll
                for (int c = 0; c < 3; c++) x[c] = m[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out[cl * 3 + c] = (float)(centre[c] + x[c]);
}

__global__ __launch_bounds__(SP_BLOCK) void attr_kernel(const float* __restrict__ attr, int channels, int64_t V, const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ start, int64_t C, float* __restrict__ out) {
    const int64_t e = blockIdx.x * (int64_t)SP_BLOCK + threadIdx.x;
    if (e >= C * channels) return;
    const int64_t cl = e / channels;
    const int ch = (int)(e - cl * channels);
    int64_t s0 = start[cl], e0 = start[cl + 1];
    s0 = s0 < 0 ? 0 : (s0 > V ? V : s0);
    e0 = e0 < s0 ? s0 : (e0 > V ? V : e0);
    double s = 0.0;
    int64_t members = 0;
    for (int64_t j = s0; j < e0; j++) {
        const int v = order[j];
        if (v < 0 || v >= V) continue;
        s = s + (double)attr[(int64_t)v * channels + ch];
        members++;
    }
    out[e] = members > 0 ? (float)(s / (double)members) : 0.0f;
}

inline unsigned sp_blocks(int64_t n) { return (unsigned)cdiv64(n, SP_BLOCK); }
inline int64_t sp_ws_bytes(int64_t n) { return align64(SP_WS_HEAD + cdiv64(n, SP_BLOCK) * 4); }
inline bool sp_finite(double x) { return x == x && x > -(double)__builtin_inff() && x < (double)__builtin_inff(); }

inline bool sp_cell(const double* cell, const double* origin, Cell3& g) {
    if (!cell || !origin) return false;
    for (int c = 0; c < 3; c++) {
        if (!(sp_finite(cell[c]) && cell[c] > 0.0 && sp_finite(origin[c]))) return false;
        g.cell[c] = cell[c];
        g.origin[c] = origin[c];
    }
    return true;
}

inline int sp_clear_total(void* workspace, hipStream_t s, const char* who) {
    if (hipMemsetAsync(workspace, 0, sizeof(int64_t), s) != hipSuccess) {
        tdgp_set_error("%s: clearing the total failed", who);
        return TDGP_ELAUNCH;
    }
    return TDGP_OK;
}

}  // namespace

#define SP_WS_CHECK(name, n)                                                                                                                   \
    TDGP_CHECK(workspace, TDGP_EINVAL, name ": null workspace");                                                                               \
    TDGP_CHECK(((uintptr_t)workspace & 15) == 0, TDGP_EINVAL, name ": workspace must be 16-byte aligned");                                     \
    TDGP_CHECK(workspace_bytes >= sp_ws_bytes(n), TDGP_EWORKSPACE, name ": workspace of %lld bytes, %lld needed", (long long)workspace_bytes, \
               (long long)sp_ws_bytes(n))

TDGP_API int tdgp_mesh_cluster_keys(const float* vertices, int64_t V, const double* cell, const double* origin, int64_t* key, tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= SP_V_MAX, TDGP_EINVAL, "mesh_cluster_keys: need 0 <= V <= 2^31 - 2 (got %lld)", (long long)V);
    Cell3 g;
    TDGP_CHECK(sp_cell(cell, origin, g), TDGP_EINVAL, "mesh_cluster_keys: cell must be three positive finite doubles and origin three finite ones");
    if (V == 0) return TDGP_OK;
    TDGP_CHECK(vertices && key, TDGP_EINVAL, "mesh_cluster_keys: null pointer");
    TDGP_LAUNCH("cluster_keys_kernel", cluster_keys_kernel, dim3(sp_blocks(V)), dim3(SP_BLOCK), 0, (hipStream_t)stream, vertices, V, g, key);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_mesh_cluster_ids_workspace_bytes(int64_t V) {
    if (V < 0 || V > SP_V_MAX) return -1;
    return sp_ws_bytes(V);
}

TDGP_API int tdgp_mesh_cluster_ids(const int64_t* sorted_key, const int32_t* order, int64_t V, int32_t* cluster, int32_t* start, int64_t* cluster_key,
                                   void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= SP_V_MAX, TDGP_EINVAL, "mesh_cluster_ids: need 0 <= V <= 2^31 - 2 (got %lld)", (long long)V);
    SP_WS_CHECK("mesh_cluster_ids", V);
    TDGP_CHECK(start, TDGP_EINVAL, "mesh_cluster_ids: null pointer");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (V == 0) {                                 // no vertex, no cluster: start[0] = total = 0
        if (hipMemsetAsync(start, 0, sizeof(int32_t), s) != hipSuccess) {
            tdgp_set_error("mesh_cluster_ids: clearing start failed");
            return TDGP_ELAUNCH;
        }
        return sp_clear_total(workspace, s, "mesh_cluster_ids");
    }
    TDGP_CHECK(sorted_key && order && cluster && cluster_key, TDGP_EINVAL, "mesh_cluster_ids: null pointer");
    if (hipMemsetAsync(cluster, 0xff, (size_t)V * sizeof(int32_t), s) != hipSuccess) {      // a vertex `order` does not name belongs to no cluster
        tdgp_set_error("mesh_cluster_ids: clearing the cluster ids failed");
        return TDGP_ELAUNCH;
    }
    uint32_t* sums = (uint32_t*)(ws + SP_WS_HEAD);
    const int64_t nb = cdiv64(V, SP_BLOCK);
    TDGP_LAUNCH("ci_sums_kernel", ci_sums_kernel, dim3((unsigned)nb), dim3(SP_BLOCK), 0, s, sorted_key, V, sums);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("sp_scan_kernel", sp_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, (int64_t*)ws);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("ci_apply_kernel", ci_apply_kernel, dim3((unsigned)nb), dim3(SP_BLOCK), 0, s, sorted_key, order, V, (const uint32_t*)sums, cluster, start, cluster_key);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

#define SP_TV_CHECK(name)                                                                                                                       \
    TDGP_CHECK(T >= 0 && T <= SP_T_MAX && V >= 0 && V <= SP_V_MAX, TDGP_EINVAL, name ": need 0 <= 3 T <= 2^31 - 1 and 0 <= V <= 2^31 - 2 (got T = %lld, V = %lld)", \
               (long long)T, (long long)V)

TDGP_API int tdgp_mesh_cluster_triangles_relabel(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster, int32_t* cluster_triangles,
                                                 int32_t* rotated, tdgp_stream_t stream) {
    SP_TV_CHECK("mesh_cluster_triangles_relabel");
    if (T == 0) return TDGP_OK;
    TDGP_CHECK(triangles && cluster_triangles && rotated && (V == 0 || cluster), TDGP_EINVAL, "mesh_cluster_triangles_relabel: null pointer");
    TDGP_LAUNCH("tri_relabel_kernel", tri_relabel_kernel, dim3(sp_blocks(T)), dim3(SP_BLOCK), 0, (hipStream_t)stream, triangles, T, V, cluster, cluster_triangles, rotated);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_mesh_cluster_triangles_workspace_bytes(int64_t T) {
    if (T < 0 || T > SP_T_MAX) return -1;
    return sp_ws_bytes(T);
}

TDGP_API int tdgp_mesh_cluster_triangles_count(const int32_t* rotated, const int32_t* perm, int64_t T, uint8_t* keep, void* workspace, int64_t workspace_bytes,
                                               tdgp_stream_t stream) {
    TDGP_CHECK(T >= 0 && T <= SP_T_MAX, TDGP_EINVAL, "mesh_cluster_triangles_count: need 0 <= 3 T <= 2^31 - 1 (got T = %lld)", (long long)T);
    SP_WS_CHECK("mesh_cluster_triangles_count", T);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (T == 0) return sp_clear_total(workspace, s, "mesh_cluster_triangles_count");
    TDGP_CHECK(rotated && keep, TDGP_EINVAL, "mesh_cluster_triangles_count: null pointer");
    if (hipMemsetAsync(keep, 0, (size_t)T, s) != hipSuccess) {
        tdgp_set_error("mesh_cluster_triangles_count: clearing the flags failed");
        return TDGP_ELAUNCH;
    }
    uint32_t* sums = (uint32_t*)(ws + SP_WS_HEAD);
    const int64_t nb = cdiv64(T, SP_BLOCK);
    TDGP_LAUNCH("tri_keep_kernel", tri_keep_kernel, dim3((unsigned)nb), dim3(SP_BLOCK), 0, s, rotated, perm, T, keep);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("tk_sums_kernel", tk_sums_kernel, dim3((unsigned)nb), dim3(SP_BLOCK), 0, s, (const uint8_t*)keep, T, sums);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("sp_scan_kernel", sp_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, (int64_t*)ws);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_cluster_triangles_emit(const int32_t* cluster_triangles, int64_t T, const uint8_t* keep, void* workspace, int64_t workspace_bytes,
                                              int32_t* out_triangles, int64_t T_out, int32_t* triangle_map, tdgp_stream_t stream) {
    TDGP_CHECK(T >= 0 && T <= SP_T_MAX && T_out >= 0 && T_out <= T, TDGP_EINVAL, "mesh_cluster_triangles_emit: need 0 <= T_out <= T, 3 T <= 2^31 - 1 (got T = %lld, T_out = %lld)",
               (long long)T, (long long)T_out);
    SP_WS_CHECK("mesh_cluster_triangles_emit", T);
    if (T == 0 || T_out == 0) return TDGP_OK;
    TDGP_CHECK(cluster_triangles && keep && out_triangles && triangle_map, TDGP_EINVAL, "mesh_cluster_triangles_emit: null pointer");
    const uint32_t* sums = (const uint32_t*)((char*)workspace + SP_WS_HEAD);
    TDGP_LAUNCH("tri_emit_kernel", tri_emit_kernel, dim3(sp_blocks(T)), dim3(SP_BLOCK), 0, (hipStream_t)stream, cluster_triangles, T, keep, sums, out_triangles, T_out,
                triangle_map);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_cluster_place(const float* vertices, int64_t V, const int32_t* order, const int32_t* start, const int64_t* cluster_key, int64_t C,
                                     const double* cell, const double* origin, const int32_t* triangles, int64_t T, const int32_t* corner_start,
                                     const int32_t* corner, int placement, double rank_tol, float* out_vertices, tdgp_stream_t stream) {
    SP_TV_CHECK("mesh_cluster_place");
    TDGP_CHECK(C >= 0 && C <= V, TDGP_EINVAL, "mesh_cluster_place: need 0 <= C <= V (got C = %lld, V = %lld)", (long long)C, (long long)V);
    TDGP_CHECK(placement == 0 || placement == 1, TDGP_EINVAL, "mesh_cluster_place: placement must be 0 (mean) or 1 (quadric), got %d", placement);
    TDGP_CHECK(sp_finite(rank_tol) && rank_tol >= 0.0, TDGP_EINVAL, "mesh_cluster_place: rank_tol must be finite and not negative");
    Cell3 g;
    TDGP_CHECK(sp_cell(cell, origin, g), TDGP_EINVAL, "mesh_cluster_place: cell must be three positive finite doubles and origin three finite ones");
    if (C == 0) return TDGP_OK;
    TDGP_CHECK(vertices && order && start && cluster_key && out_vertices, TDGP_EINVAL, "mesh_cluster_place: null pointer");
    TDGP_CHECK(placement == 0 || (corner_start && (T == 0 || (triangles && corner))), TDGP_EINVAL, "mesh_cluster_place: the quadric placement needs the triangles and their corner table");
    TDGP_LAUNCH("place_kernel", place_kernel, dim3((unsigned)cdiv64(C, SP_PLACE_BLOCK)), dim3(SP_PLACE_BLOCK), 0, (hipStream_t)stream, vertices, V, order, start, cluster_key, C, g, triangles, T,
                corner_start, corner, placement, rank_tol, out_vertices);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_cluster_attribute(const float* attribute, int channels, int64_t V, const int32_t* order, const int32_t* start, int64_t C, float* out,
                                         tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= SP_V_MAX && C >= 0 && C <= V, TDGP_EINVAL, "mesh_cluster_attribute: need 0 <= C <= V <= 2^31 - 2 (got C = %lld, V = %lld)", (long long)C,
               (long long)V);
    TDGP_CHECK(channels >= 1 && channels <= 64, TDGP_EINVAL, "mesh_cluster_attribute: channels must lie in [1, 64], got %d", channels);
    if (C == 0) return TDGP_OK;
    TDGP_CHECK(attribute && order && start && out, TDGP_EINVAL, "mesh_cluster_attribute: null pointer");
    TDGP_LAUNCH("attr_kernel", attr_kernel, dim3(sp_blocks(C * channels)), dim3(SP_BLOCK), 0, (hipStream_t)stream, attribute, channels, V, order, start, C, out);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

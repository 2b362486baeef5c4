// mesh_surface.hip -- the surface of an indexed triangle mesh on the device: the vertex -> triangle incidence (a corner table), and the three
// gathers over it -- vertex normals, the open rim, one umbrella smoothing step -- plus the per-ray interpolation of vertex normals for mesh
// frames (contract in include/tdgp.h).
//
// Replaces (host / third-party for the reference's users): trimesh / MeshLab smoothing and `vertex_normals` on a host copy of the mesh that
// scripts/extract_geometry.py builds.  Nothing here has a counterpart inside the reference itself.
//
// Corner table: corner 3t + i is slot i of triangle t.
//   ct_count_kernel   one lane per triangle: degree[v] += 1 per corner (integer atomics: a count does not depend on the order)
//   ct_sums_kernel -> ms_scan_kernel -> ct_start_kernel   start = exclusive prefix of degree (device_scan.h: block scan, ONE block over the
//                     block sums, block scan + offset)
//   ct_fill_kernel    one lane per triangle: every corner is dropped into its vertex's range of a SCRATCH list at a slot taken from an atomic
//                     cursor -- the order inside a range is whatever the atomics made it
//   ct_rank_kernel    one lane per scratch entry: its final position is start[v] + the number of entries of its range that are smaller.
//                     Corner ids are distinct, so the ranks are a permutation of the range and the output is the ascending list whatever the
//                     scratch order was: the table is a pure function of `triangles`.  O(degree) reads per corner, O(degree^2) per vertex,
//                     spread over degree lanes: marching-cubes valence is about 6; a vertex of 4096 triangles is 4096 lanes of 4096 reads.
// Gathers: one lane per vertex walks its corners in table order, in double, every operation rounded once (-ffp-contract=off): sequential
// sums, so the outputs are pure functions of the arrays as given (not invariant under a permutation of the triangles).  No float atomics,
// no kernel waits for another workgroup.
#include "common.h"
#include "device_scan.h"
#include "mesh_hit.h"

namespace {

constexpr int MS_BLOCK = 256;                 // elements per block (4 waves)
constexpr int64_t MS_WS_HEAD = 64;            // bytes in front of the block sums: the total as one int64
constexpr int64_t MS_T_MAX = 715827882ll;     // 3 T <= 2^31 - 1
constexpr int RIM_WAVE_DEGREE = 32;           // a vertex of more corners has its rim test spread over its wave

__device__ __forceinline__ bool ms_tri_ok(int a, int b, int c, int64_t V) {
    return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

// one block of 1024 threads: exclusive scan of nb block sums in place, the grand total (<= 3T < 2^31) to *total
__global__ __launch_bounds__(1024) void ms_scan_kernel(uint32_t* __restrict__ block_sums, int64_t nb, int64_t* __restrict__ total) {
    scan_block_sums<1>(block_sums, nb, total);
}

// ---- corner table ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ct_count_kernel(const int32_t* __restrict__ tris, int64_t T, int64_t V, int* degree) {
    const int64_t t = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int a = tris[t * 3 + 0], b = tris[t * 3 + 1], c = tris[t * 3 + 2];
    if (!ms_tri_ok(a, b, c, V)) return;            // an index outside [0, V) skips its triangle and is never dereferenced
    atomicAdd(degree + a, 1);
    atomicAdd(degree + b, 1);
    atomicAdd(degree + c, 1);
}

__global__ __launch_bounds__(MS_BLOCK) void ct_sums_kernel(const int* __restrict__ degree, int64_t V, uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<MS_BLOCK>(v < V ? degree[v] : 0, sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(MS_BLOCK) void ct_start_kernel(const int* __restrict__ degree, int64_t V, const uint32_t* __restrict__ block_offs,
                                                            int32_t* __restrict__ start) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    const int d = v < V ? degree[v] : 0;
    int total;
    const int pos = (int)block_offs[blockIdx.x] + block_excl_scan<MS_BLOCK>(d, sm, total);
    if (v >= V) return;
    start[v] = pos;
    if (v == V - 1) start[V] = pos + d;
}

__global__ __launch_bounds__(MS_BLOCK) void ct_fill_kernel(const int32_t* __restrict__ tris, int64_t T, int64_t V, const int32_t* __restrict__ start,
                                                           int* cursor, int32_t* __restrict__ scratch) {
    const int64_t t = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    if (t >= T) return;
    int idx[3];
#pragma unroll
    for (int i = 0; i < 3; i++) idx[i] = tris[t * 3 + i];
    if (!ms_tri_ok(idx[0], idx[1], idx[2], V)) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int64_t p = (int64_t)start[idx[i]] + atomicAdd(cursor + idx[i], 1);
        if (p >= 0 && p < 3 * T) scratch[p] = (int32_t)(t * 3 + i);          // the counts of the same triangles sized the ranges: always true
    }
}

__global__ __launch_bounds__(MS_BLOCK) void ct_rank_kernel(const int32_t* __restrict__ tris, int64_t T, int64_t V, const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ scratch, const int64_t* __restrict__ total,
                                                           int32_t* __restrict__ corner) {
    const int64_t p = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    const int64_t n = min(*total, 3 * T);
    if (p >= n) return;
    const int c = scratch[p];
    if (c < 0 || c >= 3 * T) return;
    const int v = tris[c];
    if (v < 0 || v >= V) return;
    const int64_t s = start[v], e = min((int64_t)start[v + 1], n);
    if (p < s || p >= e) return;
    int rank = 0;
    for (int64_t j = s; j < e; j++) rank += scratch[j] < c ? 1 : 0;
    corner[s + rank] = c;
}

// ---- gathers -----------------------------------------------------------------------------------------------------------------------------
// the range of vertex v in a table the caller may have built itself: clamped into [0, min(start[V], 3T)], never negative in length
__device__ __forceinline__ void corner_range(const int32_t* __restrict__ start, int64_t v, int64_t V, int64_t T, int64_t& s, int64_t& e) {
    int64_t n = start[V];
    n = n < 0 ? 0 : (n > 3 * T ? 3 * T : n);
    s = start[v];
    e = start[v + 1];
    s = s < 0 ? 0 : (s > n ? n : s);
    e = e < s ? s : (e > n ? n : e);
}

// corner c -> its triangle's three indices and its slot; false for a corner id outside [0, 3T) or a skipped triangle (nothing dereferenced)
__device__ __forceinline__ bool corner_triangle(const int32_t* __restrict__ tris, int64_t T, int64_t V, int c, int (&idx)[3], int& slot) {
    if (c < 0 || c >= 3 * T) return false;
    const int t = c / 3;
    slot = c - 3 * t;
#pragma unroll
    for (int i = 0; i < 3; i++) idx[i] = tris[(int64_t)t * 3 + i];
    return ms_tri_ok(idx[0], idx[1], idx[2], V);
}

__global__ __launch_bounds__(MS_BLOCK) void vertex_normals_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris, int64_t T, int64_t V,
                                                                  const int32_t* __restrict__ start, const int32_t* __restrict__ corner, int weight,
                                                                  float* __restrict__ normal) {
    const int64_t v = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    if (v >= V) return;
    int64_t s0, e0;
    corner_range(start, v, V, T, s0, e0);
    double s[3] = {0.0, 0.0, 0.0};
    const double inf = (double)__builtin_inff();
    for (int64_t j = s0; j < e0; j++) {
        int idx[3], slot;
        if (!corner_triangle(tris, T, V, corner[j], idx, slot)) continue;
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v0 = (double)verts[(int64_t)idx[0] * 3 + c];
            a[c] = (double)verts[(int64_t)idx[1] * 3 + c] - v0;
            b[c] = (double)verts[(int64_t)idx[2] * 3 + c] - v0;
        }
        const double g[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        if (weight == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] = s[c] + g[c];
        } else {
            const double q = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
            if (q > 0.0 && q < inf) {
                const double r = sqrt(q);
#pragma unroll
                for (int c = 0; c < 3; c++) s[c] = s[c] + g[c] / r;
            }
        }
    }
    const double q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (q > 0.0 && q < inf) {
        const double r = sqrt(q);
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = (float)(s[c] / r);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) normal[v * 3 + c] = n[c];
}

// Is the neighbour that candidate q of vertex v names (q >> 1: which of v's corners, q & 1: its next or its previous slot) next to v in
// exactly one of v's triangles?  Counts over all of v's corners: O(degree) per candidate, O(degree^2) per vertex.
__device__ __forceinline__ bool rim_candidate(const int32_t* __restrict__ tris, int64_t T, int64_t V, const int32_t* __restrict__ corner, int64_t s0,
                                              int64_t e0, int v, int64_t q) {
    int idx[3], slot;
    if (!corner_triangle(tris, T, V, corner[s0 + (q >> 1)], idx, slot)) return false;
    const int w = idx[(slot + 1 + (int)(q & 1)) % 3];
    if (w == v) return false;
    int count = 0, last = -1;
    for (int64_t j = s0; j < e0 && count < 2; j++) {
        const int c = corner[j];
        if (!corner_triangle(tris, T, V, c, idx, slot)) continue;
        const int t = c / 3;
        if (t == last) continue;                   // a triangle naming v twice is one triangle
        if (idx[(slot + 1) % 3] == w || idx[(slot + 2) % 3] == w) { count++; last = t; }
    }
    return count == 1;
}

__global__ __launch_bounds__(MS_BLOCK) void boundary_kernel(const int32_t* __restrict__ tris, int64_t T, int64_t V, const int32_t* __restrict__ start,
                                                            const int32_t* __restrict__ corner, uint8_t* __restrict__ rim) {
    const int64_t v = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    int64_t s0 = 0, e0 = 0;
    if (v < V) corner_range(start, v, V, T, s0, e0);
    const bool big = e0 - s0 > RIM_WAVE_DEGREE;
    int found = 0;
    if (!big) {
        for (int64_t q = 0; q < 2 * (e0 - s0) && !found; q++) found = rim_candidate(tris, T, V, corner, s0, e0, (int)v, q) ? 1 : 0;
    }
    // hand-over: every lane of the wave reaches this loop; a vertex of many corners is taken by the whole wave, 64 candidates per step
    unsigned long long mask = __ballot(big);
    const int lane = lane_id();
    while (mask) {
        const int src = __ffsll(mask) - 1;
        mask &= mask - 1;
        const int64_t bs = (int64_t)__shfl((int)s0, src, 64), be = (int64_t)__shfl((int)e0, src, 64);      // both within [0, 3T] < 2^31
        const int bv = __shfl((int)v, src, 64);
        int any = 0;
        for (int64_t q0 = 0; q0 < 2 * (be - bs) && !any; q0 += 64) {
            const int64_t q = q0 + lane;
            const bool hit = q < 2 * (be - bs) && rim_candidate(tris, T, V, corner, bs, be, bv, q);
            any = __ballot(hit) != 0ull ? 1 : 0;
        }
        if (lane == src) found = any;
    }
    if (v < V) rim[v] = (uint8_t)found;
}

__global__ __launch_bounds__(MS_BLOCK) void smooth_step_kernel(const float* __restrict__ vin, const int32_t* __restrict__ tris, int64_t T, int64_t V,
                                                               const int32_t* __restrict__ start, const int32_t* __restrict__ corner, double factor,
                                                               const uint8_t* __restrict__ pinned, float* __restrict__ vout) {
    const int64_t v = blockIdx.x * (int64_t)MS_BLOCK + threadIdx.x;
    if (v >= V) return;
    int64_t s0, e0;
    corner_range(start, v, V, T, s0, e0);
    const float x[3] = {vin[v * 3 + 0], vin[v * 3 + 1], vin[v * 3 + 2]};
    float out[3] = {x[0], x[1], x[2]};
    const int64_t d = e0 - s0;
    if (d > 0 && !(pinned && pinned[v] != 0)) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int64_t j = s0; j < e0; j++) {
            int idx[3], slot;
            if (!corner_triangle(tris, T, V, corner[j], idx, slot)) continue;
            const int n1 = idx[(slot + 1) % 3], n2 = idx[(slot + 2) % 3];
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] = s[c] + (double)vin[(int64_t)n1 * 3 + c];
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] = s[c] + (double)vin[(int64_t)n2 * 3 + c];
        }
        const double den = (double)(2 * d);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double m = s[c] / den;
            out[c] = (float)((double)x[c] + factor * (m - (double)x[c]));
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) vout[v * 3 + c] = out[c];
}

// ---- frames ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void interp_normals_kernel(const int32_t* __restrict__ tri, const int32_t* __restrict__ status, const float* __restrict__ t_hit,
                                                                  const float* __restrict__ ray_o, const float* __restrict__ ray_d, int64_t rays,
                                                                  const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ tris, int64_t T,
                                                                  const float* __restrict__ vnormal, float* __restrict__ normal) {
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= rays || status[ray] != 1) return;
    const int k = tri[ray];
    if (k < 0 || (int64_t)k >= T) return;
    int idx[3];
#pragma unroll
    for (int i = 0; i < 3; i++) idx[i] = tris[(int64_t)k * 3 + i];
    if (!ms_tri_ok(idx[0], idx[1], idx[2], V)) return;
    const float th = t_hit[ray];
    float x[3];
#pragma unroll
    for (int c = 0; c < 3; c++) x[c] = ray_o[ray * 3 + c] + ray_d[ray * 3 + c] * th;
    double a[3], b[3], v0[3], w[3];
    mesh_tri_frame(verts, idx, a, b, v0);
    mesh_bary_weights(a, b, v0, x, w);
    float n[3];
    if (!mesh_vertex_normal(w, idx, vnormal, n)) return;                       // the face normal tdgp_mesh_resolve wrote stays
#pragma unroll
    for (int c = 0; c < 3; c++) normal[ray * 3 + c] = n[c];
}

inline bool ms_sizes_ok(int64_t T, int64_t V) { return T >= 0 && V >= 0 && T <= MS_T_MAX && V <= (int64_t)INT32_MAX - 1; }
inline unsigned ms_blocks(int64_t n) { return (unsigned)cdiv64(n, MS_BLOCK); }

struct TableLayout {
    int64_t nbv, off_sums, off_cursor, off_scratch, bytes;
};
inline TableLayout table_layout(int64_t T, int64_t V) {
    TableLayout L;
    L.nbv = cdiv64(V, MS_BLOCK);
    L.off_sums = MS_WS_HEAD;
    L.off_cursor = align64(L.off_sums + L.nbv * 4);
    L.off_scratch = align64(L.off_cursor + V * 4);
    L.bytes = align64(L.off_scratch + 3 * T * 4);
    return L;
}

}  // namespace

#define MS_ARGS_CHECK(name)                                                                                                                    \
    TDGP_CHECK(ms_sizes_ok(T, V), TDGP_EINVAL, name ": need 0 <= 3 T <= 2^31 - 1 and 0 <= V <= 2^31 - 2 (got T = %lld, V = %lld)", (long long)T, \
               (long long)V);                                                                                                                  \
    TDGP_CHECK(T == 0 || tris, TDGP_EINVAL, name ": null triangles")

TDGP_API int64_t tdgp_mesh_corner_table_workspace_bytes(int64_t T, int64_t V) {
    if (!ms_sizes_ok(T, V)) return -1;
    return table_layout(T, V).bytes;
}

TDGP_API int tdgp_mesh_corner_table(const int32_t* tris, int64_t T, int64_t V, int32_t* degree, int32_t* start, int32_t* corner, void* workspace,
                                    int64_t workspace_bytes, tdgp_stream_t stream) {
    MS_ARGS_CHECK("mesh_corner_table");
    TDGP_CHECK(workspace && start && (V == 0 || degree) && (T == 0 || corner), TDGP_EINVAL, "mesh_corner_table: null pointer");
    TDGP_CHECK(((uintptr_t)workspace & 15) == 0, TDGP_EINVAL, "mesh_corner_table: workspace must be 16-byte aligned");
    const TableLayout L = table_layout(T, V);
    TDGP_CHECK(workspace_bytes >= L.bytes, TDGP_EWORKSPACE, "mesh_corner_table: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.bytes);
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int64_t* total = (int64_t*)ws;
    uint32_t* sums = (uint32_t*)(ws + L.off_sums);
    int* cursor = (int*)(ws + L.off_cursor);
    int32_t* scratch = (int32_t*)(ws + L.off_scratch);
    if (V == 0) {                                 // no vertex: every triangle is skipped; start[0] = total = 0
        if (hipMemsetAsync(start, 0, sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(total, 0, sizeof(int64_t), s) != hipSuccess) {
            tdgp_set_error("mesh_corner_table: clearing the total failed");
            return TDGP_ELAUNCH;
        }
        return TDGP_OK;
    }
    if (hipMemsetAsync(degree, 0, (size_t)V * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(cursor, 0, (size_t)V * sizeof(int32_t), s) != hipSuccess) {
        tdgp_set_error("mesh_corner_table: clearing the counters failed");
        return TDGP_ELAUNCH;
    }
    if (T > 0) {
        TDGP_LAUNCH("ct_count_kernel", ct_count_kernel, dim3(ms_blocks(T)), dim3(MS_BLOCK), 0, s, tris, T, V, (int*)degree);
        TDGP_LAUNCH_CHECK();
    }
    TDGP_LAUNCH("ct_sums_kernel", ct_sums_kernel, dim3((unsigned)L.nbv), dim3(MS_BLOCK), 0, s, (const int*)degree, V, sums);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("ms_scan_kernel", ms_scan_kernel, dim3(1), dim3(1024), 0, s, sums, L.nbv, total);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("ct_start_kernel", ct_start_kernel, dim3((unsigned)L.nbv), dim3(MS_BLOCK), 0, s, (const int*)degree, V, (const uint32_t*)sums, start);
    TDGP_LAUNCH_CHECK();
    if (T > 0) {
        TDGP_LAUNCH("ct_fill_kernel", ct_fill_kernel, dim3(ms_blocks(T)), dim3(MS_BLOCK), 0, s, tris, T, V, (const int32_t*)start, cursor, scratch);
        TDGP_LAUNCH_CHECK();
        TDGP_LAUNCH("ct_rank_kernel", ct_rank_kernel, dim3(ms_blocks(3 * T)), dim3(MS_BLOCK), 0, s, tris, T, V, (const int32_t*)start, (const int32_t*)scratch,
                    (const int64_t*)total, corner);
        TDGP_LAUNCH_CHECK();
    }
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_vertex_normals(const float* vertices, const int32_t* tris, int64_t T, int64_t V, const int32_t* start, const int32_t* corner, int weight,
                                      float* normal_out, tdgp_stream_t stream) {
    MS_ARGS_CHECK("mesh_vertex_normals");
    TDGP_CHECK(weight == 0 || weight == 1, TDGP_EINVAL, "mesh_vertex_normals: weight must be 0 (area) or 1 (uniform), got %d", weight);
    if (V == 0) return TDGP_OK;
    TDGP_CHECK(vertices && start && normal_out && (T == 0 || corner), TDGP_EINVAL, "mesh_vertex_normals: null pointer");
    TDGP_LAUNCH("vertex_normals_kernel", vertex_normals_kernel, dim3(ms_blocks(V)), dim3(MS_BLOCK), 0, (hipStream_t)stream, vertices, tris, T, V, start, corner, weight,
                normal_out);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_boundary_vertices(const int32_t* tris, int64_t T, int64_t V, const int32_t* start, const int32_t* corner, uint8_t* rim_out,
                                         tdgp_stream_t stream) {
    MS_ARGS_CHECK("mesh_boundary_vertices");
    if (V == 0) return TDGP_OK;
    TDGP_CHECK(start && rim_out && (T == 0 || corner), TDGP_EINVAL, "mesh_boundary_vertices: null pointer");
    TDGP_LAUNCH("boundary_kernel", boundary_kernel, dim3(ms_blocks(V)), dim3(MS_BLOCK), 0, (hipStream_t)stream, tris, T, V, start, corner, rim_out);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_smooth_step(const float* vertices_in, const int32_t* tris, int64_t T, int64_t V, const int32_t* start, const int32_t* corner, double factor,
                                   const uint8_t* pinned, float* vertices_out, tdgp_stream_t stream) {
    MS_ARGS_CHECK("mesh_smooth_step");
    TDGP_CHECK(factor == factor && factor > -(double)__builtin_inff() && factor < (double)__builtin_inff(), TDGP_EINVAL, "mesh_smooth_step: factor must be finite");
    if (V == 0) return TDGP_OK;
    TDGP_CHECK(vertices_in && vertices_out && start && (T == 0 || corner), TDGP_EINVAL, "mesh_smooth_step: null pointer");
    const char* a = (const char*)vertices_in;
    const char* b = (const char*)vertices_out;
    TDGP_CHECK(a + V * 12 <= b || b + V * 12 <= a, TDGP_EINVAL, "mesh_smooth_step: vertices_out must not overlap vertices_in");
    TDGP_LAUNCH("smooth_step_kernel", smooth_step_kernel, dim3(ms_blocks(V)), dim3(MS_BLOCK), 0, (hipStream_t)stream, vertices_in, tris, T, V, start, corner, factor,
                pinned, vertices_out);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_interp_normals(const int32_t* tri, const int32_t* status, const float* t_hit, const float* ray_o, const float* ray_d, int64_t rays,
                                      const float* vertices, int64_t V, const int32_t* tris, int64_t T, const float* vertex_normal, float* normal,
                                      tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= 2147483647ll && T >= 0 && T <= 2147483647ll, TDGP_EINVAL, "mesh_interp_normals: V and T must lie in [0, 2^31 - 1]");
    TDGP_CHECK(rays >= 0 && rays <= ((int64_t)1 << 30), TDGP_EINVAL, "mesh_interp_normals: bad ray count");
    if (rays == 0 || T == 0 || V == 0) return TDGP_OK;
    TDGP_CHECK(tri && status && t_hit && ray_o && ray_d && vertices && tris && vertex_normal && normal, TDGP_EINVAL, "mesh_interp_normals: null pointer");
    TDGP_LAUNCH("interp_normals_kernel", interp_normals_kernel, dim3((unsigned)cdiv64(rays, MS_BLOCK)), dim3(MS_BLOCK), 0, (hipStream_t)stream, tri, status, t_hit, ray_o,
                ray_d, rays, vertices, V, tris, T, vertex_normal, normal);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

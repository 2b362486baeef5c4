// mesh_decimate.hip -- round-based quadric edge collapse (Garland-Heckbert 1997) with a link-condition test, for the indexed mesh marching
// cubes leaves on the device (contract in include/tdgp.h).  Each round collapses an independent set of edges: every
// candidate claims its two one-rings with one unsigned 64-bit atomic minimum per vertex, and an edge is collapsed when it still owns its
// endpoints and its two opposite vertices -- a pure function of the arrays, the same bytes on every run.
//
// Replaces (host / third-party for the reference's users): trimesh / MeshLab quadric decimation on a host copy of the mesh.  Nothing here
// has a counterpart inside the reference itself.
//
//   quadric_kernel            one lane per vertex: position widened, the area-weighted plane quadric of its corners in corner-table order
//   candidate_kernel          one lane per corner (a -> b, a < b): edge used twice, rim, opposite vertices' valence, link condition, placement
//                             (quadric_solve.h: the Jacobi of mesh_simplify.hip), error bound, no flip -> key = (float cost bits, mix(corner))
//   claim_kernel              one lane per candidate: best[v] = min(best[v], key) over {a, b} u N(a) u N(b); a claim that a read shows lost is not sent
//   select_kernel             one lane per candidate: selected iff it holds best at a, b, c, d
//   dc_sums_kernel -> dc_scan_kernel -> dc_list_kernel        the selected corners as an ascending list, counted (device_scan.h; no atomics)
//   apply_kernel              one lane per selected edge: the survivor's position, quadric, weight, attributes; parent[removed] = survivor
//   alive_sums_kernel -> dc_scan_kernel -> gather_kernel -> map_kernel   survivors in input order as fp32, vertex_map through the parent chains
// Everything is double and sequential per lane, every operation rounded once (-ffp-contract=off).  No float atomics, no kernel waits for
// another workgroup.  The corner walks are short (valence about 6); one-wave blocks keep the divergent walks of the candidate kernel spread
// over every CU, and neighbouring lanes hold the corners of neighbouring triangles, so their gathers share lines.
#include "common.h"
#include "device_scan.h"
#include "quadric_solve.h"

namespace {

constexpr int DC_BLOCK = 256;
constexpr int DC_WALK_BLOCK = 64;
constexpr int64_t DC_WS_HEAD = 64;            // bytes in front of the block sums: the total as one int64
constexpr int64_t DC_T_MAX = 715827882ll;     // 3 T <= 2^31 - 1
constexpr int64_t DC_V_MAX = (int64_t)INT32_MAX - 1;
constexpr int DC_CHANNELS_MAX = 4096;
constexpr uint64_t DC_NONE = ~0ull;

struct DcMesh {
    const int32_t* tris;
    int64_t T, V;
    const int32_t* start;
    const int32_t* corner;
};

// the clamped corner range of v (include/tdgp.h, the gathers of the mesh-surface block)
__device__ __forceinline__ void dc_range(const DcMesh& m, int64_t v, int64_t& s, int64_t& e) {
    int64_t n = m.start[m.V];
    n = n < 0 ? 0 : (n > 3 * m.T ? 3 * m.T : n);
    s = m.start[v];
    e = m.start[v + 1];
    s = s < 0 ? 0 : (s > n ? n : s);
    e = e < s ? s : (e > n ? n : e);
}

// corner j of the table -> its triangle's indices and its slot; false for an id outside [0, 3T) or a triangle naming an index outside [0, V)
__device__ __forceinline__ bool dc_corner(const DcMesh& m, int64_t j, int (&idx)[3], int& slot) {
    const int cid = m.corner[j];
    if (cid < 0 || cid >= 3 * m.T) return false;
    const int64_t t = cid / 3;
    slot = (int)(cid - 3 * t);
#pragma unroll
    for (int i = 0; i < 3; i++) idx[i] = m.tris[t * 3 + i];
    return idx[0] >= 0 && idx[1] >= 0 && idx[2] >= 0 && idx[0] < m.V && idx[1] < m.V && idx[2] < m.V;
}

__device__ __forceinline__ bool dc_edge(const DcMesh& m, int64_t k, int& a, int& b) {
    const int64_t t = k / 3;
    const int i = (int)(k - 3 * t);
    const int i0 = m.tris[t * 3 + 0], i1 = m.tris[t * 3 + 1], i2 = m.tris[t * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= m.V || i1 >= m.V || i2 >= m.V) return false;
    a = i == 0 ? i0 : (i == 1 ? i1 : i2);
    b = i == 0 ? i1 : (i == 1 ? i2 : i0);
    return true;
}

__device__ __forceinline__ uint32_t dc_mix(uint32_t h) {       // a bijection on uint32: xor-shifts and multiplications by odd constants
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ void dc_cross(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], double (&n)[3]) {
    double e1[3], e2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        e1[c] = p1[c] - p0[c];
        e2[c] = p2[c] - p0[c];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

__global__ __launch_bounds__(1024) void dc_scan_kernel(uint32_t* __restrict__ block_sums, int64_t nb, int64_t* __restrict__ total) {
    scan_block_sums<1>(block_sums, nb, total);
}

// ---- quadrics ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DC_WALK_BLOCK) void quadric_kernel(const float* __restrict__ verts, DcMesh m, double* __restrict__ pos,
                                                                 double* __restrict__ quadric, double* __restrict__ weight) {
    const int64_t v = blockIdx.x * (int64_t)DC_WALK_BLOCK + threadIdx.x;
    if (v >= m.V) return;
#pragma unroll
    for (int c = 0; c < 3; c++) pos[v * 3 + c] = (double)verts[v * 3 + c];
    double Q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double w = 0.0;
    int64_t s, e;
    dc_range(m, v, s, e);
    for (int64_t j = s; j < e; j++) {
        int idx[3], slot;
        if (!dc_corner(m, j, idx, slot)) continue;
        double p[3][3], n[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) p[i][c] = (double)verts[(int64_t)idx[i] * 3 + c];
        dc_cross(p[0], p[1], p[2], n);
        const double l = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        if (!(l > 0.0 && l < (double)__builtin_inff())) continue;
        double q[4];
#pragma unroll
        for (int c = 0; c < 3; c++) q[c] = n[c] / l;
        q[3] = -((q[0] * p[0][0] + q[1] * p[0][1]) + q[2] * p[0][2]);
        const double wt = l * 0.5;
        int o = 0;
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = r; c < 4; c++) {
                Q[o] = Q[o] + (wt * q[r]) * q[c];
                o++;
            }
        w = w + wt;
    }
#pragma unroll
    for (int i = 0; i < 10; i++) quadric[v * 10 + i] = Q[i];
    weight[v] = w;
}

// ---- candidates --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dc_is_neighbour(const DcMesh& m, int v, int w) {
    int64_t s, e;
    dc_range(m, v, s, e);
    for (int64_t j = s; j < e; j++) {
        int idx[3], slot;
        if (!dc_corner(m, j, idx, slot)) continue;
        if (idx[(slot + 1) % 3] == w || idx[(slot + 2) % 3] == w) return true;
    }
    return false;
}

// every triangle of v that does not name `other` keeps the side it faces when v moves to x
__device__ __forceinline__ bool dc_no_flip(const DcMesh& m, const double* __restrict__ pos, int v, int other, const double (&x)[3]) {
    int64_t s, e;
    dc_range(m, v, s, e);
    for (int64_t j = s; j < e; j++) {
        int idx[3], slot;
        if (!dc_corner(m, j, idx, slot)) continue;
        if (idx[0] == other || idx[1] == other || idx[2] == other) continue;
        double p[3][3], q[3][3], n0[3], n1[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                p[i][c] = pos[(int64_t)idx[i] * 3 + c];
                q[i][c] = i == slot ? x[c] : p[i][c];
            }
        dc_cross(p[0], p[1], p[2], n0);
        dc_cross(q[0], q[1], q[2], n1);
        const double dot = (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2];
        if (!(dot > 0.0)) return false;
    }
    return true;
}

__global__ __launch_bounds__(DC_WALK_BLOCK) void candidate_kernel(const double* __restrict__ pos, const double* __restrict__ quadric,
                                                                   const double* __restrict__ weight, const uint8_t* __restrict__ rim, DcMesh m,
                                                                   int bounded, double max_error2, double rank_tol, uint64_t* __restrict__ key,
                                                                   double* __restrict__ place, int32_t* __restrict__ opposite) {
    const int64_t k = blockIdx.x * (int64_t)DC_WALK_BLOCK + threadIdx.x;
    if (k >= 3 * m.T) return;
    key[k] = DC_NONE;
    int a, b;
    if (!dc_edge(m, k, a, b) || !(a < b)) return;
    const bool rim_a = rim && rim[a] != 0, rim_b = rim && rim[b] != 0;
    if (rim_a && rim_b) return;
    // the triangles on the edge and their third vertices, in a's table order
    int64_t sa, ea;
    dc_range(m, a, sa, ea);
    int used = 0, cd[2] = {-1, -1};
    for (int64_t j = sa; j < ea; j++) {
        int idx[3], slot;
        if (!dc_corner(m, j, idx, slot)) continue;
        const int nx = idx[(slot + 1) % 3], pv = idx[(slot + 2) % 3];
        if (nx == b || pv == b) {
            if (used < 2) cd[used] = nx == b ? pv : nx;
            used++;
        }
    }
    if (used != 2 || cd[0] == cd[1]) return;
    int64_t s, e;
    dc_range(m, cd[0], s, e);
    if (e - s <= 3) return;
    dc_range(m, cd[1], s, e);
    if (e - s <= 3) return;
    // link condition: no common neighbour besides the two opposite vertices
    for (int64_t j = sa; j < ea; j++) {
        int idx[3], slot;
        if (!dc_corner(m, j, idx, slot)) continue;
#pragma unroll
        for (int h = 1; h <= 2; h++) {
            const int w = idx[(slot + h) % 3];
            if (w == a || w == b || w == cd[0] || w == cd[1]) continue;
            if (dc_is_neighbour(m, b, w)) return;
        }
    }
    // placement
    double Q[10], pa[3], pb[3], x[3];
#pragma unroll
    for (int i = 0; i < 10; i++) Q[i] = quadric[(int64_t)a * 10 + i] + quadric[(int64_t)b * 10 + i];
    const double w = weight[a] + weight[b];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        pa[c] = pos[(int64_t)a * 3 + c];
        pb[c] = pos[(int64_t)b * 3 + c];
    }
    const double A[3][3] = {{Q[0], Q[1], Q[2]}, {Q[1], Q[4], Q[5]}, {Q[2], Q[5], Q[7]}};
    const double bv[3] = {Q[3], Q[6], Q[8]};
    if (rim_a || rim_b) {
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] = rim_a ? pa[c] : pb[c];
    } else {
        double mid[3];
#pragma unroll
        for (int c = 0; c < 3; c++) mid[c] = (pa[c] + pb[c]) * 0.5;
        quadric_minimise(A, bv, mid, rank_tol, x);
        bool finite = true;
#pragma unroll
        for (int c = 0; c < 3; c++) finite = finite && (x[c] - x[c] == 0.0);
        if (!finite) {
#pragma unroll
            for (int c = 0; c < 3; c++) x[c] = mid[c];
        }
    }
    double Ax[3];
#pragma unroll
    for (int c = 0; c < 3; c++) Ax[c] = (A[c][0] * x[0] + A[c][1] * x[1]) + A[c][2] * x[2];
    const double xAx = (x[0] * Ax[0] + x[1] * Ax[1]) + x[2] * Ax[2];
    const double bx = (bv[0] * x[0] + bv[1] * x[1]) + bv[2] * x[2];
    double cost = (xAx + 2.0 * bx) + Q[9];
    if (cost != cost) return;
    cost = cost > 0.0 ? cost : 0.0;
    if (bounded && !(cost <= max_error2 * w)) return;
    if (!dc_no_flip(m, pos, a, b, x) || !dc_no_flip(m, pos, b, a, x)) return;
#pragma unroll
    for (int c = 0; c < 3; c++) place[k * 3 + c] = x[c];
    opposite[k * 2 + 0] = cd[0];
    opposite[k * 2 + 1] = cd[1];
    key[k] = ((uint64_t)__float_as_uint((float)cost) << 32) | (uint64_t)dc_mix((uint32_t)k);
}

// best[v] = min(best[v], key).  Values only fall, so a plain read that already shows a smaller one makes the atomic a no-op that can be left out:
// a vertex is claimed by every candidate of its two-ring, and all but a few of them lose.  The result is the same minimum either way.
__device__ __forceinline__ void dc_claim(unsigned long long* __restrict__ best, int v, uint64_t key) {
    if (__atomic_load_n(best + v, __ATOMIC_RELAXED) > key) atomicMin(best + v, (unsigned long long)key);
}

__global__ __launch_bounds__(DC_WALK_BLOCK) void claim_kernel(const uint64_t* __restrict__ key, DcMesh m, unsigned long long* __restrict__ best) {
    const int64_t k = blockIdx.x * (int64_t)DC_WALK_BLOCK + threadIdx.x;
    if (k >= 3 * m.T) return;
    const uint64_t kk = key[k];
    if (kk == DC_NONE) return;
    int ab[2];
    if (!dc_edge(m, k, ab[0], ab[1])) return;
    for (int h = 0; h < 2; h++) {
        dc_claim(best, ab[h], kk);
        int64_t s, e;
        dc_range(m, ab[h], s, e);
        for (int64_t j = s; j < e; j++) {
            int idx[3], slot;
            if (!dc_corner(m, j, idx, slot)) continue;
            dc_claim(best, idx[(slot + 1) % 3], kk);
            dc_claim(best, idx[(slot + 2) % 3], kk);
        }
    }
}

__global__ __launch_bounds__(DC_BLOCK) void select_kernel(const uint64_t* __restrict__ key, const uint64_t* __restrict__ best,
                                                          const int32_t* __restrict__ opposite, DcMesh m, uint8_t* __restrict__ flag) {
    const int64_t k = blockIdx.x * (int64_t)DC_BLOCK + threadIdx.x;
    if (k >= 3 * m.T) return;
    const uint64_t kk = key[k];
    int a, b;
    bool sel = kk != DC_NONE && dc_edge(m, k, a, b);
    if (sel) {
        const int c = opposite[k * 2 + 0], d = opposite[k * 2 + 1];
        sel = c >= 0 && c < m.V && d >= 0 && d < m.V && best[a] == kk && best[b] == kk && best[c] == kk && best[d] == kk;
    }
    flag[k] = sel ? 1 : 0;
}

__global__ __launch_bounds__(DC_BLOCK) void dc_sums_kernel(const uint8_t* __restrict__ flag, int64_t n, uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t i = blockIdx.x * (int64_t)DC_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<DC_BLOCK>(i < n && flag[i] != 0 ? 1 : 0, sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(DC_BLOCK) void dc_list_kernel(const uint8_t* __restrict__ flag, int64_t n, const uint32_t* __restrict__ block_offs,
                                                           int32_t* __restrict__ list) {
    __shared__ int sm[4];
    const int64_t i = blockIdx.x * (int64_t)DC_BLOCK + threadIdx.x;
    const int f = i < n && flag[i] != 0 ? 1 : 0;
    int total;
    const int64_t at = (int64_t)block_offs[blockIdx.x] + block_excl_scan<DC_BLOCK>(f, sm, total);
    if (f && at < n) list[at] = (int32_t)i;
}

// ---- apply -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DC_BLOCK) void apply_kernel(const int32_t* __restrict__ list, int64_t K, DcMesh m, const uint8_t* __restrict__ rim,
                                                         const double* __restrict__ place, double* __restrict__ pos, double* __restrict__ quadric,
                                                         double* __restrict__ weight, double* __restrict__ attr, int channels,
                                                         int32_t* __restrict__ parent) {
    const int64_t j = blockIdx.x * (int64_t)DC_BLOCK + threadIdx.x;
    if (j >= K) return;
    const int64_t k = list[j];
    if (k < 0 || k >= 3 * m.T) return;
    int a, b;
    if (!dc_edge(m, k, a, b) || a == b) return;
    const bool keep_b = rim && rim[a] == 0 && rim[b] != 0;
    const int s = keep_b ? b : a, r = keep_b ? a : b;
    double x[3], pa[3], pb[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x[c] = place[k * 3 + c];
        pa[c] = pos[(int64_t)a * 3 + c];
        pb[c] = pos[(int64_t)b * 3 + c];
    }
    if (channels > 0) {
        double d[3];
#pragma unroll
        for (int c = 0; c < 3; c++) d[c] = pb[c] - pa[c];
        const double num = ((x[0] - pa[0]) * d[0] + (x[1] - pa[1]) * d[1]) + (x[2] - pa[2]) * d[2];
        const double den = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        double t = num / den;
        t = t > 0.0 ? t : 0.0;                                   // NaN -> 0
        t = t > 1.0 ? 1.0 : t;
        const double u = 1.0 - t;
        for (int ch = 0; ch < channels; ch++) {
            const double va = attr[(int64_t)a * channels + ch], vb = attr[(int64_t)b * channels + ch];
            attr[(int64_t)s * channels + ch] = u * va + t * vb;
        }
    }
#pragma unroll
    for (int i = 0; i < 10; i++) quadric[(int64_t)s * 10 + i] = quadric[(int64_t)a * 10 + i] + quadric[(int64_t)b * 10 + i];
    weight[s] = weight[a] + weight[b];
#pragma unroll
    for (int c = 0; c < 3; c++) pos[(int64_t)s * 3 + c] = x[c];
    parent[r] = s;
}

// ---- the final gather --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int dc_alive(const int32_t* __restrict__ parent, int64_t v, int64_t V) { return v < V && parent[v] == (int32_t)v ? 1 : 0; }

__global__ __launch_bounds__(DC_BLOCK) void alive_sums_kernel(const int32_t* __restrict__ parent, int64_t V, uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)DC_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<DC_BLOCK>(dc_alive(parent, v, V), sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(DC_BLOCK) void gather_kernel(const double* __restrict__ pos, const double* __restrict__ attr, int channels,
                                                          const int32_t* __restrict__ parent, int64_t V, const uint32_t* __restrict__ block_offs,
                                                          float* __restrict__ out_v, int64_t V_out, float* __restrict__ out_attr,
                                                          int32_t* __restrict__ vertex_map) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)DC_BLOCK + threadIdx.x;
    const int f = dc_alive(parent, v, V);
    int total;
    const int64_t at = (int64_t)block_offs[blockIdx.x] + block_excl_scan<DC_BLOCK>(f, sm, total);
    if (v >= V) return;
    if (!f || at >= V_out) {
        vertex_map[v] = -1;                                      // map_kernel follows the parents of a removed vertex
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out_v[at * 3 + c] = (float)pos[v * 3 + c];
    for (int ch = 0; ch < channels; ch++) out_attr[at * channels + ch] = (float)attr[v * channels + ch];
    vertex_map[v] = (int32_t)at;
}

__global__ __launch_bounds__(DC_BLOCK) void map_kernel(const int32_t* __restrict__ parent, int64_t V, int64_t max_hops, int32_t* __restrict__ vertex_map) {
    const int64_t v = blockIdx.x * (int64_t)DC_BLOCK + threadIdx.x;
    if (v >= V) return;
    int64_t r = parent[v];
    if (r == v) return;                                          // a survivor: gather_kernel wrote its index, and nobody else writes it
    for (int64_t hop = 0; hop < max_hops; hop++) {
        if (r < 0 || r >= V) return;
        const int64_t p = parent[r];
        if (p == r) {
            vertex_map[v] = vertex_map[r];
            return;
        }
        r = p;
    }
}

inline int64_t dc_ws_bytes(int64_t n) { return align64(DC_WS_HEAD + cdiv64(n, DC_BLOCK) * 4); }
inline bool dc_finite(double x) { return x == x && x > -(double)__builtin_inff() && x < (double)__builtin_inff(); }

inline int dc_clear_total(void* workspace, hipStream_t s, const char* who) {
    if (hipMemsetAsync(workspace, 0, sizeof(int64_t), s) != hipSuccess) {
        tdgp_set_error("%s: clearing the total failed", who);
        return TDGP_ELAUNCH;
    }
    return TDGP_OK;
}

}  // namespace

#define DC_TV_CHECK(name)                                                                                                                       \
    TDGP_CHECK(T >= 0 && T <= DC_T_MAX && V >= 0 && V <= DC_V_MAX, TDGP_EINVAL, name ": need 0 <= 3 T <= 2^31 - 1 and 0 <= V <= 2^31 - 2 (got T = %lld, V = %lld)", \
               (long long)T, (long long)V)

#define DC_WS_CHECK(name, n)                                                                                                                   \
    TDGP_CHECK(workspace, TDGP_EINVAL, name ": null workspace");                                                                               \
    TDGP_CHECK(((uintptr_t)workspace & 15) == 0, TDGP_EINVAL, name ": workspace must be 16-byte aligned");                                     \
    TDGP_CHECK(workspace_bytes >= dc_ws_bytes(n), TDGP_EWORKSPACE, name ": workspace of %lld bytes, %lld needed", (long long)workspace_bytes, \
               (long long)dc_ws_bytes(n))

TDGP_API int tdgp_mesh_decimate_quadrics(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const int32_t* start, const int32_t* corner,
                                         double* position, double* quadric, double* weight, tdgp_stream_t stream) {
    DC_TV_CHECK("mesh_decimate_quadrics");
    if (V == 0) return TDGP_OK;
    TDGP_CHECK(vertices && start && position && quadric && weight && (T == 0 || (triangles && corner)), TDGP_EINVAL, "mesh_decimate_quadrics: null pointer");
    const DcMesh m{triangles, T, V, start, corner};
    TDGP_LAUNCH("quadric_kernel", quadric_kernel, dim3((unsigned)cdiv64(V, DC_WALK_BLOCK)), dim3(DC_WALK_BLOCK), 0, (hipStream_t)stream, vertices, m, position, quadric, weight);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_decimate_candidates(const double* position, const double* quadric, const double* weight, const uint8_t* rim, const int32_t* triangles,
                                           int64_t T, int64_t V, const int32_t* start, const int32_t* corner, double max_error, double rank_tol,
                                           uint64_t* key, double* placement, int32_t* opposite, tdgp_stream_t stream) {
    DC_TV_CHECK("mesh_decimate_candidates");
    TDGP_CHECK(max_error == 0.0 || (dc_finite(max_error) && max_error > 0.0), TDGP_EINVAL, "mesh_decimate_candidates: max_error must be 0 (no bound) or positive and finite");
    TDGP_CHECK(dc_finite(rank_tol) && rank_tol >= 0.0, TDGP_EINVAL, "mesh_decimate_candidates: rank_tol must be finite and not negative");
    if (T == 0) return TDGP_OK;
    TDGP_CHECK(position && quadric && weight && triangles && start && corner && key && placement && opposite, TDGP_EINVAL, "mesh_decimate_candidates: null pointer");
    const DcMesh m{triangles, T, V, start, corner};
    TDGP_LAUNCH("candidate_kernel", candidate_kernel, dim3((unsigned)cdiv64(3 * T, DC_WALK_BLOCK)), dim3(DC_WALK_BLOCK), 0, (hipStream_t)stream, position, quadric, weight, rim,
                m, max_error > 0.0 ? 1 : 0, max_error * max_error, rank_tol, key, placement, opposite);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_decimate_claim(const uint64_t* key, const int32_t* triangles, int64_t T, int64_t V, const int32_t* start, const int32_t* corner,
                                      uint64_t* best, tdgp_stream_t stream) {
    DC_TV_CHECK("mesh_decimate_claim");
    if (V == 0) return TDGP_OK;
    TDGP_CHECK(best, TDGP_EINVAL, "mesh_decimate_claim: null pointer");
    if (hipMemsetAsync(best, 0xff, (size_t)V * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) {
        tdgp_set_error("mesh_decimate_claim: clearing the claims failed");
        return TDGP_ELAUNCH;
    }
    if (T == 0) return TDGP_OK;
    TDGP_CHECK(key && triangles && start && corner, TDGP_EINVAL, "mesh_decimate_claim: null pointer");
    const DcMesh m{triangles, T, V, start, corner};
    TDGP_LAUNCH("claim_kernel", claim_kernel, dim3((unsigned)cdiv64(3 * T, DC_WALK_BLOCK)), dim3(DC_WALK_BLOCK), 0, (hipStream_t)stream, key, m, (unsigned long long*)best);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_mesh_decimate_select_workspace_bytes(int64_t T) {
    if (T < 0 || T > DC_T_MAX) return -1;
    return dc_ws_bytes(3 * T);
}

TDGP_API int tdgp_mesh_decimate_select(const uint64_t* key, const uint64_t* best, const int32_t* opposite, const int32_t* triangles, int64_t T, int64_t V,
                                       uint8_t* flag, int32_t* selected, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    DC_TV_CHECK("mesh_decimate_select");
    DC_WS_CHECK("mesh_decimate_select", 3 * T);
    hipStream_t s = (hipStream_t)stream;
    if (T == 0 || V == 0) return dc_clear_total(workspace, s, "mesh_decimate_select");
    TDGP_CHECK(key && best && opposite && triangles && flag && selected, TDGP_EINVAL, "mesh_decimate_select: null pointer");
    const DcMesh m{triangles, T, V, nullptr, nullptr};
    const int64_t n = 3 * T, nb = cdiv64(n, DC_BLOCK);
    uint32_t* sums = (uint32_t*)((char*)workspace + DC_WS_HEAD);
    TDGP_LAUNCH("select_kernel", select_kernel, dim3((unsigned)nb), dim3(DC_BLOCK), 0, s, key, best, opposite, m, flag);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("dc_sums_kernel", dc_sums_kernel, dim3((unsigned)nb), dim3(DC_BLOCK), 0, s, (const uint8_t*)flag, n, sums);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("dc_scan_kernel", dc_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, (int64_t*)workspace);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("dc_list_kernel", dc_list_kernel, dim3((unsigned)nb), dim3(DC_BLOCK), 0, s, (const uint8_t*)flag, n, (const uint32_t*)sums, selected);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_decimate_apply(const int32_t* selected, int64_t K, const int32_t* triangles, int64_t T, int64_t V, const uint8_t* rim, const double* placement,
                                      double* position, double* quadric, double* weight, double* attribute, int channels, int32_t* parent, tdgp_stream_t stream) {
    DC_TV_CHECK("mesh_decimate_apply");
    TDGP_CHECK(K >= 0 && K <= 3 * T, TDGP_EINVAL, "mesh_decimate_apply: need 0 <= K <= 3 T (got K = %lld)", (long long)K);
    TDGP_CHECK(channels >= 0 && channels <= DC_CHANNELS_MAX, TDGP_EINVAL, "mesh_decimate_apply: channels must lie in [0, %d], got %d", DC_CHANNELS_MAX, channels);
    if (K == 0) return TDGP_OK;
    TDGP_CHECK(selected && triangles && placement && position && quadric && weight && parent && (channels == 0 || attribute), TDGP_EINVAL, "mesh_decimate_apply: null pointer");
    const DcMesh m{triangles, T, V, nullptr, nullptr};
    TDGP_LAUNCH("apply_kernel", apply_kernel, dim3((unsigned)cdiv64(K, DC_BLOCK)), dim3(DC_BLOCK), 0, (hipStream_t)stream, selected, K, m, rim, placement, position, quadric, weight,
                attribute, channels, parent);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_mesh_decimate_gather_workspace_bytes(int64_t V) {
    if (V < 0 || V > DC_V_MAX) return -1;
    return dc_ws_bytes(V);
}

TDGP_API int tdgp_mesh_decimate_gather_count(const int32_t* parent, int64_t V, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= DC_V_MAX, TDGP_EINVAL, "mesh_decimate_gather_count: need 0 <= V <= 2^31 - 2 (got %lld)", (long long)V);
    DC_WS_CHECK("mesh_decimate_gather_count", V);
    hipStream_t s = (hipStream_t)stream;
    if (V == 0) return dc_clear_total(workspace, s, "mesh_decimate_gather_count");
    TDGP_CHECK(parent, TDGP_EINVAL, "mesh_decimate_gather_count: null pointer");
    const int64_t nb = cdiv64(V, DC_BLOCK);
    uint32_t* sums = (uint32_t*)((char*)workspace + DC_WS_HEAD);
    TDGP_LAUNCH("alive_sums_kernel", alive_sums_kernel, dim3((unsigned)nb), dim3(DC_BLOCK), 0, s, parent, V, sums);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("dc_scan_kernel", dc_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, (int64_t*)workspace);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_decimate_gather(const double* position, const double* attribute, int channels, const int32_t* parent, int64_t V, int64_t max_hops,
                                       void* workspace, int64_t workspace_bytes, float* out_vertices, int64_t V_out, float* out_attribute, int32_t* vertex_map,
                                       tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= DC_V_MAX && V_out >= 0 && V_out <= V, TDGP_EINVAL, "mesh_decimate_gather: need 0 <= V_out <= V <= 2^31 - 2 (got V = %lld, V_out = %lld)",
               (long long)V, (long long)V_out);
    TDGP_CHECK(channels >= 0 && channels <= DC_CHANNELS_MAX, TDGP_EINVAL, "mesh_decimate_gather: channels must lie in [0, %d], got %d", DC_CHANNELS_MAX, channels);
    TDGP_CHECK(max_hops >= 0, TDGP_EINVAL, "mesh_decimate_gather: max_hops must not be negative");
    DC_WS_CHECK("mesh_decimate_gather", V);
    if (V == 0) return TDGP_OK;
    TDGP_CHECK(position && parent && vertex_map && (V_out == 0 || out_vertices) && (channels == 0 || (attribute && (V_out == 0 || out_attribute))), TDGP_EINVAL,
               "mesh_decimate_gather: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = cdiv64(V, DC_BLOCK);
    const uint32_t* sums = (const uint32_t*)((char*)workspace + DC_WS_HEAD);
    TDGP_LAUNCH("gather_kernel", gather_kernel, dim3((unsigned)nb), dim3(DC_BLOCK), 0, s, position, attribute, channels, parent, V, sums, out_vertices, V_out, out_attribute,
                vertex_map);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("map_kernel", map_kernel, dim3((unsigned)nb), dim3(DC_BLOCK), 0, s, parent, V, max_hops, vertex_map);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

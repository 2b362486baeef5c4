// mesh_components.hip -- connected components of an indexed triangle mesh, per-component measurements and an order-preserving filter, on
// the device (contract in include/tdgp.h).
//
// Replaces (host / third-party for the reference's users): trimesh's `split` + "keep the largest" on a host copy of the mesh that
// scripts/extract_geometry.py:38-42 builds.  Nothing here has a counterpart inside the reference itself.
//
// Labels: a lock-free union-find over parent[V] with parent[v] <= v AT ALL TIMES (the larger root is always linked under the smaller, so
// the root of a finished component is its smallest vertex):
//   cc_init_kernel      parent[v] = v
//   cc_union_kernel     one lane per triangle: unite(a, b), unite(b, c).  Every access to `parent` is an agent-scope relaxed atomic; the only
//                       retry is the CAS retry (a failure means another lane's link succeeded); no lane waits for another workgroup
//   cc_flatten_kernel   (after the kernel boundary: plain loads) label[v] = root of v
// Dense ids and the filter: positions decided by scans alone -- a block-local scan of 256 flags, ONE block scanning the block sums, block-local
// scan + block offset (device_scan.h, shared with marching cubes), so every output is the same bytes on every run.
// Stats: counts and boxes by integer / ordered-bit atomics (exact, order-independent); the fp64 sums in the store-then-sum form: per-triangle
// terms stored once, summed per component in the fixed order tdgp.h states.  No float atomics anywhere.
#include "common.h"
#include "device_scan.h"

namespace {

constexpr int CC_BLOCK = 256;                 // elements per block (4 waves)
constexpr int64_t CC_WS_HEAD = 64;            // bytes in front of the block sums: totals / counters as int64
constexpr int STATS_ITEMS = 8;               // consecutive 256-element rows a block of the stats kernels takes
constexpr int SUM_BLOCK = 256;                // lanes of the per-component summation (its order is part of the contract)

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

// one block of 1024 threads: exclusive scan of nb block sums in place, the grand total to *total (every total here is at most V or T < 2^31)
__global__ __launch_bounds__(1024) void cc_scan_kernel(uint32_t* __restrict__ block_sums, int64_t nb, int64_t* __restrict__ total) {
    scan_block_sums<1>(block_sums, nb, total);
}

// ---- labels ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int par_load(int* parent, int v) { return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of v.  The walk terminates by the invariant parent[x] <= x: a step goes to p = parent[x] only when p != x, i.e. p < x, so x strictly
// decreases and the walk takes at most v steps whatever the other lanes do meanwhile; it waits for nobody.  On the way every visited vertex
// is pointed at its grandparent (path halving) with an atomic minimum: the new value is an ancestor of x no larger than the old one, so the
// invariant and the partition are kept, and a root (parent[x] == x) is never written here -- roots change only through the CAS of unite().
__device__ __forceinline__ int find_root(int* parent, int x) {
    int p = par_load(parent, x);
    while (p != x) {
        const int g = par_load(parent, p);         // g <= p < x
        if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// Joins the sets of a and b; returns the number of failed compare-and-swaps.  The loop is the lock-free retry only: a CAS on parent[hi] fails
// exactly when another lane linked hi under something smaller in the meantime (that lane succeeded), and the retry continues from the value
// the CAS returned, `seen` < hi.  The larger of the pair therefore strictly decreases from one iteration to the next: at most max(a, b)
// iterations even without anybody else's progress.  (A plain cached load could show "hi is a root" for ever; the atomic load and the CAS's
// own return value cannot.)
__device__ __forceinline__ int unite(int* parent, int a, int b) {
    int fails = 0;
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return fails;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return fails;
        fails++;
        a = seen;                                  // < hi: what hi was linked under
        b = lo;
    }
}

__global__ __launch_bounds__(CC_BLOCK) void cc_init_kernel(int* __restrict__ parent, int64_t V, unsigned long long* __restrict__ retries) {
    const int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (v < V) parent[v] = (int)v;
    if (v == 0) *retries = 0;
}

__device__ __forceinline__ bool tri_ok(int a, int b, int c, int64_t V) {
    return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_union_kernel(const int32_t* __restrict__ tris, int64_t T, int64_t V, int* parent,
                                                            unsigned long long* retries) {
    const int64_t t = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    int fails = 0;
    if (t < T) {
        const int a = tris[t * 3 + 0], b = tris[t * 3 + 1], c = tris[t * 3 + 2];
        if (tri_ok(a, b, c, V)) {                  // an index outside [0, V) skips its triangle and is never dereferenced
            if (a != b) fails += unite(parent, a, b);
            if (b != c) fails += unite(parent, b, c);
        }
    }
    const unsigned wave_fails = wave_sum_u32((unsigned)fails);      // the diagnostic counter: one add per wave, not one per lane
    if (lane_id() == 0 && wave_fails) atomicAdd(retries, (unsigned long long)wave_fails);
}

// runs after the kernel boundary and only reads `parent`: plain loads
__global__ __launch_bounds__(CC_BLOCK) void cc_flatten_kernel(const int* __restrict__ parent, int32_t* __restrict__ label, int64_t V) {
    const int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (v >= V) return;
    int x = (int)v;
    for (int p = parent[x]; p != x; p = parent[x]) x = p;      // terminates: parent[x] <= x, so x strictly decreases
    label[v] = x;
}

// ---- dense ids ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_BLOCK) void ids_count_kernel(const int32_t* __restrict__ label, int64_t V, uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<CC_BLOCK>(v < V && label[v] == (int)v ? 1 : 0, sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(CC_BLOCK) void ids_roots_kernel(const int32_t* __restrict__ label, int64_t V, const uint32_t* __restrict__ block_offs,
                                                             int32_t* __restrict__ component) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    const bool root = v < V && label[v] == (int)v;
    int total;
    const int rank = (int)block_offs[blockIdx.x] + block_excl_scan<CC_BLOCK>(root ? 1 : 0, sm, total);
    if (root) component[v] = rank;
}

// roots were written by the launch before and are not written here
__global__ __launch_bounds__(CC_BLOCK) void ids_spread_kernel(const int32_t* __restrict__ label, int64_t V, int32_t* component) {
    const int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int l = label[v];
    if (l != (int)v) component[v] = (l >= 0 && l < V) ? component[l] : -1;
}

// ---- stats -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_BLOCK) void stats_init_kernel(int64_t K, unsigned long long* __restrict__ tri_count, unsigned long long* __restrict__ vert_count,
                                                              uint32_t* __restrict__ box_min, uint32_t* __restrict__ box_max) {
    const int64_t k = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (k >= K) return;
    tri_count[k] = 0;
    vert_count[k] = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) { box_min[k * 3 + c] = 0xffffffffu; box_max[k * 3 + c] = 0u; }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64); v = o > v ? o : v; }
    return v;
}

// A minimum / maximum only has to reach memory when it improves what is there.  The load may be stale, but the stored value only ever moves
// one way, so a stale value is never better than the current one: an improvement is never skipped, and the result stays exact.
__device__ __forceinline__ void box_min(uint32_t* p, uint32_t key) {
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}
__device__ __forceinline__ void box_max(uint32_t* p, uint32_t key) {
    if (key > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, key);
}

// A block takes STATS_ITEMS * 256 consecutive vertices.  Marching cubes numbers neighbours together, so most of them lie in the component of
// the block's first vertex (`kb`): those are folded in registers and leave the block as ONE set of 7 atomics (thousands of same-address
// atomics serialise, about 0.15 us each measured); every other vertex issues its own.  Either way the results are a count and minima /
// maxima of integers: exact and independent of the order.
__global__ __launch_bounds__(CC_BLOCK) void stats_verts_kernel(const float* __restrict__ verts, const int32_t* __restrict__ component, int64_t V, int64_t K,
                                                               unsigned long long* vert_count, uint32_t* box_min_, uint32_t* box_max_) {
    __shared__ int kb_s;
    __shared__ uint32_t red_lo[4][3], red_hi[4][3];
    __shared__ unsigned red_n[4];
    const int64_t base = blockIdx.x * (int64_t)(CC_BLOCK * STATS_ITEMS);
    if (threadIdx.x == 0) {
        const int k = base < V ? component[base] : -1;
        kb_s = (k >= 0 && k < K) ? k : -1;
    }
    __syncthreads();
    const int kb = kb_s;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    unsigned n = 0;
    for (int r = 0; r < STATS_ITEMS; r++) {
        const int64_t v = base + (int64_t)r * CC_BLOCK + threadIdx.x;
        if (v >= V) break;
        const int k = component[v];
        if (k < 0 || k >= K) continue;
        uint32_t key[3];
#pragma unroll
        for (int c = 0; c < 3; c++) key[c] = f32_key(verts[v * 3 + c]);
        if (k == kb) {
            n++;
#pragma unroll
            for (int c = 0; c < 3; c++) { lo[c] = key[c] < lo[c] ? key[c] : lo[c]; hi[c] = key[c] > hi[c] ? key[c] : hi[c]; }
        } else {
            atomicAdd(vert_count + k, 1ull);
#pragma unroll
            for (int c = 0; c < 3; c++) { box_min(box_min_ + (int64_t)k * 3 + c, key[c]); box_max(box_max_ + (int64_t)k * 3 + c, key[c]); }
        }
    }
    n = wave_sum_u32(n);
#pragma unroll
    for (int c = 0; c < 3; c++) { lo[c] = wave_min_u32(lo[c]); hi[c] = wave_max_u32(hi[c]); }
    const int wv = threadIdx.x >> 6;
    if (lane_id() == 0) {
        red_n[wv] = n;
#pragma unroll
        for (int c = 0; c < 3; c++) { red_lo[wv][c] = lo[c]; red_hi[wv][c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x != 0 || kb < 0) return;
    const unsigned total = red_n[0] + red_n[1] + red_n[2] + red_n[3];
    if (total == 0) return;
    atomicAdd(vert_count + kb, (unsigned long long)total);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        uint32_t l = red_lo[0][c], h = red_hi[0][c];
#pragma unroll
        for (int w = 1; w < 4; w++) { l = red_lo[w][c] < l ? red_lo[w][c] : l; h = red_hi[w][c] > h ? red_hi[w][c] : h; }
        box_min(box_min_ + (int64_t)kb * 3 + c, l);
        box_max(box_max_ + (int64_t)kb * 3 + c, h);
    }
}

__global__ __launch_bounds__(CC_BLOCK) void stats_decode_kernel(int64_t n, uint32_t* box_min, uint32_t* box_max) {
    const int64_t i = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (i >= n) return;
    reinterpret_cast<float*>(box_min)[i] = key_f32(box_min[i]);
    reinterpret_cast<float*>(box_max)[i] = key_f32(box_max[i]);
}

// component of triangle t (that of its first vertex), or K for a triangle with an index out of range: K sorts behind every component and is
// summed by nobody
__device__ __forceinline__ int tri_component(const int32_t* tris, const int32_t* component, int64_t t, int64_t V, int64_t K) {
    const int ia = tris[t * 3 + 0], ib = tris[t * 3 + 1], ic = tris[t * 3 + 2];
    if (!tri_ok(ia, ib, ic, V)) return (int)K;
    const int k = component[ia];
    return (k >= 0 && k < K) ? k : (int)K;
}

// A block takes STATS_ITEMS * 256 consecutive triangles: per triangle its key and its two terms; the triangle count like the vertex count above
// (the triangles of the block's first component are counted in registers and leave as one atomic, the others issue their own).
__global__ __launch_bounds__(CC_BLOCK) void stats_tris_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris, const int32_t* __restrict__ component,
                                                              int64_t T, int64_t V, int64_t K, unsigned long long* tri_count, int32_t* __restrict__ tri_key,
                                                              double* __restrict__ area_term, double* __restrict__ vol_term) {
    __shared__ int kb_s;
    __shared__ unsigned red_n[4];
    const int64_t base = blockIdx.x * (int64_t)(CC_BLOCK * STATS_ITEMS);
    if (threadIdx.x == 0) kb_s = base < T ? tri_component(tris, component, base, V, K) : (int)K;
    __syncthreads();
    const int kb = kb_s;
    unsigned n = 0;
    for (int r = 0; r < STATS_ITEMS; r++) {
        const int64_t t = base + (int64_t)r * CC_BLOCK + threadIdx.x;
        if (t >= T) break;
        const int k = tri_component(tris, component, t, V, K);
        double area = 0.0, vol = 0.0;
        if (k < K) {
            const int ia = tris[t * 3 + 0], ib = tris[t * 3 + 1], ic = tris[t * 3 + 2];
            double a[3], b[3], c[3];
#pragma unroll
            for (int j = 0; j < 3; j++) { a[j] = (double)verts[(int64_t)ia * 3 + j]; b[j] = (double)verts[(int64_t)ib * 3 + j]; c[j] = (double)verts[(int64_t)ic * 3 + j]; }
            const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2], w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
            const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
            area = 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            const double x0 = b[1] * c[2] - b[2] * c[1], x1 = b[2] * c[0] - b[0] * c[2], x2 = b[0] * c[1] - b[1] * c[0];
            vol = (a[0] * x0 + a[1] * x1) + a[2] * x2;
            if (k == kb) n++;
            else atomicAdd(tri_count + k, 1ull);
        }
        tri_key[t] = k;
        area_term[t] = area;
        vol_term[t] = vol;
    }
    n = wave_sum_u32(n);
    if (lane_id() == 0) red_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x != 0 || kb >= K) return;
    const unsigned total = red_n[0] + red_n[1] + red_n[2] + red_n[3];
    if (total) atomicAdd(tri_count + kb, (unsigned long long)total);
}

// one block per component: the fixed summation order of tdgp.h.  order[] = the triangles sorted by component with their order kept (a stable
// sort of tri_key), start[k] = exclusive prefix of tri_count.
__global__ __launch_bounds__(SUM_BLOCK) void stats_sum_kernel(const int64_t* __restrict__ order, const int64_t* __restrict__ start, const int64_t* __restrict__ tri_count,
                                                              int64_t T, const double* __restrict__ area_term, const double* __restrict__ vol_term,
                                                              double* __restrict__ area, double* __restrict__ volume) {
    __shared__ double sa[SUM_BLOCK], sv[SUM_BLOCK];
    const int64_t k = blockIdx.x;
    const int64_t s0 = start[k], n = tri_count[k];
    double pa = 0.0, pv = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += SUM_BLOCK) {
        const int64_t pos = s0 + j;
        if (pos < 0 || pos >= T) break;            // the caller's arrays are never trusted past T
        const int64_t t = order[pos];
        if (t < 0 || t >= T) continue;
        pa += area_term[t];
        pv += vol_term[t];
    }
    sa[threadIdx.x] = pa;
    sv[threadIdx.x] = pv;
    __syncthreads();
    for (int d = SUM_BLOCK / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) { sa[threadIdx.x] += sa[threadIdx.x + d]; sv[threadIdx.x] += sv[threadIdx.x + d]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { area[k] = sa[0]; volume[k] = sv[0] / 6.0; }
}

// ---- compaction --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vert_kept(const int32_t* component, const uint8_t* keep, int64_t v, int64_t K) {
    const int k = component[v];
    return k >= 0 && k < K && keep[k] != 0;
}
__device__ __forceinline__ bool tri_kept(const int32_t* tris, const int32_t* component, const uint8_t* keep, int64_t t, int64_t V, int64_t K) {
    const int a = tris[t * 3 + 0], b = tris[t * 3 + 1], c = tris[t * 3 + 2];
    // all three corners are asked: for labels of this mesh they agree; for a caller's own component array no kept triangle names a dropped vertex
    return tri_ok(a, b, c, V) && vert_kept(component, keep, a, K) && vert_kept(component, keep, b, K) && vert_kept(component, keep, c, K);
}

__global__ __launch_bounds__(CC_BLOCK) void compact_count_verts_kernel(const int32_t* __restrict__ component, const uint8_t* __restrict__ keep, int64_t V, int64_t K,
                                                                       uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<CC_BLOCK>(v < V && vert_kept(component, keep, v, K) ? 1 : 0, sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(CC_BLOCK) void compact_count_tris_kernel(const int32_t* __restrict__ tris, const int32_t* __restrict__ component,
                                                                      const uint8_t* __restrict__ keep, int64_t T, int64_t V, int64_t K, uint32_t* __restrict__ block_sums) {
    __shared__ int sm[4];
    const int64_t t = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    int total;
    block_excl_scan<CC_BLOCK>(t < T && tri_kept(tris, component, keep, t, V, K) ? 1 : 0, sm, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(CC_BLOCK) void compact_emit_verts_kernel(const float* __restrict__ verts, const int32_t* __restrict__ component, const uint8_t* __restrict__ keep,
                                                                      int64_t V, int64_t K, const uint32_t* __restrict__ block_offs, float* __restrict__ out_verts, int64_t Vout,
                                                                      int32_t* __restrict__ vertex_map) {
    __shared__ int sm[4];
    const int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    const bool kept = v < V && vert_kept(component, keep, v, K);
    int total;
    const int64_t pos = (int64_t)block_offs[blockIdx.x] + block_excl_scan<CC_BLOCK>(kept ? 1 : 0, sm, total);
    if (v >= V) return;
    const bool fits = kept && pos < Vout;          // Vout is the caller's: never write past the buffer it sized
    vertex_map[v] = fits ? (int32_t)pos : -1;
    if (fits && out_verts) {
        out_verts[pos * 3 + 0] = verts[v * 3 + 0];
        out_verts[pos * 3 + 1] = verts[v * 3 + 1];
        out_verts[pos * 3 + 2] = verts[v * 3 + 2];
    }
}

// vertex_map was written by the launch before
__global__ __launch_bounds__(CC_BLOCK) void compact_emit_tris_kernel(const int32_t* __restrict__ tris, const int32_t* __restrict__ component, const uint8_t* __restrict__ keep,
                                                                     int64_t T, int64_t V, int64_t K, const uint32_t* __restrict__ block_offs,
                                                                     const int32_t* __restrict__ vertex_map, int32_t* __restrict__ out_tris, int64_t Tout) {
    __shared__ int sm[4];
    const int64_t t = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    const bool kept = t < T && tri_kept(tris, component, keep, t, V, K);
    int total;
    const int64_t pos = (int64_t)block_offs[blockIdx.x] + block_excl_scan<CC_BLOCK>(kept ? 1 : 0, sm, total);
    if (!kept || pos >= Tout) return;
#pragma unroll
    for (int c = 0; c < 3; c++) out_tris[pos * 3 + c] = vertex_map[tris[t * 3 + c]];
}

// rows of a [V, C] fp32 array to the positions vertex_map names: one lane per element
__global__ __launch_bounds__(CC_BLOCK) void compact_gather_kernel(const float* __restrict__ src, int64_t V, int C, const int32_t* __restrict__ vertex_map,
                                                                  float* __restrict__ dst, int64_t Vout) {
    const int64_t i = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x;
    if (i >= V * C) return;
    const int64_t v = i / C;
    const int c = (int)(i - v * C);
    const int m = vertex_map[v];
    if (m >= 0 && m < Vout) dst[(int64_t)m * C + c] = src[i];
}

inline bool sizes_ok(int64_t T, int64_t V) { return T >= 0 && V >= 0 && T <= (int64_t)INT32_MAX && V <= (int64_t)INT32_MAX; }
inline unsigned blocks_of(int64_t n) { return (unsigned)cdiv64(n, CC_BLOCK); }

struct CompactLayout {
    int64_t nbv, nbt, off_v, off_t, bytes;
};
inline CompactLayout compact_layout(int64_t T, int64_t V) {
    CompactLayout L;
    L.nbv = cdiv64(V, CC_BLOCK);
    L.nbt = cdiv64(T, CC_BLOCK);
    L.off_v = CC_WS_HEAD;
    L.off_t = align64(L.off_v + L.nbv * 4);
    L.bytes = align64(L.off_t + L.nbt * 4);
    return L;
}

}  // namespace

#define CC_ARGS_CHECK(name)                                                                                                                  \
    TDGP_CHECK(sizes_ok(T, V), TDGP_EINVAL, name ": T = %lld and V = %lld must lie in [0, 2^31 - 1]", (long long)T, (long long)V);       \
    TDGP_CHECK(T == 0 || tris, TDGP_EINVAL, name ": null triangles")

TDGP_API int64_t tdgp_mesh_labels_workspace_bytes(int64_t T, int64_t V) {
    if (!sizes_ok(T, V)) return -1;
    return CC_WS_HEAD + align64(V * 4);
}

TDGP_API int tdgp_mesh_labels(const int32_t* tris, int64_t T, int64_t V, int32_t* label, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    CC_ARGS_CHECK("mesh_labels");
    TDGP_CHECK(workspace && (V == 0 || label), TDGP_EINVAL, "mesh_labels: null pointer");
    TDGP_CHECK(((uintptr_t)workspace & 15) == 0, TDGP_EINVAL, "mesh_labels: workspace must be 16-byte aligned");
    const int64_t need = tdgp_mesh_labels_workspace_bytes(T, V);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EWORKSPACE, "mesh_labels: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    char* ws = (char*)workspace;
    unsigned long long* retries = (unsigned long long*)ws;
    int* parent = (int*)(ws + CC_WS_HEAD);
    hipStream_t s = (hipStream_t)stream;
    TDGP_LAUNCH("cc_init_kernel", cc_init_kernel, dim3(blocks_of(V > 0 ? V : 1)), dim3(CC_BLOCK), 0, s, parent, V, retries);
    TDGP_LAUNCH_CHECK();
    if (V == 0) return TDGP_OK;
    if (T > 0) {
        TDGP_LAUNCH("cc_union_kernel", cc_union_kernel, dim3(blocks_of(T)), dim3(CC_BLOCK), 0, s, tris, T, V, parent, retries);
        TDGP_LAUNCH_CHECK();
    }
    TDGP_LAUNCH("cc_flatten_kernel", cc_flatten_kernel, dim3(blocks_of(V)), dim3(CC_BLOCK), 0, s, (const int*)parent, label, V);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_mesh_component_ids_workspace_bytes(int64_t V) {
    if (V < 0 || V > (int64_t)INT32_MAX) return -1;
    return CC_WS_HEAD + align64(cdiv64(V, CC_BLOCK) * 4);
}

TDGP_API int tdgp_mesh_component_ids(const int32_t* label, int64_t V, int32_t* component, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= (int64_t)INT32_MAX, TDGP_EINVAL, "mesh_component_ids: V = %lld must lie in [0, 2^31 - 1]", (long long)V);
    TDGP_CHECK(workspace && (V == 0 || (label && component)), TDGP_EINVAL, "mesh_component_ids: null pointer");
    TDGP_CHECK(((uintptr_t)workspace & 15) == 0, TDGP_EINVAL, "mesh_component_ids: workspace must be 16-byte aligned");
    const int64_t need = tdgp_mesh_component_ids_workspace_bytes(V);
    TDGP_CHECK(workspace_bytes >= need, TDGP_EWORKSPACE, "mesh_component_ids: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    char* ws = (char*)workspace;
    uint32_t* sums = (uint32_t*)(ws + CC_WS_HEAD);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = cdiv64(V, CC_BLOCK);
    if (nb > 0) {
        TDGP_LAUNCH("ids_count_kernel", ids_count_kernel, dim3((unsigned)nb), dim3(CC_BLOCK), 0, s, label, V, sums);
        TDGP_LAUNCH_CHECK();
    }
    TDGP_LAUNCH("cc_scan_kernel", cc_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, (int64_t*)ws);
    TDGP_LAUNCH_CHECK();
    if (nb > 0) {
        TDGP_LAUNCH("ids_roots_kernel", ids_roots_kernel, dim3((unsigned)nb), dim3(CC_BLOCK), 0, s, label, V, (const uint32_t*)sums, component);
        TDGP_LAUNCH_CHECK();
        TDGP_LAUNCH("ids_spread_kernel", ids_spread_kernel, dim3((unsigned)nb), dim3(CC_BLOCK), 0, s, label, V, component);
        TDGP_LAUNCH_CHECK();
    }
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_component_stats(const float* vertices, const int32_t* tris, int64_t T, int64_t V, const int32_t* component, int64_t K,
                                       int64_t* tri_count, int64_t* vert_count, float* bbox_min, float* bbox_max, int32_t* tri_key, double* area_term,
                                       double* vol_term, tdgp_stream_t stream) {
    CC_ARGS_CHECK("mesh_component_stats");
    TDGP_CHECK(K >= 0 && K <= V, TDGP_EINVAL, "mesh_component_stats: K = %lld outside [0, V]", (long long)K);
    TDGP_CHECK(V == 0 || (vertices && component), TDGP_EINVAL, "mesh_component_stats: null pointer");
    TDGP_CHECK(K == 0 || (tri_count && vert_count && bbox_min && bbox_max), TDGP_EINVAL, "mesh_component_stats: null output");
    TDGP_CHECK(T == 0 || (tri_key && area_term && vol_term), TDGP_EINVAL, "mesh_component_stats: null per-triangle output");
    hipStream_t s = (hipStream_t)stream;
    if (K > 0) {
        TDGP_LAUNCH("stats_init_kernel", stats_init_kernel, dim3(blocks_of(K)), dim3(CC_BLOCK), 0, s, K, (unsigned long long*)tri_count,
                    (unsigned long long*)vert_count, (uint32_t*)bbox_min, (uint32_t*)bbox_max);
        TDGP_LAUNCH_CHECK();
        TDGP_LAUNCH("stats_verts_kernel", stats_verts_kernel, dim3((unsigned)cdiv64(V, CC_BLOCK * STATS_ITEMS)), dim3(CC_BLOCK), 0, s, vertices, component, V, K,
                    (unsigned long long*)vert_count, (uint32_t*)bbox_min, (uint32_t*)bbox_max);
        TDGP_LAUNCH_CHECK();
        TDGP_LAUNCH("stats_decode_kernel", stats_decode_kernel, dim3(blocks_of(K * 3)), dim3(CC_BLOCK), 0, s, K * 3, (uint32_t*)bbox_min, (uint32_t*)bbox_max);
        TDGP_LAUNCH_CHECK();
    }
    if (T > 0) {
        TDGP_LAUNCH("stats_tris_kernel", stats_tris_kernel, dim3((unsigned)cdiv64(T, CC_BLOCK * STATS_ITEMS)), dim3(CC_BLOCK), 0, s, vertices, tris, component, T, V, K,
                    (unsigned long long*)tri_count, tri_key, area_term, vol_term);
        TDGP_LAUNCH_CHECK();
    }
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_component_sums(const int64_t* order, const int64_t* start, const int64_t* tri_count, int64_t K, int64_t T, const double* area_term,
                                      const double* vol_term, double* area, double* volume, tdgp_stream_t stream) {
    TDGP_CHECK(K >= 0 && K <= (int64_t)INT32_MAX && T >= 0 && T <= (int64_t)INT32_MAX, TDGP_EINVAL, "mesh_component_sums: K = %lld, T = %lld outside [0, 2^31 - 1]",
               (long long)K, (long long)T);
    if (K == 0) return TDGP_OK;
    TDGP_CHECK(start && tri_count && area && volume && (T == 0 || (order && area_term && vol_term)), TDGP_EINVAL, "mesh_component_sums: null pointer");
    TDGP_LAUNCH("stats_sum_kernel", stats_sum_kernel, dim3((unsigned)K), dim3(SUM_BLOCK), 0, (hipStream_t)stream, order, start, tri_count, T, area_term, vol_term,
                area, volume);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_mesh_compact_workspace_bytes(int64_t T, int64_t V) {
    if (!sizes_ok(T, V)) return -1;
    return compact_layout(T, V).bytes;
}

TDGP_API int tdgp_mesh_compact_count(const int32_t* tris, int64_t T, int64_t V, const int32_t* component, const uint8_t* keep, int64_t K, void* workspace,
                                     int64_t workspace_bytes, tdgp_stream_t stream) {
    CC_ARGS_CHECK("mesh_compact_count");
    TDGP_CHECK(K >= 0 && K <= V, TDGP_EINVAL, "mesh_compact_count: K = %lld outside [0, V]", (long long)K);
    TDGP_CHECK(workspace && (V == 0 || component) && (K == 0 || keep), TDGP_EINVAL, "mesh_compact_count: null pointer");
    TDGP_CHECK(((uintptr_t)workspace & 15) == 0, TDGP_EINVAL, "mesh_compact_count: workspace must be 16-byte aligned");
    const CompactLayout L = compact_layout(T, V);
    TDGP_CHECK(workspace_bytes >= L.bytes, TDGP_EWORKSPACE, "mesh_compact_count: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.bytes);
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (L.nbv > 0) {
        TDGP_LAUNCH("compact_count_verts_kernel", compact_count_verts_kernel, dim3((unsigned)L.nbv), dim3(CC_BLOCK), 0, s, component, keep, V, K, (uint32_t*)(ws + L.off_v));
        TDGP_LAUNCH_CHECK();
    }
    if (L.nbt > 0) {
        TDGP_LAUNCH("compact_count_tris_kernel", compact_count_tris_kernel, dim3((unsigned)L.nbt), dim3(CC_BLOCK), 0, s, tris, component, keep, T, V, K,
                    (uint32_t*)(ws + L.off_t));
        TDGP_LAUNCH_CHECK();
    }
    TDGP_LAUNCH("cc_scan_kernel", cc_scan_kernel, dim3(1), dim3(1024), 0, s, (uint32_t*)(ws + L.off_v), L.nbv, (int64_t*)ws);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("cc_scan_kernel", cc_scan_kernel, dim3(1), dim3(1024), 0, s, (uint32_t*)(ws + L.off_t), L.nbt, (int64_t*)ws + 1);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_compact_emit(const float* vertices, const int32_t* tris, int64_t T, int64_t V, const int32_t* component, const uint8_t* keep, int64_t K,
                                    void* workspace, int64_t workspace_bytes, float* out_vertices, int64_t Vout, int32_t* out_tris, int64_t Tout,
                                    int32_t* vertex_map, const void* const* attr_in, void* const* attr_out, const int32_t* attr_channels, int num_attr,
                                    tdgp_stream_t stream) {
    CC_ARGS_CHECK("mesh_compact_emit");
    TDGP_CHECK(K >= 0 && K <= V, TDGP_EINVAL, "mesh_compact_emit: K = %lld outside [0, V]", (long long)K);
    TDGP_CHECK(workspace && (V == 0 || (component && vertices && vertex_map)) && (K == 0 || keep), TDGP_EINVAL, "mesh_compact_emit: null pointer");
    const CompactLayout L = compact_layout(T, V);
    TDGP_CHECK(workspace_bytes >= L.bytes, TDGP_EWORKSPACE, "mesh_compact_emit: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.bytes);
    TDGP_CHECK(Vout >= 0 && Tout >= 0 && Vout <= V && Tout <= T && (Vout == 0 || out_vertices) && (Tout == 0 || out_tris), TDGP_EINVAL,
               "mesh_compact_emit: bad output buffers");
    TDGP_CHECK(num_attr >= 0 && (num_attr == 0 || (attr_in && attr_out && attr_channels)), TDGP_EINVAL, "mesh_compact_emit: bad attribute list");
    for (int i = 0; i < num_attr; i++) {
        TDGP_CHECK(attr_channels[i] >= 1 && (int64_t)attr_channels[i] * V <= (int64_t)INT32_MAX, TDGP_EINVAL,
                   "mesh_compact_emit: attribute %d has %d channels (at least 1, V * C at most 2^31 - 1)", i, attr_channels[i]);
        TDGP_CHECK(V == 0 || (attr_in[i] && (Vout == 0 || attr_out[i])), TDGP_EINVAL, "mesh_compact_emit: attribute %d: null pointer", i);
    }
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (L.nbv == 0) return TDGP_OK;
    TDGP_LAUNCH("compact_emit_verts_kernel", compact_emit_verts_kernel, dim3((unsigned)L.nbv), dim3(CC_BLOCK), 0, s, vertices, component, keep, V, K,
                (const uint32_t*)(ws + L.off_v), out_vertices, Vout, vertex_map);
    TDGP_LAUNCH_CHECK();
    if (L.nbt > 0 && Tout > 0) {
        TDGP_LAUNCH("compact_emit_tris_kernel", compact_emit_tris_kernel, dim3((unsigned)L.nbt), dim3(CC_BLOCK), 0, s, tris, component, keep, T, V, K,
                    (const uint32_t*)(ws + L.off_t), (const int32_t*)vertex_map, out_tris, Tout);
        TDGP_LAUNCH_CHECK();
    }
    for (int i = 0; i < num_attr && Vout > 0; i++) {
        const int C = attr_channels[i];
        TDGP_LAUNCH("compact_gather_kernel", compact_gather_kernel, dim3(blocks_of(V * C)), dim3(CC_BLOCK), 0, s, (const float*)attr_in[i], V, C,
                    (const int32_t*)vertex_map, (float*)attr_out[i], Vout);
        TDGP_LAUNCH_CHECK();
    }
    return TDGP_OK;
}

// step_tail.hip -- what a training phase does after its backward passes (training_loop.py:334-347 of the reference) and the per-batch
// EMA update (:357-367), with a constant number of launches.
//
//   tdgp_grads_pack           torch.cat of the gradients into the flat buffer the all-reduce runs on
//   tdgp_grads_sanitise_norm  x / world, nan_to_num(nan=0, posinf=1e5, neginf=-1e5), and the 2-norm of the result (fp64)
//   tdgp_adam_step            clip coefficient from that norm + torch.optim.Adam's update on the optimiser's own state tensors
//   tdgp_ema_update           p_ema <- lerp(p, p_ema, beta) for every parameter pair, b_ema <- b for every buffer pair
//
// Every kernel is a multi-tensor kernel: block b works on ONE chunk of CHUNK elements of ONE tensor, named by the chunk -> tensor map at
// the end of the table (include/tdgp.h).  Tensors are only known to be 4-byte aligned (a gradient's slice of the flat buffer starts
// wherever the tensors before it end), so a chunk is walked as  head (< 4 scalar elements, up to the 16-byte boundary of the stream the
// kernel stores most to), body (16-byte accesses on every stream that is aligned there, four scalar accesses on the others; the choice is
// uniform over the block), tail (< 4 scalar elements).
// One writer per value, no atomics, no kernel waits on another; the sums of the norm are taken in a fixed order: same bytes on every run.
#include "common.h"

namespace {

constexpr int CHUNK = TDGP_STEP_TAIL_CHUNK;
constexpr int NT = 256;

// Pointers read from a table are generic to the compiler; they are device-memory addresses, and saying so (address space 1) keeps the
// accesses on the global path instead of the flat one.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) float4 gfloat4;
__device__ __forceinline__ gfloat* gptr(int64_t word) { return (gfloat*)(uintptr_t)word; }
__device__ __forceinline__ int head_of(const gfloat* p) { return (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2); }
__device__ __forceinline__ bool aligned16(const gfloat* p) { return ((uintptr_t)p & 15u) == 0; }

__device__ __forceinline__ float4 ld4(const gfloat* p, bool al) {
    if (al) {
        const gfloat4* q = (const gfloat4*)p;
        return make_float4(q->x, q->y, q->z, q->w);
    }
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void st4(gfloat* p, bool al, float4 v) {
    if (al) {
        typedef float vec4 __attribute__((ext_vector_type(4)));
        *(__attribute__((address_space(1))) vec4*)p = vec4{v.x, v.y, v.z, v.w};
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

// head / body / tail walk of `len` elements; f1(i) handles element i, f4(i) elements i .. i + 3.  A thread's own order is fixed.
template <class F4, class F1>
__device__ __forceinline__ void for_span(int len, int head, F4 f4, F1 f1) {
    const int tid = (int)threadIdx.x;
    head = head < len ? head : len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + (nvec << 2);
    if (tid < head) f1(tid);
    for (int i = tid; i < nvec; i += NT) f4(head + (i << 2));
    if (tid < len - tail0) f1(tail0 + tid);
}

struct Span { int t; int64_t start; int len; };
// rows: rows of the table in front of the map; n_row: the row holding the element counts
__device__ __forceinline__ Span span_of(const int64_t* __restrict__ tab, int rows, int n_row, int T, int64_t NB) {
    const int64_t b = blockIdx.x;
    Span s;
    s.t = (int)tab[(int64_t)rows * T + b];
    s.start = tab[(int64_t)rows * T + NB + b];
    const int64_t left = tab[(int64_t)n_row * T + s.t] - s.start;
    s.len = (int)(left < CHUNK ? left : CHUNK);
    return s;
}

// sum over the block in a fixed order (DPP scan inside a wave, the four wave totals added in order by thread 0); valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v) {
    __shared__ double part[NT / 64];
    v = wave_sum_f64(v);
    if (lane_id() == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
    for (int w = 1; w < NT / 64; w++) s = s + part[w];
    return s;
}

__global__ __launch_bounds__(NT) void grads_pack_kernel(const int64_t* __restrict__ gtab, const int64_t* __restrict__ tab, int T, int64_t NB,
                                                        float* __restrict__ flat) {
    const Span s = span_of(tab, 5, 3, T, NB);
    if (s.len <= 0) return;
    const gfloat* src = gptr(gtab[s.t]) + s.start;
    gfloat* dst = (gfloat*)flat + tab[4 * (int64_t)T + s.t] + s.start;
    const int head = head_of(dst);
    const bool sa = aligned16(src + head);
    for_span(s.len, head, [&](int i) { st4(dst + i, true, ld4(src + i, sa)); }, [&](int i) { dst[i] = src[i]; });
}

__device__ __forceinline__ float sanitise(float x, float world) {
    x = x / world;
    if (x != x) return 0.0f;
    if (x == INFINITY) return 1e5f;
    if (x == -INFINITY) return -1e5f;
    return x;
}

__global__ __launch_bounds__(NT) void grads_sanitise_kernel(float* __restrict__ flat, int64_t total, float world, double* __restrict__ partials) {
    const int64_t start = (int64_t)blockIdx.x * CHUNK;
    const int64_t left = total - start;
    const int len = (int)(left < CHUNK ? left : CHUNK);
    gfloat* p = (gfloat*)flat + start;
    double acc = 0.0;
    if (len > 0) {
        for_span(len, head_of(p),
                 [&](int i) {
                     float4 v = ld4(p + i, true);
                     v.x = sanitise(v.x, world); v.y = sanitise(v.y, world); v.z = sanitise(v.z, world); v.w = sanitise(v.w, world);
                     st4(p + i, true, v);
                     acc = acc + (double)v.x * (double)v.x;
                     acc = acc + (double)v.y * (double)v.y;
                     acc = acc + (double)v.z * (double)v.z;
                     acc = acc + (double)v.w * (double)v.w;
                 },
                 [&](int i) {
                     const float v = sanitise(p[i], world);
                     p[i] = v;
                     acc = acc + (double)v * (double)v;
                 });
    }
    const double s = block_sum_f64(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(NT) void grads_norm_kernel(const double* __restrict__ partials, int64_t n, double* __restrict__ norm) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += NT) acc = acc + partials[i];
    const double s = block_sum_f64(acc);
    if (threadIdx.x == 0) norm[0] = sqrt(s);
}

struct AdamArgs {
    double w1, beta2, w2, eps;                              // w1 = 1 - beta1, w2 = 1 - beta2
    double max_norm;                                        // < 0: no clipping
};

// torch.optim.Adam's update:  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g;  p += -(lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
// Each of m, v and p is evaluated in fp64 from the fp32 operands (hyper-parameters and clip coefficient as the doubles they are) and
// rounded ONCE: half an fp32 ulp from the exact update, where the eager chain of fp32 tensor ops carries one rounding per op (an fp32
// version of this function missed the tests' bound on a one-element tensor).  The kernel moves 28 bytes per element; whether the fp64
// sqrt and division hide behind that has not been measured (the step is bound by the host).  The two forms of the moving
// average are at::lerp's, so that beta1 = 0 gives m = g exactly.
struct AdamOut { float p, m, v; };
__device__ __forceinline__ AdamOut adam_one(float pf, float mf, float vf, float gf, double coef, double neg_step_size, double bc2_sqrt, const AdamArgs& a) {
    const double g = (double)gf * coef;
    const double d = g - (double)mf;
    const double m = a.w1 < 0.5 ? (double)mf + a.w1 * d : g - d * (1.0 - a.w1);
    const double v = (double)vf * a.beta2 + a.w2 * g * g;
    const double denom = sqrt(v) / bc2_sqrt + a.eps;
    const double p = (double)pf + neg_step_size * (m / denom);
    return {(float)p, (float)m, (float)v};
}

__global__ __launch_bounds__(NT) void adam_step_kernel(const int64_t* __restrict__ tab, const int64_t* __restrict__ stab, int T, int64_t NB, const float* __restrict__ flat,
                                                       const double* __restrict__ norm, AdamArgs a) {
    const Span s = span_of(tab, 5, 3, T, NB);
    if (s.len <= 0) return;
    double coef = 1.0;
    if (a.max_norm >= 0.0) {
        const double c = a.max_norm / (norm[0] + 1e-6);
        coef = c < 1.0 ? c : 1.0;
    }
    // the tensor's own step size and bias correction (tensors of one optimiser may be at different step counts)
    const double nss = __longlong_as_double(stab[(int64_t)T + s.t]), bc2s = __longlong_as_double(stab[2 * (int64_t)T + s.t]);
    gfloat* p = gptr(tab[s.t]) + s.start;
    gfloat* m = gptr(tab[(int64_t)T + s.t]) + s.start;
    gfloat* v = gptr(tab[2 * (int64_t)T + s.t]) + s.start;
    const gfloat* g = (const gfloat*)flat + tab[4 * (int64_t)T + s.t] + s.start;
    const int head = head_of(p);
    const bool ma = aligned16(m + head), va = aligned16(v + head), ga = aligned16(g + head);
    for_span(s.len, head,
             [&](int i) {
                 float4 P = ld4(p + i, true), M = ld4(m + i, ma), V = ld4(v + i, va);
                 const float4 G = ld4(g + i, ga);
                 const AdamOut x = adam_one(P.x, M.x, V.x, G.x, coef, nss, bc2s, a), y = adam_one(P.y, M.y, V.y, G.y, coef, nss, bc2s, a),
                               z = adam_one(P.z, M.z, V.z, G.z, coef, nss, bc2s, a), w = adam_one(P.w, M.w, V.w, G.w, coef, nss, bc2s, a);
                 st4(p + i, true, make_float4(x.p, y.p, z.p, w.p));
                 st4(m + i, ma, make_float4(x.m, y.m, z.m, w.m));
                 st4(v + i, va, make_float4(x.v, y.v, z.v, w.v));
             },
             [&](int i) {
                 const AdamOut x = adam_one(p[i], m[i], v[i], g[i], coef, nss, bc2s, a);
                 p[i] = x.p; m[i] = x.m; v[i] = x.v;
             });
}

// at::lerp(self = p, end = p_ema, weight = beta), evaluated in fp64 and rounded once
__device__ __forceinline__ float ema_one(float p, float pe, double beta) {
    const double d = (double)pe - (double)p;
    return (float)(beta < 0.5 ? (double)p + beta * d : (double)pe - d * (1.0 - beta));
}

__global__ __launch_bounds__(NT) void ema_update_kernel(const int64_t* __restrict__ tab, int T, int64_t NB, double beta, int copy_all) {
    const Span s = span_of(tab, 4, 2, T, NB);
    if (s.len <= 0) return;
    const gfloat* src = gptr(tab[s.t]) + s.start;
    gfloat* dst = gptr(tab[(int64_t)T + s.t]) + s.start;
    const bool copy = copy_all || tab[3 * (int64_t)T + s.t] != 0;
    const int head = head_of(dst);
    const bool sa = aligned16(src + head);
    if (copy) {
        for_span(s.len, head, [&](int i) { st4(dst + i, true, ld4(src + i, sa)); }, [&](int i) { dst[i] = src[i]; });
    } else {
        for_span(s.len, head,
                 [&](int i) {
                     const float4 a = ld4(src + i, sa), e = ld4(dst + i, true);
                     st4(dst + i, true, make_float4(ema_one(a.x, e.x, beta), ema_one(a.y, e.y, beta), ema_one(a.z, e.z, beta), ema_one(a.w, e.w, beta)));
                 },
                 [&](int i) { dst[i] = ema_one(src[i], dst[i], beta); });
    }
}

bool table_args_ok(const void* table, int T, int64_t NB, int chunk, const char* what) {
    if (chunk != CHUNK) {
        tdgp_set_error("%s: chunk %d, this library was built with TDGP_STEP_TAIL_CHUNK = %d", what, chunk, CHUNK);
        return false;
    }
    if (!table || T < 1 || NB < 1 || NB < T || NB > 0x7fffffffll) {
        tdgp_set_error("%s: bad table (null, or not 1 <= num_tensors <= num_blocks < 2^31)", what);
        return false;
    }
    return true;
}

}  // namespace

TDGP_API int tdgp_grads_pack(const int64_t* grad_table, const int64_t* table, int num_tensors, int64_t num_blocks, int chunk, float* flat,
                             int64_t total, tdgp_stream_t stream) {
    if (!table_args_ok(table, num_tensors, num_blocks, chunk, "grads_pack")) return TDGP_EINVAL;
    TDGP_CHECK(grad_table && flat && total >= 1, TDGP_EINVAL, "grads_pack: null pointer or empty flat buffer");
    TDGP_CHECK(num_blocks <= cdiv64(total, CHUNK) + num_tensors, TDGP_EINVAL, "grads_pack: more blocks than %lld elements in %d tensors can have",
               (long long)total, num_tensors);
    TDGP_LAUNCH("grads_pack_kernel", grads_pack_kernel, dim3((unsigned)num_blocks), dim3(NT), 0, (hipStream_t)stream, grad_table, table, num_tensors,
                num_blocks, flat);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_grads_sanitise_norm(float* flat, int64_t total, int world, int chunk, double* partials, int64_t num_partials, double* norm,
                                      tdgp_stream_t stream) {
    TDGP_CHECK(chunk == CHUNK, TDGP_EINVAL, "grads_sanitise_norm: chunk %d, this library was built with TDGP_STEP_TAIL_CHUNK = %d", chunk, CHUNK);
    TDGP_CHECK(flat && partials && norm, TDGP_EINVAL, "grads_sanitise_norm: null pointer");
    TDGP_CHECK(total >= 1 && world >= 1, TDGP_EINVAL, "grads_sanitise_norm: total and world must be >= 1");
    TDGP_CHECK(num_partials == cdiv64(total, CHUNK) && num_partials <= 0x7fffffffll, TDGP_EINVAL,
               "grads_sanitise_norm: num_partials must be ceil(total / chunk) and below 2^31");
    TDGP_LAUNCH("grads_sanitise_kernel", grads_sanitise_kernel, dim3((unsigned)num_partials), dim3(NT), 0, (hipStream_t)stream, flat, total, (float)world,
                partials);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("grads_norm_kernel", grads_norm_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const double*)partials, num_partials, norm);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_adam_step(const int64_t* table, const int64_t* step_table, int num_tensors, int64_t num_blocks, int chunk, const float* flat,
                            int64_t total, const double* norm, double max_norm, double beta1, double beta2, double eps, tdgp_stream_t stream) {
    if (!table_args_ok(table, num_tensors, num_blocks, chunk, "adam_step")) return TDGP_EINVAL;
    TDGP_CHECK(step_table && flat && total >= 1, TDGP_EINVAL, "adam_step: null pointer or empty flat buffer");
    TDGP_CHECK(num_blocks <= cdiv64(total, CHUNK) + num_tensors, TDGP_EINVAL, "adam_step: more blocks than %lld elements in %d tensors can have",
               (long long)total, num_tensors);
    TDGP_CHECK(max_norm < 0.0 || norm, TDGP_EINVAL, "adam_step: clipping needs the norm");
    TDGP_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, TDGP_EINVAL, "adam_step: betas in [0, 1) and eps >= 0 expected");
    AdamArgs a;
    a.w1 = 1.0 - beta1;
    a.beta2 = beta2;
    a.w2 = 1.0 - beta2;
    a.eps = eps;
    a.max_norm = max_norm;
    TDGP_LAUNCH("adam_step_kernel", adam_step_kernel, dim3((unsigned)num_blocks), dim3(NT), 0, (hipStream_t)stream, table, step_table, num_tensors,
                num_blocks, flat, norm, a);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_ema_update(const int64_t* table, int num_tensors, int64_t num_blocks, int chunk, double beta, tdgp_stream_t stream) {
    if (!table_args_ok(table, num_tensors, num_blocks, chunk, "ema_update")) return TDGP_EINVAL;
    TDGP_CHECK(beta >= 0.0 && beta <= 1.0, TDGP_EINVAL, "ema_update: beta in [0, 1] expected");
    TDGP_LAUNCH("ema_update_kernel", ema_update_kernel, dim3((unsigned)num_blocks), dim3(NT), 0, (hipStream_t)stream, table, num_tensors, num_blocks,
                beta, beta == 0.0 ? 1 : 0);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

// device_scan.h -- the integer scans behind every "count, scan, emit" compaction (marching cubes in geometry.hip, dense ids and the filter in
// mesh_components.hip), and the ordered-bits float key (mesh_components.hip, metrics.hip).  Positions come from scans alone, never from
// atomics: a block-local scan of BLOCK values, ONE block scanning the block sums, block-local scan + block offset -- so every output is the
// same bytes on every run.  Everything here is inlined into its caller.
#pragma once
#include "common.h"

static inline int64_t align64(int64_t x) { return (x + 63) & ~(int64_t)63; }

__device__ __forceinline__ int wave_incl_scan_i32(int v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane_id() >= d) v += o;
    }
    return v;
}

template <int W>
__device__ __forceinline__ int sum_ints(const int* p) {
    if constexpr (W == 1) return p[0];
    else return sum_ints<W - 1>(p) + p[W - 1];
}

// exclusive prefix of `v` over the block's BLOCK threads (thread order); `total` = the block's sum.  `sm` holds BLOCK / 64 ints.
template <int BLOCK>
__device__ __forceinline__ int block_excl_scan(int v, int* sm, int& total) {
    static_assert(BLOCK % 64 == 0, "whole waves");
    const int incl = wave_incl_scan_i32(v);
    const int wv = threadIdx.x >> 6;
    __syncthreads();                               // `sm` may still be read from an earlier scan
    if (lane_id() == 63) sm[wv] = incl;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / 64; i++) base += (i < wv) ? sm[i] : 0;
    total = sum_ints<BLOCK / 64>(sm);
    return base + incl - v;
}

// Body of a kernel of ONE block of 1024 threads: exclusive scan, in place, of the sums that nb blocks left for N interleaved counters
// (counter c of block b at block_sums[N * b + c]); totals[c] = the grand total of counter c.  Thread t takes the contiguous run
// [t * per, (t + 1) * per) of blocks.  The offsets are exact as long as every total fits 32 bits, which the callers' size checks see to.
template <int N>
__device__ __forceinline__ void scan_block_sums(uint32_t* __restrict__ block_sums, int64_t nb, int64_t* __restrict__ totals) {
    __shared__ unsigned long long part[N][1024];
    const int t = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b0 = min((int64_t)t * per, nb), b1 = min(b0 + per, nb);
    struct Row { uint32_t c[N]; };                 // the N counters of a block: one load, one store
    Row* const rows = reinterpret_cast<Row*>(block_sums);
    unsigned long long s[N];
#pragma unroll
    for (int c = 0; c < N; c++) s[c] = 0;
    for (int64_t b = b0; b < b1; b++) {
        const Row r = rows[b];
#pragma unroll
        for (int c = 0; c < N; c++) s[c] += r.c[c];
    }
#pragma unroll
    for (int c = 0; c < N; c++) part[c][t] = s[c];
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {           // Hillis-Steele over the 1024 partial sums
        unsigned long long a[N];
#pragma unroll
        for (int c = 0; c < N; c++) a[c] = 0;
        if (t >= d) {
#pragma unroll
            for (int c = 0; c < N; c++) a[c] = part[c][t - d];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < N; c++) part[c][t] += a[c];
        __syncthreads();
    }
    unsigned long long e[N];
#pragma unroll
    for (int c = 0; c < N; c++) e[c] = part[c][t] - s[c];
    for (int64_t b = b0; b < b1; b++) {
        const Row r = rows[b];
        Row w;
#pragma unroll
        for (int c = 0; c < N; c++) w.c[c] = (uint32_t)e[c];
        rows[b] = w;
#pragma unroll
        for (int c = 0; c < N; c++) e[c] += r.c[c];
    }
    if (t == 1023) {
#pragma unroll
        for (int c = 0; c < N; c++) totals[c] = (int64_t)part[c][1023];
    }
}

// floats as unsigned keys whose integer order is the floats' order (-0 below +0), and back; f32_bits_key for a caller that holds the bits
__device__ __forceinline__ uint32_t f32_bits_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t f32_key(float f) { return f32_bits_key(__float_as_uint(f)); }
__device__ __forceinline__ float key_f32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

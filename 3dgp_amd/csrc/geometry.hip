// geometry.hip -- shape extraction: the voxel grid of scripts/extract_geometry.py and marching cubes, on the device.
//
// Replaces (CPU / third-party in the reference):
//   scripts/extract_geometry.py:55-76   create_voxel_coords (torch CPU ops over the whole res^3 grid, then a host-to-device copy)
//   scripts/extract_geometry.py:38-40   mcubes.marching_cubes on a host copy of the density grid
//
// Marching cubes is four plain launches over the grid points of a [D,H,W] volume, 256 points per block, no kernel waiting on another:
//   mc_count_kernel       one thread per grid point: the 8-bit case of the cell whose lower corner it is, the sign-changing edges it OWNS
//                         (the up-to-three edges leaving it toward +d, +h, +w: every edge of the volume has exactly one owner, boundary
//                         points own the edges that exist), a 2-byte code per point and the block's vertex / triangle sums
//   mc_scan_kernel        ONE block: exclusive scan of the per-block sums, grand totals (the only numbers the host reads back)
//   mc_emit_verts_kernel  block-local scan + block offset -> every owned edge's vertex id and position; the id of a point's first
//                         vertex is kept (with the ranks of its h / w edges) for the cells around it
//   mc_emit_tris_kernel   block-local scan + block offset -> triangles through the case table, indexed into the shared vertices
// Positions in the outputs are decided by the scans alone (no atomics): vertices ordered by owning grid point then axis (d, h, w),
// triangles by cell then table order, bit-identical from run to run.  Winding: normals point toward lower values (mc_table.inc).
#include "common.h"
#include "device_scan.h"
#define MC_TABLE_QUAL __device__ const __attribute__((aligned(16)))
#include "mc_table.inc"

namespace {

constexpr int MC_BLOCK = 256;                 // grid points per block (4 waves)
constexpr int64_t MC_WS_HEAD = 64;            // bytes in front of the block sums: totals (V, T) as two int64
constexpr uint32_t MC_VID_MAX = 1u << 29;     // vertex ids are kept as id << 3 | rank bits in one uint32

// exactly the reference's chain: index -> fp32, two unfloored fp32 divisions, torch.remainder (fmod for non-negative operands), then
// `* voxel_size + origin` as two roundings.  z comes from the INTEGER remainder (coords[:, 2] = overall_index % resolution).
__global__ __launch_bounds__(256) void voxel_coords_kernel(float* __restrict__ out, int64_t i0, int64_t n, int res, float vs, float ox, float oy,
                                                          float oz) {
    const float r = (float)res;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t idx = i0 + k;
        const float f = (float)idx;
        const float z = (float)(idx % res);
        const float q = f / r;
        const float y = fmodf(q, r);
        const float x = fmodf(q / r, r);
        out[k * 3 + 0] = x * vs + ox;
        out[k * 3 + 1] = y * vs + oy;
        out[k * 3 + 2] = z * vs + oz;
    }
}

// code of a grid point: bits 0-7 the case of its cell (0 where it has none), bits 8-10 its owned sign-changing edges along d / h / w
__device__ __forceinline__ int popc3(int f) { return (f & 1) + ((f >> 1) & 1) + ((f >> 2) & 1); }

__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(const float* __restrict__ vol, int D, int H, int W, float thresh,
                                                            uint16_t* __restrict__ code, uint32_t* __restrict__ block_sums, int64_t N) {
    __shared__ unsigned char ntri_s[256];
    __shared__ int sm[4];
    ntri_s[threadIdx.x] = MC_TABLE[threadIdx.x][0];
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)MC_BLOCK + threadIdx.x;
    int nv = 0, nt = 0;
    if (i < N) {
        const int64_t HW = (int64_t)H * W;
        const int w = (int)(i % W), h = (int)((i / W) % H), d = (int)(i / HW);
        const bool hd = d + 1 < D, hh = h + 1 < H, hw = w + 1 < W;
        const bool in0 = vol[i] >= thresh;
        // neighbours are read only where they exist
        const bool i001 = hw ? vol[i + 1] >= thresh : in0;
        const bool i010 = hh ? vol[i + W] >= thresh : in0;
        const bool i100 = hd ? vol[i + HW] >= thresh : in0;
        const int flags = (int)(i100 != in0) | ((int)(i010 != in0) << 1) | ((int)(i001 != in0) << 2);
        int cs = 0;
        if (hd && hh && hw) {
            cs = (int)in0 | ((int)i001 << 1) | ((int)i010 << 2) | ((int)(vol[i + W + 1] >= thresh) << 3) | ((int)i100 << 4) |
                 ((int)(vol[i + HW + 1] >= thresh) << 5) | ((int)(vol[i + HW + W] >= thresh) << 6) | ((int)(vol[i + HW + W + 1] >= thresh) << 7);
        }
        code[i] = (uint16_t)(cs | (flags << 8));
        nv = popc3(flags);
        nt = ntri_s[cs];
    }
    int tv, tt;
    block_excl_scan<MC_BLOCK>(nv, sm, tv);
    block_excl_scan<MC_BLOCK>(nt, sm, tt);
    if (threadIdx.x == 0) {
        block_sums[2 * (int64_t)blockIdx.x + 0] = (uint32_t)tv;
        block_sums[2 * (int64_t)blockIdx.x + 1] = (uint32_t)tt;
    }
}

// one block of 1024 threads over the (vertex, triangle) sums of every block: totals[0] = V, totals[1] = T
__global__ __launch_bounds__(1024) void mc_scan_kernel(uint32_t* __restrict__ block_sums, int64_t nb, int64_t* __restrict__ totals) {
    scan_block_sums<2>(block_sums, nb, totals);
}

__global__ __launch_bounds__(MC_BLOCK) void mc_emit_verts_kernel(const float* __restrict__ vol, int D, int H, int W, float thresh,
                                                                 const uint16_t* __restrict__ code, const uint32_t* __restrict__ block_offs,
                                                                 uint32_t* __restrict__ vid, float* __restrict__ verts, int64_t V, int64_t N) {
    __shared__ int sm[4];
    const int64_t i = blockIdx.x * (int64_t)MC_BLOCK + threadIdx.x;
    const int flags = i < N ? (code[i] >> 8) & 7 : 0;
    int total;
    const int64_t first = (int64_t)block_offs[2 * (int64_t)blockIdx.x] + block_excl_scan<MC_BLOCK>(popc3(flags), sm, total);
    if (i >= N) return;
    // rank of the h edge = (d edge present), rank of the w edge = (d edge) + (h edge)
    vid[i] = ((uint32_t)first << 3) | (uint32_t)(flags & 1) | ((uint32_t)((flags & 1) + ((flags >> 1) & 1)) << 1);
    if (!flags) return;
    const int64_t HW = (int64_t)H * W;
    const int w = (int)(i % W), h = (int)((i / W) % H), d = (int)(i / HW);
    const float v0 = vol[i];
    const float p[3] = {(float)d, (float)h, (float)w};
    const int64_t step[3] = {HW, (int64_t)W, 1};
    int64_t id = first;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!((flags >> a) & 1)) continue;
        const float v1 = vol[i + step[a]];          // the flag is only set where this neighbour exists
        const float t = (thresh - v0) / (v1 - v0);
        if (id < V) {                               // V is the caller's: never write past the buffer it sized
            verts[id * 3 + 0] = a == 0 ? p[0] + t : p[0];
            verts[id * 3 + 1] = a == 1 ? p[1] + t : p[1];
            verts[id * 3 + 2] = a == 2 ? p[2] + t : p[2];
        }
        id++;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_emit_tris_kernel(int H, int W, const uint16_t* __restrict__ code, const uint32_t* __restrict__ block_offs,
                                                                const uint32_t* __restrict__ vid, int32_t* __restrict__ tris, int64_t T, int64_t N) {
    __shared__ __attribute__((aligned(16))) unsigned char tab_s[256][16];
    __shared__ int sm[4];
    {
        const uint4* src = reinterpret_cast<const uint4*>(&MC_TABLE[0][0]);
        reinterpret_cast<uint4*>(&tab_s[0][0])[threadIdx.x] = src[threadIdx.x];       // 256 rows of 16 bytes, one per thread
    }
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)MC_BLOCK + threadIdx.x;
    const int cs = i < N ? code[i] & 255 : 0;
    const int nt = tab_s[cs][0];
    int total;
    int64_t tid = (int64_t)block_offs[2 * (int64_t)blockIdx.x + 1] + block_excl_scan<MC_BLOCK>(nt, sm, total);
    if (!nt) return;                                // a non-zero case only exists where the whole cell does
    const int64_t HW = (int64_t)H * W;
    for (int k = 0; k < nt; k++, tid++) {
        int32_t ids[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int e = tab_s[cs][1 + 3 * k + c];
            const int axis = e >> 2, xb = (e >> 1) & 1, xc = e & 1;
            // offset of the edge's owner (its lower corner): the two non-axis coordinates in ascending axis order
            const int dd = axis == 0 ? 0 : xb, dh = axis == 0 ? xb : (axis == 1 ? 0 : xc), dw = axis == 2 ? 0 : xc;
            const uint32_t o = vid[i + dd * HW + dh * (int64_t)W + dw];
            const int rank = axis == 0 ? 0 : (axis == 1 ? (int)(o & 1) : (int)((o >> 1) & 3));
            ids[c] = (int32_t)((o >> 3) + rank);
        }
        if (tid < T) {
            tris[tid * 3 + 0] = ids[0];
            tris[tid * 3 + 1] = ids[1];
            tris[tid * 3 + 2] = ids[2];
        }
    }
}

struct McLayout {
    int64_t N, nb, off_sums, off_code, off_vid, bytes;
};
inline McLayout mc_layout(int D, int H, int W) {
    McLayout L;
    L.N = (int64_t)D * H * W;
    L.nb = cdiv64(L.N, MC_BLOCK);
    L.off_sums = MC_WS_HEAD;
    L.off_code = align64(L.off_sums + L.nb * 8);
    L.off_vid = align64(L.off_code + L.N * 2);
    L.bytes = align64(L.off_vid + L.N * 4);
    return L;
}
inline bool mc_shape_ok(int D, int H, int W) {
    return D >= 2 && H >= 2 && W >= 2 && (int64_t)D * H * W <= (int64_t)INT32_MAX;
}

}  // namespace

TDGP_API int tdgp_voxel_coords(float* coords, int64_t i0, int64_t n, int res, float voxel_size, float origin_x, float origin_y, float origin_z,
                               tdgp_stream_t stream) {
    TDGP_CHECK(coords, TDGP_EINVAL, "voxel_coords: null pointer");
    TDGP_CHECK(res >= 2 && res <= 2048, TDGP_EINVAL, "voxel_coords: resolution %d outside [2, 2048]", res);
    TDGP_CHECK(i0 >= 0 && n >= 0 && i0 + n <= (int64_t)res * res * res, TDGP_EINVAL, "voxel_coords: indices [%lld, %lld) outside the %d^3 grid",
               (long long)i0, (long long)(i0 + n), res);
    if (n == 0) return TDGP_OK;
    TDGP_LAUNCH("voxel_coords_kernel", voxel_coords_kernel, dim3((int)min((int64_t)4096, cdiv64(n, 256))), dim3(256), 0, (hipStream_t)stream, coords, i0, n,
                res, voxel_size, origin_x, origin_y, origin_z);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int64_t tdgp_mcubes_workspace_bytes(int D, int H, int W) {
    if (!mc_shape_ok(D, H, W)) return -1;
    return mc_layout(D, H, W).bytes;
}

TDGP_API int tdgp_mcubes_count(const float* volume, int D, int H, int W, float thresh, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream) {
    TDGP_CHECK(volume && workspace, TDGP_EINVAL, "mcubes_count: null pointer");
    TDGP_CHECK(mc_shape_ok(D, H, W), TDGP_EINVAL, "mcubes_count: volume [%d,%d,%d] needs every side >= 2 and at most 2^31 - 1 points", D, H, W);
    TDGP_CHECK(((uintptr_t)workspace & 15) == 0, TDGP_EINVAL, "mcubes_count: workspace must be 16-byte aligned");
    const McLayout L = mc_layout(D, H, W);
    TDGP_CHECK(workspace_bytes >= L.bytes, TDGP_EINVAL, "mcubes_count: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.bytes);
    char* ws = (char*)workspace;
    TDGP_LAUNCH("mc_count_kernel", mc_count_kernel, dim3((unsigned)L.nb), dim3(MC_BLOCK), 0, (hipStream_t)stream, volume, D, H, W, thresh,
                (uint16_t*)(ws + L.off_code), (uint32_t*)(ws + L.off_sums), L.N);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("mc_scan_kernel", mc_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (uint32_t*)(ws + L.off_sums), L.nb, (int64_t*)ws);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mcubes_emit(const float* volume, int D, int H, int W, float thresh, void* workspace, int64_t workspace_bytes, float* vertices,
                              int64_t V, int32_t* triangles, int64_t T, tdgp_stream_t stream) {
    TDGP_CHECK(volume && workspace, TDGP_EINVAL, "mcubes_emit: null pointer");
    TDGP_CHECK(mc_shape_ok(D, H, W), TDGP_EINVAL, "mcubes_emit: volume [%d,%d,%d] needs every side >= 2 and at most 2^31 - 1 points", D, H, W);
    const McLayout L = mc_layout(D, H, W);
    TDGP_CHECK(workspace_bytes >= L.bytes, TDGP_EINVAL, "mcubes_emit: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.bytes);
    TDGP_CHECK(V >= 0 && T >= 0 && (V == 0 || vertices) && (T == 0 || triangles), TDGP_EINVAL, "mcubes_emit: bad output buffers");
    TDGP_CHECK(V < (int64_t)MC_VID_MAX && T <= (int64_t)INT32_MAX, TDGP_EUNSUPPORTED, "mcubes_emit: %lld vertices / %lld triangles exceed the 2^29 / 2^31 "
               "this build indexes; extract the volume in parts", (long long)V, (long long)T);
    if (V == 0 && T == 0) return TDGP_OK;
    char* ws = (char*)workspace;
    TDGP_LAUNCH("mc_emit_verts_kernel", mc_emit_verts_kernel, dim3((unsigned)L.nb), dim3(MC_BLOCK), 0, (hipStream_t)stream, volume, D, H, W, thresh,
                (const uint16_t*)(ws + L.off_code), (const uint32_t*)(ws + L.off_sums), (uint32_t*)(ws + L.off_vid), vertices, V, L.N);
    TDGP_LAUNCH_CHECK();
    TDGP_LAUNCH("mc_emit_tris_kernel", mc_emit_tris_kernel, dim3((unsigned)L.nb), dim3(MC_BLOCK), 0, (hipStream_t)stream, H, W,
                (const uint16_t*)(ws + L.off_code), (const uint32_t*)(ws + L.off_sums), (const uint32_t*)(ws + L.off_vid), triangles, T, L.N);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

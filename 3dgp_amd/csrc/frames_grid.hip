// frames_grid.hip -- ray-major fp32 frames -> uint8 image grids [images, GH, GW, 3], the block a video / image encoder takes.
//
// Replaces (torch CPU ops + torchvision in the reference, on fp32 CHW images fetched from the device):
//   src/training/inference_utils.py:113-117   depth normalisation, clamp(-1, 1) * 0.5 + 0.5
//   scripts/inference.py:66,74-75             make_grid(nrow, padding=2, pad_value=0) / torch.cat(dim=3), (x * 255).to(uint8), permute to [T,H,W,C]
// One streaming kernel: 4 bytes read per channel value, 1 written; no workspace, no atomics, one writer per output dword, so the same bytes
// come out on every run.  The fp32 chain is the CPU one, each operation rounded once (the library is built with -ffp-contract=off and `/` is
// the correctly rounded division).
#include "common.h"

namespace {

struct GridGeom {
    int h, w, C;              // source frame: h x w rays of C floats
    int GH, GW;               // one output image
    int pad;                  // 0 for a single tile
    int xmaps, tiles;
    int64_t stride_image, stride_tile;
    int normalise;
    float mid, range;
};

__device__ __forceinline__ uint32_t to_byte(float x, const GridGeom& g) {
    float y = x;
    if (g.normalise) y = ((x - g.mid) / g.range) * 2.0f;
    y = y < -1.0f ? -1.0f : y;                     // comparisons leave a NaN in place, as torch.clamp does
    y = y > 1.0f ? 1.0f : y;
    const float z = y * 0.5f + 0.5f;
    const float s = z * 255.0f;
    return s == s ? (uint32_t)(int)s : 0u;         // z in [0, 1]: the cast truncates; NaN -> 0 by definition
}

// Where a grid row / column falls: shifted by one tile so that the leading padding needs no signed division -- (y + h) / (h + pad) is the
// tile row + 1 and the remainder the row inside the tile (>= h: padding); columns likewise.
struct Pos { int t, r; };
__device__ __forceinline__ Pos locate(int v, int size, int pad) {
    const uint32_t s = (uint32_t)(v + size), period = (uint32_t)(size + pad);
    const uint32_t t = s / period;
    return Pos{(int)t, (int)(s - t * period)};
}

// One block = one grid row at a time, one lane = one aligned dword of the flat output.  Rows are GW * 3 bytes with any residue mod 4, so the
// dwords are not aligned to rows: a row owns the dwords whose first byte lies in it, and the lane of its last dword runs on into the next row
// (or image).  What is per row (image, tile row) is computed once per block from uniform values; a lane locates its first byte with one
// division by the tile period and finds the next three by stepping -- located per byte by division, 64-bit per dword, this kernel was bound
// by its integer arithmetic at a third of the copy rate.  The last total % 4 bytes of the buffer are written as single bytes.
// IDX = uint32_t when the output has fewer than 2^32 rows and bytes.
template <typename IDX>
__global__ __launch_bounds__(256) void frames_to_grid_u8_kernel(const float* __restrict__ frames, uint8_t* __restrict__ out, GridGeom g, int64_t total, int64_t rows) {
    const int row_bytes = g.GW * 3;
    const int64_t frame_floats = (int64_t)g.h * g.w * g.C;
    for (int64_t R = blockIdx.x; R < rows; R += gridDim.x) {
        const int64_t img0 = (int64_t)((IDX)R / (IDX)g.GH);
        const int y0 = (int)(R - img0 * g.GH);
        const Pos row0 = locate(y0, g.h, g.pad);
        const int64_t row_start = R * row_bytes, row_end = row_start + row_bytes;
        for (int64_t d = ((row_start + 3) >> 2) + threadIdx.x; (d << 2) < row_end; d += blockDim.x) {
            const int64_t b0 = d << 2;
            int64_t img = img0;
            int y = y0;
            Pos row = row0;
            const int xb = (int)(b0 - row_start);
            int x = xb / 3, c = xb - 3 * x;
            Pos col = locate(x, g.w, g.pad);
            const int n = (int)((total - b0) < 4 ? (total - b0) : 4);
            // the four loads are issued back to back (a byte outside every tile reads frames[0] and is dropped): behind a branch each, the
            // lane would wait out four memory latencies in turn
            float val[4];
            bool inside[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int k = (row.t - 1) * g.xmaps + (col.t - 1);
                // inside a tile (col.t <= xmaps and row.t <= ymaps follow from x < GW, y < GH), and not an empty cell of a ragged last row
                inside[j] = j < n && row.t >= 1 && col.t >= 1 && row.r < g.h && col.r < g.w && k < g.tiles;
                const int64_t f = img * g.stride_image + (int64_t)k * g.stride_tile;
                const int64_t at = f * frame_floats + (int64_t)(row.r * g.w + col.r) * g.C + (g.C == 1 ? 0 : c);
                val[j] = frames[inside[j] ? at : 0];
                if (++c == 3) {
                    c = 0;
                    if (++x == g.GW) {                                           // the dword runs into the next row (or image)
                        x = 0;
                        if (++y == g.GH) { y = 0; img++; }
                        row = locate(y, g.h, g.pad);
                        col = locate(0, g.w, g.pad);
                    } else if (++col.r == g.w + g.pad) {
                        col.r = 0;
                        col.t++;
                    }
                }
            }
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) v |= (inside[j] ? to_byte(val[j], g) : 0u) << (8 * j);
            if (n == 4) {
                *reinterpret_cast<uint32_t*>(out + b0) = v;
            } else {
                for (int j = 0; j < n; j++) out[b0 + j] = (uint8_t)(v >> (8 * j));
            }
        }
    }
}

}  // namespace

TDGP_API int tdgp_frames_to_grid_u8(const float* frames, int64_t num_frames, int h, int w, int C, uint8_t* out, int images, int tiles,
                                    int64_t stride_image, int64_t stride_tile, int nrow, int padding, int normalise, float mid, float range,
                                    tdgp_stream_t stream) {
    TDGP_CHECK(frames && out, TDGP_EINVAL, "frames_to_grid_u8: null pointer");
    TDGP_CHECK(((uintptr_t)out & 3) == 0 && ((uintptr_t)frames & 3) == 0, TDGP_EINVAL, "frames_to_grid_u8: frames and out must be 4-byte aligned");
    TDGP_CHECK(C == 1 || C == 3, TDGP_EINVAL, "frames_to_grid_u8: C must be 1 or 3");
    TDGP_CHECK(h >= 1 && w >= 1 && images >= 1 && tiles >= 1 && nrow >= 1 && padding >= 0 && num_frames >= 1, TDGP_EINVAL, "frames_to_grid_u8: bad shape");
    TDGP_CHECK(stride_image >= 0 && stride_tile >= 0, TDGP_EINVAL, "frames_to_grid_u8: negative stride");
    TDGP_CHECK((double)(images - 1) * (double)stride_image + (double)(tiles - 1) * (double)stride_tile < (double)num_frames, TDGP_EINVAL,
               "frames_to_grid_u8: source frame index out of range");
    GridGeom g;
    g.h = h; g.w = w; g.C = C; g.tiles = tiles;
    g.xmaps = nrow < tiles ? nrow : tiles;
    const int ymaps = cdiv(tiles, g.xmaps);
    g.pad = tiles == 1 ? 0 : padding;
    const int64_t GH = tiles == 1 ? (int64_t)h : ((int64_t)h + padding) * ymaps + padding;
    const int64_t GW = tiles == 1 ? (int64_t)w : ((int64_t)w + padding) * g.xmaps + padding;
    TDGP_CHECK(GH * GW * 3 < ((int64_t)1 << 31) && (int64_t)h + padding < ((int64_t)1 << 30) && (int64_t)w + padding < ((int64_t)1 << 30), TDGP_EINVAL,
               "frames_to_grid_u8: one output image must stay below 2^31 bytes");
    TDGP_CHECK((int64_t)h * w < ((int64_t)1 << 31) && (double)num_frames * h * w * C < 9.0e18 && (double)images * (double)(GH * GW * 3) < 9.0e18, TDGP_EINVAL, "frames_to_grid_u8: tensor too large");
    g.GH = (int)GH; g.GW = (int)GW;
    g.stride_image = stride_image; g.stride_tile = stride_tile;
    g.normalise = normalise ? 1 : 0; g.mid = mid; g.range = range;
    const int64_t total = (int64_t)images * GH * GW * 3;
    const int64_t rows = (int64_t)images * GH;
    const dim3 grid((int)min((int64_t)262144, rows));
    if (total < ((int64_t)1 << 32)) {
        TDGP_LAUNCH("frames_to_grid_u8_kernel", frames_to_grid_u8_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream, frames, out, g, total, rows);
    } else {
        TDGP_LAUNCH("frames_to_grid_u8_kernel", frames_to_grid_u8_kernel<uint64_t>, grid, dim3(256), 0, (hipStream_t)stream, frames, out, g, total, rows);
    }
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

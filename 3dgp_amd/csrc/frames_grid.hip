// frames_grid.hip -- ray-major fp32 frames -> uint8 image grids [images, GH, GW, 3], the block a video / image encoder takes.
//
// Replaces (torch CPU ops + torchvision in the reference, on fp32 CHW images fetched from the device):
//   src/training/inference_utils.py:113-117   depth normalisation, clamp(-1, 1) * 0.5 + 0.5
//   scripts/inference.py:66,74-75             make_grid(nrow, padding=2, pad_value=0) / torch.cat(dim=3), (x * 255).to(uint8), permute to [T,H,W,C]
// One streaming kernel: 4 bytes read per channel value, 1 written; no workspace, no atomics, one writer per output dword, so the same bytes
// come out on every run.  The fp32 chain is the CPU one, each operation rounded once (the library is built with -ffp-contract=off and `/` is
// the correctly rounded division).
//
// Also here: ppl_frames_kernel (tdgp_ppl_frames), the fp32 image tail of the perceptual path length from the same ray-major frames
//   src/metrics/perceptual_path_length.py:71-85   centre crop, box mean to 256^2, (x + 1) * 127.5, grey replicated
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

// The image tail of the perceptual path length (src/metrics/perceptual_path_length.py:71-85 behind the reshape of networks_epigraf.py:242):
// centre crop, factor x factor box mean, (x + 1) * 127.5, grey replicated -- one thread per output pixel, all three channels.  The box is
// summed in fp64 in row-major order and divided by factor^2 there (one rounding to fp32); the two fp32 operations that follow are rounded
// separately (the library is built with -ffp-contract=off): at factor 1 the bits of torch's CPU chain.
struct TailGeom {
    int h, w, C;              // source frame
    int y0, x0;               // first row / column of the window
    int oh, ow, factor;
};

__global__ __launch_bounds__(256) void ppl_frames_kernel(const float* __restrict__ frames, float* __restrict__ out, TailGeom g, int64_t pixels) {
    const int64_t plane = (int64_t)g.oh * g.ow;
    const double area = (double)g.factor * (double)g.factor;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = p / plane;
        const int64_t r = p - f * plane;
        const int oy = (int)(r / g.ow), ox = (int)(r - (int64_t)oy * g.ow);
        const float* __restrict__ src = frames + (f * g.h * g.w + (int64_t)(g.y0 + oy * g.factor) * g.w + (g.x0 + ox * g.factor)) * g.C;
        float y[3] = {0.f, 0.f, 0.f};
        for (int c = 0; c < g.C; c++) {
            float x;
            if (g.factor == 1) {
                x = src[c];
            } else {
                double s = 0.0;
                for (int dy = 0; dy < g.factor; dy++)
                    for (int dx = 0; dx < g.factor; dx++) s += (double)src[((int64_t)dy * g.w + dx) * g.C + c];
                x = (float)(s / area);
            }
            y[c] = (x + 1.0f) * 127.5f;
        }
        float* __restrict__ dst = out + f * 3 * plane + r;
        dst[0] = y[0];
        dst[plane] = g.C == 1 ? y[0] : y[1];
        dst[2 * plane] = g.C == 1 ? y[0] : y[2];
    }
}

}  // namespace

TDGP_API int tdgp_ppl_frames(const float* frames, int64_t num_frames, int h, int w, int C, int crop, int factor, float* out, tdgp_stream_t stream) {
    TDGP_CHECK(num_frames >= 0 && h >= 1 && w >= 1, TDGP_EINVAL, "ppl_frames: bad shape (%lld frames of %d x %d)", (long long)num_frames, h, w);
    TDGP_CHECK(C == 1 || C == 3, TDGP_EINVAL, "ppl_frames: C must be 1 or 3");
    TDGP_CHECK(factor >= 1, TDGP_EINVAL, "ppl_frames: factor = %d, must be >= 1", factor);
    TailGeom g;
    g.h = h; g.w = w; g.C = C; g.factor = factor;
    g.y0 = g.x0 = 0;
    int wh = h, ww = w;
    if (crop) {
        TDGP_CHECK(h == w, TDGP_EINVAL, "ppl_frames: the centre crop needs a square frame, got %d x %d", h, w);
        const int c = h / 8;
        TDGP_CHECK(c >= 1, TDGP_EINVAL, "ppl_frames: the centre crop of a %d x %d frame is empty", h, w);
        g.y0 = 3 * c; g.x0 = 2 * c;
        wh = ww = 4 * c;
    }
    TDGP_CHECK(wh % factor == 0 && ww % factor == 0, TDGP_EINVAL, "ppl_frames: the %d x %d window does not divide by factor %d", wh, ww, factor);
    g.oh = wh / factor; g.ow = ww / factor;
    TDGP_CHECK((int64_t)h * w < ((int64_t)1 << 31) && (double)num_frames * h * w * 3 < 9.0e18, TDGP_EINVAL, "ppl_frames: tensor too large");
    if (num_frames == 0) return TDGP_OK;
    TDGP_CHECK(frames && out, TDGP_EINVAL, "ppl_frames: null pointer");
    TDGP_CHECK(((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 3) == 0, TDGP_EINVAL, "ppl_frames: frames and out must be 4-byte aligned");
    const int64_t pixels = num_frames * g.oh * g.ow;
    const dim3 grid((unsigned)std::min<int64_t>(262144, cdiv64(pixels, 256)));
    TDGP_LAUNCH("ppl_frames_kernel", ppl_frames_kernel, grid, dim3(256), 0, (hipStream_t)stream, frames, out, g, pixels);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

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

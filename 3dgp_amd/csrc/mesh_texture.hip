// mesh_texture.hip -- mesh textures: a per-triangle atlas baked from the field and fetched at the hits of a mesh frame (mesh_texture.py,
// DESIGN.md 5.23).  The atlas is a pure function of the triangle count: tile k of (n + 2)^2 texels holds triangle 2k in its lower-left half
// and triangle 2k + 1, rotated by a half turn, in its upper-right half.
//   tdgp_atlas_points (per texel: its owner and the point of the owner's plane it stands for) -> [the field at the points: the caller's]
//   -> tdgp_atlas_texels (per texel: the colour as three bytes)
//   tdgp_mesh_resolve -> tdgp_mesh_sample_texture -> tdgp_mesh_shade (per ray: nearest or bilinear fetch inside the hit triangle's tile)
// The barycentric coordinates of a texel are NOT clamped: the one or two diagonals of a half tile beyond the hypotenuse (the gutter) are
// sampled on the triangle's plane just outside it (b0 < 0), and that extrapolation is what makes a bilinear fetch reproduce a colour that
// is linear in position exactly, hypotenuse included: all four taps of a fetch inside the triangle belong to the triangle's own half.
// Arithmetic contract (include/tdgp.h): double where stated, every operation rounded once in the order written (-ffp-contract=off),
// ordered comparisons, one writer per element, no atomics, no workspace.  A numpy restatement reproduces all three bit for bit
// (tests/mesh_texture_reference.py).
#include "common.h"
#include "mesh_hit.h"

namespace {

constexpr int MT_BLOCK = 256;
constexpr int MT_TEXELS_MIN = 2, MT_TEXELS_MAX = 64, MT_SIDE_MAX = 16384;
constexpr int64_t MT_RAYS_MAX = (int64_t)1 << 30;

__global__ __launch_bounds__(MT_BLOCK) void atlas_points_kernel(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ triangles, int64_t T,
                                                                int n, int r, int W, int64_t texels, float* __restrict__ points, int32_t* __restrict__ owner) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= texels) return;
    const int S = n + 2;
    const int row = (int)(i / W), col = (int)(i - (int64_t)row * W);
    const int tx = col / S, ty = row / S;
    const int px = col - tx * S, py = row - ty * S;
    const bool lower = px + py <= n;
    const int64_t t = 2 * ((int64_t)ty * r + tx) + (lower ? 0 : 1);
    const int qx = lower ? px : S - 1 - px, qy = lower ? py : S - 1 - py;
    bool owned = t < T;
    int idx[3] = {0, 0, 0};
    if (owned) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            idx[c] = triangles[t * 3 + c];
            owned = owned && idx[c] >= 0 && (int64_t)idx[c] < V;
        }
    }
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (owned) {
        const double m = (double)(n - 1);
        const double b1 = (double)qx / m, b2 = (double)qy / m;
        const double b0 = (1.0 - b1) - b2;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v0 = (double)vertices[(int64_t)idx[0] * 3 + c], v1 = (double)vertices[(int64_t)idx[1] * 3 + c];
            const double v2 = (double)vertices[(int64_t)idx[2] * 3 + c];
            p[c] = (float)((b0 * v0 + b1 * v1) + b2 * v2);
        }
    }
    owner[i] = owned ? (int32_t)t : -1;
#pragma unroll
    for (int c = 0; c < 3; c++) points[i * 3 + c] = p[c];
}

struct Fill {
    uint8_t c[3];
};

__global__ __launch_bounds__(MT_BLOCK) void atlas_texels_kernel(const float* __restrict__ rgb, int64_t stride, const int32_t* __restrict__ owner, int64_t texels,
                                                                Fill fill, uint8_t* __restrict__ image) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= texels) return;
    const bool owned = owner[i] >= 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        uint8_t byte = fill.c[c];
        if (owned) {
            float k = rgb[i * stride + c] * 0.5f + 0.5f;
            if (!(k > 0.0f)) k = 0.0f;
            if (k > 1.0f) k = 1.0f;
            byte = (uint8_t)rintf(k * 255.0f);
        }
        image[i * 3 + c] = byte;
    }
}

__global__ __launch_bounds__(MT_BLOCK) void sample_texture_kernel(const int32_t* __restrict__ tri, const int32_t* __restrict__ status, const float* __restrict__ t_hit,
                                                                  const float* __restrict__ ray_o, const float* __restrict__ ray_d, int64_t rays,
                                                                  const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ tris, int64_t T,
                                                                  const uint8_t* __restrict__ image, int n, int r, int W, int filter, float* __restrict__ colour) {
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= rays) return;
    float out[3] = {0.0f, 0.0f, 0.0f};
    const int k = tri[ray];
    bool hit = status[ray] == 1 && k >= 0 && (int64_t)k < T;
    int idx[3] = {0, 0, 0};
    if (hit) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            idx[i] = tris[(int64_t)k * 3 + i];
            hit = hit && idx[i] >= 0 && (int64_t)idx[i] < V;
        }
    }
    if (hit) {
        const float th = t_hit[ray];
        float x[3];
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] = ray_o[ray * 3 + c] + ray_d[ray * 3 + c] * th;
        double a[3], b[3], v0[3], w[3];
        mesh_tri_frame(verts, idx, a, b, v0);
        mesh_bary_weights(a, b, v0, x, w);                              // shared with tdgp_mesh_resolve and tdgp_mesh_interp_normals (mesh_bary.h)
        mesh_texture_fetch(w, k, image, n, r, W, filter, out);          // shared with tdgp_mesh_resolve_ms (mesh_hit.h)
    }
#pragma unroll
    for (int c = 0; c < 3; c++) colour[ray * 3 + c] = out[c];
}

// shared argument checks of the three entry points; `what` names the caller in the message
int atlas_check(const char* what, int64_t T, int n, int r, int W, int H) {
    TDGP_CHECK(T >= 0 && T <= 2147483647ll, TDGP_EINVAL, "%s: T must lie in [0, 2^31 - 1]", what);
    TDGP_CHECK(n >= MT_TEXELS_MIN && n <= MT_TEXELS_MAX, TDGP_EINVAL, "%s: texels must lie in [%d, %d], got %d", what, MT_TEXELS_MIN, MT_TEXELS_MAX, n);
    TDGP_CHECK(r >= 0 && W >= 0 && H >= 0, TDGP_EINVAL, "%s: negative atlas size", what);
    TDGP_CHECK(W <= MT_SIDE_MAX && H <= MT_SIDE_MAX, TDGP_EUNSUPPORTED, "%s: an atlas of %d x %d texels exceeds the %d x %d this build takes (fewer texels per triangle, or a simpler mesh)",
               what, W, H, MT_SIDE_MAX, MT_SIDE_MAX);
    TDGP_CHECK(atlas_is(T, n, r, W, H), TDGP_EINVAL, "%s: (tiles_per_row %d, width %d, height %d) is not the atlas of %lld triangles at %d texels", what, r, W, H,
               (long long)T, n);
    return TDGP_OK;
}

}  // namespace

TDGP_API int tdgp_atlas_points(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int n, int r, int W, int H, float* points,
                               int32_t* owner, tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= 2147483647ll, TDGP_EINVAL, "atlas_points: V must lie in [0, 2^31 - 1]");
    const int rc = atlas_check("atlas_points", T, n, r, W, H);
    if (rc != TDGP_OK) return rc;
    const int64_t texels = (int64_t)H * W;
    if (texels == 0) return TDGP_OK;
    TDGP_CHECK((vertices || V == 0) && triangles && points && owner, TDGP_EINVAL, "atlas_points: null pointer");
    TDGP_LAUNCH("atlas_points_kernel", atlas_points_kernel, dim3((unsigned)cdiv64(texels, MT_BLOCK)), dim3(MT_BLOCK), 0, (hipStream_t)stream, vertices, V, triangles, T,
                n, r, W, texels, points, owner);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_atlas_texels(const float* rgb, int64_t rgb_stride, const int32_t* owner, int64_t texels, const uint8_t* fill, uint8_t* image,
                               tdgp_stream_t stream) {
    TDGP_CHECK(texels >= 0 && texels <= (int64_t)MT_SIDE_MAX * MT_SIDE_MAX, TDGP_EINVAL, "atlas_texels: the texel count must lie in [0, 16384^2]");
    TDGP_CHECK(rgb_stride >= 3 && rgb_stride <= 1024, TDGP_EINVAL, "atlas_texels: rgb_stride must lie in [3, 1024] elements, got %lld", (long long)rgb_stride);
    TDGP_CHECK(fill, TDGP_EINVAL, "atlas_texels: fill must point to 3 bytes on the host");
    if (texels == 0) return TDGP_OK;
    TDGP_CHECK(rgb && owner && image, TDGP_EINVAL, "atlas_texels: null pointer");
    const Fill f{{fill[0], fill[1], fill[2]}};
    TDGP_LAUNCH("atlas_texels_kernel", atlas_texels_kernel, dim3((unsigned)cdiv64(texels, MT_BLOCK)), dim3(MT_BLOCK), 0, (hipStream_t)stream, rgb, rgb_stride, owner,
                texels, f, image);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

TDGP_API int tdgp_mesh_sample_texture(const int32_t* tri, const int32_t* status, const float* t_hit, const float* ray_o, const float* ray_d, int64_t rays,
                                      const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* image, int n, int r, int W,
                                      int H, int filter, float* colour, tdgp_stream_t stream) {
    TDGP_CHECK(V >= 0 && V <= 2147483647ll, TDGP_EINVAL, "mesh_sample_texture: V must lie in [0, 2^31 - 1]");
    TDGP_CHECK(rays >= 0 && rays <= MT_RAYS_MAX, TDGP_EINVAL, "mesh_sample_texture: bad ray count");
    TDGP_CHECK(filter == 0 || filter == 1, TDGP_EINVAL, "mesh_sample_texture: filter must be 0 (nearest) or 1 (bilinear), got %d", filter);
    const int rc = atlas_check("mesh_sample_texture", T, n, r, W, H);
    if (rc != TDGP_OK) return rc;
    if (rays == 0) return TDGP_OK;
    TDGP_CHECK(tri && status && t_hit && ray_o && ray_d && colour, TDGP_EINVAL, "mesh_sample_texture: null pointer");
    TDGP_CHECK(T == 0 || (vertices && triangles && image), TDGP_EINVAL, "mesh_sample_texture: null mesh or image pointer");
    TDGP_LAUNCH("sample_texture_kernel", sample_texture_kernel, dim3((unsigned)cdiv64(rays, MT_BLOCK)), dim3(MT_BLOCK), 0, (hipStream_t)stream, tri, status, t_hit,
                ray_o, ray_d, rays, vertices, V, triangles, T, image, n, r, W, filter, colour);
    TDGP_LAUNCH_CHECK();
    return TDGP_OK;
}

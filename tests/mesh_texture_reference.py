"""The yardstick of the mesh-texture tests: the atlas layout, the corner UVs and the contracts of tdgp_atlas_points / tdgp_atlas_texels /
tdgp_mesh_sample_texture (include/tdgp.h) restated in numpy, operation for operation -- float64 / float32 arrays whose every operation numpy
rounds once, never fusing a multiply into an add.  Visibility, resolve, shading and the meshes come from mesh_raster_reference; the
barycentric weights are restated here array-wise from the same contract (mesh_surface_reference has them ray by ray).  Written from the
contract, for these tests."""
import collections

import numpy as np

import mesh_raster_reference as MR

F = np.float32
D = np.float64
Atlas = collections.namedtuple('Atlas', ['texels', 'tile', 'tiles_per_row', 'width', 'height'])
FILTERS = {'nearest': 0, 'bilinear': 1}


def atlas_layout(T, n):
    S, P = n + 2, (T + 1) // 2
    r = 0
    while r * r < P:
        r += 1
    rows = (P + r - 1) // r if r else 0
    return Atlas(n, S, r, r * S, rows * S)


def texel_owner(T, atlas):
    """Per texel of the image, integers only -> (t int64 [H,W]: the triangle of that half tile, -1 beyond T; qx, qy int64 [H,W])."""
    n, S, r, W, H = atlas
    col, row = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    if W == 0 or H == 0:
        z = np.zeros((H, W), np.int64)
        return z - 1, z, z
    tx, ty = col // S, row // S
    px, py = col - tx * S, row - ty * S
    lower = px + py <= n
    t = 2 * (ty * r + tx) + np.where(lower, 0, 1)
    qx, qy = np.where(lower, px, S - 1 - px), np.where(lower, py, S - 1 - py)
    return np.where(t < T, t, -1), qx, qy


def atlas_uvs(T, atlas):
    n, S, r, W, H = atlas
    out = np.zeros((T, 3, 2), F)
    for t in range(T):
        k = t // 2
        X0, Y0 = (k % r) * S, (k // r) * S
        corners = ((0, 0), (n - 1, 0), (0, n - 1))
        for i, (qx, qy) in enumerate(corners):
            x, y = (X0 + qx, Y0 + qy) if t % 2 == 0 else (X0 + S - 1 - qx, Y0 + S - 1 - qy)
            out[t, i] = (F((D(x) + 0.5) / D(W)), F(1.0 - (D(y) + 0.5) / D(H)))
    return out


def atlas_points(vertices, triangles, atlas):
    """-> (points fp32 [H*W,3], owner int32 [H*W])."""
    v, tri = np.asarray(vertices, F).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(v), len(tri)
    n = atlas.texels
    t, qx, qy = (a.reshape(-1) for a in texel_owner(T, atlas))
    idx = tri[np.where(t >= 0, t, 0)] if T else np.zeros((len(t), 3), np.int64)
    owned = (t >= 0) & np.all((idx >= 0) & (idx < V), axis=1)
    idx = np.where(owned[:, None], idx, 0)
    P = v[idx].astype(D) if V else np.zeros((len(t), 3, 3))
    m = D(n - 1)
    b1, b2 = qx.astype(D) / m, qy.astype(D) / m
    b0 = (D(1) - b1) - b2
    with np.errstate(all='ignore'):
        p = ((b0[:, None] * P[:, 0] + b1[:, None] * P[:, 1]) + b2[:, None] * P[:, 2]).astype(F)
    return np.where(owned[:, None], p, F(0)).astype(F), np.where(owned, t, -1).astype(np.int32)


def atlas_texels(rgb, owner, fill=(0, 0, 0)):
    """rgb fp32 [N, >=3], owner [N] -> uint8 [N,3]."""
    c = np.asarray(rgb, F)[:, :3]
    with np.errstate(all='ignore'):
        k = c * F(0.5) + F(0.5)
        k = np.where(k > 0, k, F(0)).astype(F)
        k = np.where(k > 1, F(1), k).astype(F)
        byte = np.rint(k * F(255)).astype(np.uint8)
    return np.where((np.asarray(owner) >= 0)[:, None], byte, np.asarray(fill, np.uint8)[None, :]).astype(np.uint8)


def bake(vertices, triangles, colour_fn, texels, fill=(0, 0, 0)):
    """-> (image uint8 [H,W,3], uvs, atlas, points, owner); colour_fn: numpy points fp32 [N,3] -> fp32 [N, >=3]."""
    T = len(np.asarray(triangles).reshape(-1, 3))
    atlas = atlas_layout(T, texels)
    points, owner = atlas_points(vertices, triangles, atlas)
    image = atlas_texels(colour_fn(points), owner, fill) if len(owner) else np.zeros((0, 3), np.uint8)
    return image.reshape(atlas.height, atlas.width, 3), atlas_uvs(T, atlas), atlas, points, owner


def bary_weights(v0, a, b, x):
    """tdgp_mesh_resolve's colour weights, array-wise: v0, a, b float64 [N,3], x fp32 [N,3] -> (b0, b1, b2) float64 [N]."""
    dot = lambda u, w: (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]      # noqa: E731
    with np.errstate(all='ignore'):
        e = x.astype(D) - v0
        d11, d12, d22, e1, e2 = dot(a, a), dot(a, b), dot(b, b), dot(e, a), dot(e, b)
        den = d11 * d22 - d12 * d12
        b1, b2 = (d22 * e1 - d12 * e2) / den, (d11 * e2 - d12 * e1) / den
        b1, b2 = np.where(b1 >= 0, b1, 0.0), np.where(b2 >= 0, b2, 0.0)
        sm = b1 + b2
        over = sm > 1
        b1, b2 = np.where(over, b1 / sm, b1), np.where(over, b2 / sm, b2)
        return (1.0 - b1) - b2, b1, b2


def _clamp(x, hi):
    x = np.where(x >= 0, x, 0.0)
    return np.where(x > hi, hi, x)


def sample_texture(tri_hit, status, t_hit, ray_o, ray_d, vertices, triangles, image, atlas, filter='bilinear'):
    """-> colour fp32 [rays,3]."""
    v, tri = np.asarray(vertices, F).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    o, d, th = np.asarray(ray_o, F).reshape(-1, 3), np.asarray(ray_d, F).reshape(-1, 3), np.asarray(t_hit, F).reshape(-1)
    k = np.asarray(tri_hit, np.int64).reshape(-1)
    V, T, rays = len(v), len(tri), len(k)
    n, S, r, W, H = atlas
    image = np.asarray(image, np.uint8).reshape(H, W, 3)
    hit = (np.asarray(status).reshape(-1) == 1) & (k >= 0) & (k < T)
    idx = tri[np.where(hit, k, 0)] if T else np.zeros((rays, 3), np.int64)
    hit &= np.all((idx >= 0) & (idx < V), axis=1)
    out = np.zeros((rays, 3), F)
    if not hit.any():
        return out
    sel = np.flatnonzero(hit)
    k, idx = k[sel], idx[sel]
    with np.errstate(all='ignore'):
        x = o[sel] + d[sel] * th[sel, None]                               # fp32
        P = v[idx].astype(D)
        _, b1, b2 = bary_weights(P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], x)
        m, hi = D(n - 1), D(S - 1)
        u, w = b1 * m, b2 * m
        upper = (k & 1) == 1
        tx, ty = _clamp(np.where(upper, hi - u, u), hi), _clamp(np.where(upper, hi - w, w), hi)
    tile = k >> 1
    X0, Y0 = (tile % r) * S, (tile // r) * S
    if FILTERS.get(filter, filter) == 0:
        x0, y0 = np.rint(tx).astype(np.int64), np.rint(ty).astype(np.int64)
        out[sel] = (image[Y0 + y0, X0 + x0].astype(D) / D(255)).astype(F)
        return out
    fx0, fy0 = np.floor(tx), np.floor(ty)
    fx, fy = (tx - fx0)[:, None], (ty - fy0)[:, None]
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)
    gx, gy = D(1) - fx, D(1) - fy
    w00, w10, w01, w11 = gx * gy, fx * gy, gx * fy, fx * fy
    t00, t10 = image[Y0 + y0, X0 + x0].astype(D), image[Y0 + y0, X0 + x1].astype(D)
    t01, t11 = image[Y0 + y1, X0 + x0].astype(D), image[Y0 + y1, X0 + x1].astype(D)
    out[sel] = (((w00 * t00 + w10 * t10) + (w01 * t01 + w11 * t11)) / D(255)).astype(F)
    return out


def frames(vertices, triangles, c2w, focal, ray_o, ray_d, h, w, near, cull, step, t_miss, image, atlas, filter='bilinear', vertex_normal=None, **shade_kw):
    """resolve -> (interp) -> sample -> shade: the frames of render_mesh_views(mode='colour', texture=...) -> dict as mesh_raster_reference.frames."""
    vis, _ = MR.visibility(vertices, triangles, c2w, focal, ray_d, h, w, near, cull)
    out = MR.resolve(vis, vertices, triangles, ray_o, ray_d, step, t_miss)
    if vertex_normal is not None:
        import mesh_surface_reference as SR
        out['normal'] = SR.interp_normals(out['tri'], out['status'], out['t_hit'], ray_o, ray_d, vertices, triangles, vertex_normal, out['normal'])
    out['colour'] = sample_texture(out['tri'], out['status'], out['t_hit'], ray_o, ray_d, vertices, triangles, image, atlas, filter)
    out['rgb'] = MR.shade(out['normal'], out['status'], ray_d, out['colour'], 'colour', **shade_kw)
    return out

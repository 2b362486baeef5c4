"""The yardstick of the mesh-frame tests: the contracts of tdgp_mesh_visibility / tdgp_mesh_resolve / tdgp_mesh_shade (include/tdgp.h) restated
in numpy, operation for operation -- float64 / float32 arrays whose every operation numpy rounds once (never fusing a multiply into an add,
`/` and `sqrt` correctly rounded), int64 arrays for the coverage -- plus an icosphere and the analytic helpers the tests measure against.
`visibility` also returns how many triangles cover each pixel.  Written from the contract, for these tests."""
import numpy as np

F = np.float32
D = np.float64
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MODES = {'shaded': 0, 'normals': 1, 'colour': 2}
CULL = {'none': 0, 'back': 1, 'front': 2}
LIMIT = 2.0 ** 30


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def visibility(vertices, triangles, c2w, focal, ray_d, h, w, near, cull=0):
    """-> (vis uint64 [C, h*w], count int32 [C, h*w]: the triangles whose candidate reached the minimum of that pixel)."""
    v, tri = _f(vertices).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    c2w, focal = _f(c2w).reshape(-1, 4, 4), _f(focal).reshape(-1)
    C, V, T, R = c2w.shape[0], v.shape[0], tri.shape[0], h * w
    ray_d = _f(ray_d).reshape(C, R, 3)
    cull = CULL.get(cull, cull)
    vis = np.full((C, R), EMPTY, np.uint64)
    count = np.zeros((C, R), np.int32)
    if T == 0:
        return vis, count
    hw, hh, near = D(w - 1) * D(0.5), D(h - 1) * D(0.5), D(F(near))
    in_range = np.all((tri >= 0) & (tri < V), axis=1)
    P = v[np.where(in_range[:, None], tri, 0)].astype(D) if V else np.zeros((T, 3, 3))          # [T, vertex, component]
    for c in range(C):
        m = c2w[c].astype(D)
        f = (-c2w[c, :3, 2]).astype(D)
        fc = D(focal[c])
        with np.errstate(all='ignore'):
            p0, p1, p2 = P[..., 0] - m[0, 3], P[..., 1] - m[1, 3], P[..., 2] - m[2, 3]
            xc = (p0 * m[0, 0] + p1 * m[1, 0]) + p2 * m[2, 0]
            yc = (p0 * m[0, 1] + p1 * m[1, 1]) + p2 * m[2, 1]
            zc = (p0 * f[0] + p1 * f[1]) + p2 * f[2]
            fx = ((((xc * fc) / zc) + D(1)) * hw) * D(256)
            fy = ((D(1) - ((yc * fc) / zc)) * hh) * D(256)
            iz = D(1) / zc
            ok = in_range & np.all(zc >= near, axis=1) & np.all((np.abs(fx) < LIMIT) & (np.abs(fy) < LIMIT), axis=1)
            X = np.where(ok[:, None], np.rint(fx), 0).astype(np.int64)
            Y = np.where(ok[:, None], np.rint(fy), 0).astype(np.int64)
        area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        ok &= area2 != 0
        if cull == 1:
            ok &= ~(area2 > 0)
        elif cull == 2:
            ok &= ~(area2 < 0)
        c0 = np.maximum(0, (X.min(axis=1) + 255) >> 8)
        c1 = np.minimum(w - 1, X.max(axis=1) >> 8)
        r0 = np.maximum(0, (Y.min(axis=1) + 255) >> 8)
        r1 = np.minimum(h - 1, Y.max(axis=1) >> 8)
        ok &= (c0 <= c1) & (r0 <= r1)
        for k in np.nonzero(ok)[0]:
            s = -1 if area2[k] < 0 else 1
            px = (np.arange(c0[k], c1[k] + 1, dtype=np.int64) << 8)[None, :]
            py = (np.arange(r0[k], r1[k] + 1, dtype=np.int64) << 8)[:, None]
            Xk, Yk = [int(a) for a in X[k]], [int(a) for a in Y[k]]
            e, inside = [], True
            for i in range(3):
                a, b = (i + 1) % 3, (i + 2) % 3
                dx, dy = s * (Xk[b] - Xk[a]), s * (Yk[b] - Yk[a])
                ei = dx * (py - Yk[a]) - dy * (px - Xk[a])
                top_left = dy < 0 or (dy == 0 and dx > 0)
                inside = inside & ((ei > 0) | ((ei == 0) & top_left))
                e.append(ei)
            if not inside.any():
                continue
            ray = (py >> 8) * w + (px >> 8)
            d = ray_d[c][ray].astype(D)
            with np.errstate(all='ignore'):
                q = (e[0].astype(D) * iz[k, 0] + e[1].astype(D) * iz[k, 1]) + e[2].astype(D) * iz[k, 2]
                depth = D(abs(int(area2[k]))) / q
                df = (d[..., 0] * f[0] + d[..., 1] * f[1]) + d[..., 2] * f[2]
                t = (depth / df).astype(F)
                valid = inside & (t > 0) & (t < np.inf)
            key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(k)
            r = ray[valid]
            vis[c, r] = np.minimum(vis[c, r], key[valid])
            count[c, r] += 1
    return vis, count


def resolve(vis, vertices, triangles, ray_o, ray_d, step, t_miss, vertex_rgb=None):
    """-> dict(t_hit [rays], status int32, tri int32, normal [rays,3], colour [rays,3] or None, points [rays,7,3])."""
    vis = np.asarray(vis).reshape(-1).view(np.uint64)
    v, tri = _f(vertices).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    o, d = _f(ray_o).reshape(-1, 3), _f(ray_d).reshape(-1, 3)
    V, T, rays = v.shape[0], tri.shape[0], vis.shape[0]
    step = F(step)
    k = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    k = np.where(k >= 2 ** 31, k - 2 ** 32, k)                       # the low word read as int32
    hit = (vis != EMPTY) & (k >= 0) & (k < T)
    idx = tri[np.where(hit, k, 0)] if T else np.zeros((rays, 3), np.int64)
    hit &= np.all((idx >= 0) & (idx < V), axis=1)
    idx = np.where(hit[:, None], idx, 0)
    th = np.where(hit, (vis >> np.uint64(32)).astype(np.uint32).view(F), F(t_miss)).astype(F)
    with np.errstate(all='ignore'):
        x = o + d * th[:, None]
        P = v[idx].astype(D) if V else np.zeros((rays, 3, 3))
        v0, a, b = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        g = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        q = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        toward = (-d) / dn[:, None]
        ok = (q > 0) & (q < np.inf)
        n = np.where(ok[:, None], (g / np.sqrt(q)[:, None]).astype(F), toward).astype(F)
        n = np.where(hit[:, None], n, F(0)).astype(F)
        colour = None
        if vertex_rgb is not None:
            rgb = _f(vertex_rgb).reshape(-1, 3)[idx].astype(D) if V else np.zeros((rays, 3, 3))
            dot = lambda u, w_: (u[:, 0] * w_[:, 0] + u[:, 1] * w_[:, 1]) + u[:, 2] * w_[:, 2]      # noqa: E731
            e = x.astype(D) - v0
            d11, d12, d22, e1, e2 = dot(a, a), dot(a, b), dot(b, b), dot(e, a), dot(e, b)
            den = d11 * d22 - d12 * d12
            b1, b2 = (d22 * e1 - d12 * e2) / den, (d11 * e2 - d12 * e1) / den
            b1, b2 = np.where(b1 >= 0, b1, 0.0), np.where(b2 >= 0, b2, 0.0)
            sm = b1 + b2
            over = sm > 1
            b1, b2 = np.where(over, b1 / sm, b1), np.where(over, b2 / sm, b2)
            b0 = (1.0 - b1) - b2
            colour = ((b0[:, None] * rgb[:, 0] + b1[:, None] * rgb[:, 1]) + b2[:, None] * rgb[:, 2]).astype(F)
            colour = np.where(hit[:, None], colour, F(0)).astype(F)
        points = np.repeat(x[:, None, :], 7, axis=1)
        for i in range(3):
            points[:, 1 + 2 * i, i] = x[:, i] + step
            points[:, 2 + 2 * i, i] = x[:, i] - step
    return dict(t_hit=th, status=hit.astype(np.int32), tri=np.where(hit, k, -1).astype(np.int32), normal=n, colour=colour, points=points)


def shade(normal, status, ray_d, colour=None, mode='shaded', light=None, ambient=0.2, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0)):
    """-> rgb [rays,3]."""
    n, d = _f(normal).reshape(-1, 3), _f(ray_d).reshape(-1, 3)
    status = np.asarray(status).reshape(-1)
    ambient, albedo, background = F(ambient), _f(albedo), _f(background)
    with np.errstate(all='ignore'):
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        l = (-d) / dn[:, None] if light is None else np.broadcast_to(_f(light), d.shape)
        c = (n[:, 0] * l[:, 0] + n[:, 1] * l[:, 1]) + n[:, 2] * l[:, 2]
        c = np.where(c > 0, c, F(0)).astype(F)
        v = ambient + (F(1) - ambient) * c
        if MODES[mode] == 0:
            out = (albedo[None, :] * v[:, None]) * F(2) - F(1)
        elif MODES[mode] == 1:
            out = n
        else:
            k = _f(colour).reshape(-1, 3)
            k = np.where(k > 0, k, F(0)).astype(F)
            k = np.where(k > 1, F(1), k).astype(F)
            out = (k * v[:, None]) * F(2) - F(1)
    return np.where((status == 0)[:, None], background[None, :], out).astype(F)


def frames(vertices, triangles, c2w, focal, ray_o, ray_d, h, w, near, cull, step, t_miss, vertex_rgb=None, mode='shaded', **shade_kw):
    """The three contracts in a row -> dict(vis, count, t_hit, status, tri, normal, colour, points, rgb), flat over [C * h*w] rays."""
    vis, count = visibility(vertices, triangles, c2w, focal, ray_d, h, w, near, cull)
    out = resolve(vis, vertices, triangles, ray_o, ray_d, step, t_miss, vertex_rgb)
    out.update(vis=vis.reshape(-1), count=count.reshape(-1))
    out['rgb'] = shade(out['normal'], out['status'], ray_d, out['colour'], mode, **shade_kw)
    return out


# ---- meshes and analytic helpers ---------------------------------------------------------------------------------------

def icosphere(subdivisions, radius=1.0):
    """A closed sphere mesh of 20 * 4^subdivisions triangles wound counter-clockwise seen from outside -> (vertices fp32 [V,3], triangles int32 [T,3])."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [tuple(np.array(p, D) / np.linalg.norm(p)) for p in verts]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        cache, out = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                p = (np.array(verts[i]) + np.array(verts[j])) / 2.0
                verts.append(tuple(p / np.linalg.norm(p)))
                cache[key] = len(verts) - 1
            return cache[key]

        for a, b, c in tris:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = out
    return _f(np.array(verts, D) * radius), np.array(tris, np.int32)


def sagitta(vertices, triangles, radius):
    """How far the flat facets of a mesh inscribed in the sphere |x| = radius lie inside it, at most: radius - the least distance of a facet's plane."""
    P = np.asarray(vertices, D)[np.asarray(triangles)]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return float(radius - np.abs((n * P[:, 0]).sum(1)).min())


def pinhole_camera(fov_deg, radius=1.0):
    """(c2w [1,4,4], focal [1]) of shapes_reference.pinhole_rays' camera: at (0, 0, radius), looking down -z at the origin."""
    c2w = np.eye(4, dtype=F)[None].copy()
    c2w[0, 2, 3] = radius
    return c2w, _f([1.0 / np.tan(np.deg2rad(fov_deg) / 2.0)])


def impact_parameter(ray_o, ray_d):
    """Float64 distance of each ray's line from the origin."""
    o, d = np.asarray(ray_o, D), np.asarray(ray_d, D)
    return np.linalg.norm(np.cross(o, d), axis=-1) / np.linalg.norm(d, axis=-1)


def sphere_cosine(ray_o, ray_d, t, radius):
    """Float64 cosine between -d and the sphere's outward normal at o + t d."""
    o, d = np.asarray(ray_o, D), np.asarray(ray_d, D)
    x = o + d * np.asarray(t, D)[:, None]
    return -(x * d).sum(-1) / (np.linalg.norm(x, axis=-1) * np.linalg.norm(d, axis=-1))

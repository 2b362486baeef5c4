"""The yardstick of the multisampled mesh-frame tests: the contracts of tdgp_mesh_visibility_ms / tdgp_mesh_resolve_ms (include/tdgp.h) restated
in numpy, operation for operation -- int64 arrays for the coverage, float64 / float32 arrays whose every operation numpy rounds once.  A
sample is resolved and shaded as a ray is, so the per-hit arithmetic is not restated again: every sample goes, as a ray of its own, through
the restatements of the one-sample kernels (mesh_raster_reference.resolve / shade, mesh_texture_reference.sample_texture and the weights of
mesh_texture_reference.bary_weights for the vertex normals).  Plus the exact area of a triangle inside a pixel, by clipping in float64.
Written from the contract, for these tests."""
import numpy as np

import mesh_raster_reference as MR
import mesh_texture_reference as TR

F = np.float32
D = np.float64
EMPTY = MR.EMPTY
PAD = 96
PATTERNS = {4: ((-32, -96), (96, -32), (-96, 32), (32, 96)),
            16: tuple((ox, oy) for oy in (-96, -32, 32, 96) for ox in (-96, -32, 32, 96))}


def offsets(S):
    """-> (ox, oy) int64 [S] in 1/256 pixel; S = 1 is the pixel centre alone (the one-sample route, for the coverage-error comparison)."""
    p = np.asarray(PATTERNS[S] if S != 1 else ((0, 0),), np.int64)
    return p[:, 0], p[:, 1]


def cover(X, Y, c0, c1, r0, r1, S):
    """One triangle with snapped vertices X, Y (three ints each, area != 0) on the pixels [r0, r1] x [c0, c1] ->
    (inside bool [rows, cols, S], e: the three edge functions int64 [rows, cols, S], sx, sy int64 [rows, cols, S])."""
    X, Y = [int(a) for a in X], [int(a) for a in Y]
    area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    s = -1 if area2 < 0 else 1
    ox, oy = offsets(S)
    sx = (np.arange(c0, c1 + 1, dtype=np.int64) << 8)[None, :, None] + ox[None, None, :] + np.zeros((r1 - r0 + 1, 1, 1), np.int64)
    sy = (np.arange(r0, r1 + 1, dtype=np.int64) << 8)[:, None, None] + oy[None, None, :] + np.zeros((1, c1 - c0 + 1, 1), np.int64)
    e, inside = [], np.ones(sx.shape, bool)
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = s * (X[b] - X[a]), s * (Y[b] - Y[a])
        ei = dx * (sy - Y[a]) - dy * (sx - X[a])
        top_left = dy < 0 or (dy == 0 and dx > 0)
        inside &= (ei > 0) | ((ei == 0) & top_left)
        e.append(ei)
    return inside, e, sx, sy


def box(X, Y, h, w, pad):
    c0, c1 = max(0, (int(min(X)) - pad + 255) >> 8), min(w - 1, (int(max(X)) + pad) >> 8)
    r0, r1 = max(0, (int(min(Y)) - pad + 255) >> 8), min(h - 1, (int(max(Y)) + pad) >> 8)
    return c0, c1, r0, r1


def hit_counts(X, Y, h, w, S):
    """The samples of every pixel of an h x w frame that the snapped triangle covers -> int64 [h, w] (S = 1: the pixel centre)."""
    out = np.zeros((h, w), np.int64)
    X, Y = [int(a) for a in X], [int(a) for a in Y]
    if (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]) == 0:
        return out
    c0, c1, r0, r1 = box(X, Y, h, w, PAD if S != 1 else 0)
    if c0 <= c1 and r0 <= r1:
        out[r0:r1 + 1, c0:c1 + 1] = cover(X, Y, c0, c1, r0, r1, S)[0].sum(axis=2)
    return out


def sample_ray(sx, sy, h, w, fc):
    """(u, v, len) float64 of the screen positions sx, sy (int64 arrays)."""
    hw, hh = D(w - 1) * D(0.5), D(h - 1) * D(0.5)
    u = (sx.astype(D) / (D(256) * hw) - D(1)) / fc
    v = (D(1) - sy.astype(D) / (D(256) * hh)) / fc
    return u, v, np.sqrt((u * u + v * v) + D(1))


def sample_rays(c2w, focal, h, w, S):
    """-> (ray_o, ray_d) fp32 [C, h*w, S, 3]: the ray of every sample."""
    c2w, focal = np.asarray(c2w, F).reshape(-1, 4, 4), np.asarray(focal, F).reshape(-1)
    C = c2w.shape[0]
    ox, oy = offsets(S)
    row, col = np.divmod(np.arange(h * w, dtype=np.int64), w)
    sx, sy = (col << 8)[:, None] + ox[None, :], (row << 8)[:, None] + oy[None, :]
    o, d = np.zeros((C, h * w, S, 3), F), np.zeros((C, h * w, S, 3), F)
    for c in range(C):
        m = c2w[c].astype(D)
        u, v, ln = sample_ray(sx, sy, h, w, D(focal[c]))
        for j in range(3):
            d[c, :, :, j] = (((u * m[j, 0] + v * m[j, 1]) + D(-c2w[c, j, 2])) / ln).astype(F)
            o[c, :, :, j] = c2w[c, j, 3]
    return o, d


def visibility_ms(vertices, triangles, c2w, focal, h, w, S, near, cull=0):
    """-> vis uint64 [C, h*w, S]."""
    v, tri = MR._f(vertices).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    c2w, focal = MR._f(c2w).reshape(-1, 4, 4), MR._f(focal).reshape(-1)
    C, V, T = c2w.shape[0], v.shape[0], tri.shape[0]
    cull = MR.CULL.get(cull, cull)
    vis = np.full((C, h * w, S), EMPTY, np.uint64)
    if T == 0:
        return vis
    hw, hh, near = D(w - 1) * D(0.5), D(h - 1) * D(0.5), D(F(near))
    in_range = np.all((tri >= 0) & (tri < V), axis=1)
    P = v[np.where(in_range[:, None], tri, 0)].astype(D) if V else np.zeros((T, 3, 3))
    for c in range(C):
        m = c2w[c].astype(D)
        f = (-c2w[c, :3, 2]).astype(D)
        fc = D(focal[c])
        with np.errstate(all='ignore'):                                # the vertices: tdgp_mesh_visibility's, once per triangle
            p0, p1, p2 = P[..., 0] - m[0, 3], P[..., 1] - m[1, 3], P[..., 2] - m[2, 3]
            xc = (p0 * m[0, 0] + p1 * m[1, 0]) + p2 * m[2, 0]
            yc = (p0 * m[0, 1] + p1 * m[1, 1]) + p2 * m[2, 1]
            zc = (p0 * f[0] + p1 * f[1]) + p2 * f[2]
            fx = ((((xc * fc) / zc) + D(1)) * hw) * D(256)
            fy = ((D(1) - ((yc * fc) / zc)) * hh) * D(256)
            iz = D(1) / zc
            ok = in_range & np.all(zc >= near, axis=1) & np.all((np.abs(fx) < MR.LIMIT) & (np.abs(fy) < MR.LIMIT), axis=1)
            X = np.where(ok[:, None], np.rint(fx), 0).astype(np.int64)
            Y = np.where(ok[:, None], np.rint(fy), 0).astype(np.int64)
        area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        ok &= area2 != 0
        if cull == 1:
            ok &= ~(area2 > 0)
        elif cull == 2:
            ok &= ~(area2 < 0)
        for k in np.nonzero(ok)[0]:
            c0, c1, r0, r1 = box(X[k], Y[k], h, w, PAD)
            if c0 > c1 or r0 > r1:
                continue
            inside, e, sx, sy = cover(X[k], Y[k], c0, c1, r0, r1, S)
            if not inside.any():
                continue
            with np.errstate(all='ignore'):
                q = (e[0].astype(D) * iz[k, 0] + e[1].astype(D) * iz[k, 1]) + e[2].astype(D) * iz[k, 2]
                depth = D(abs(int(area2[k]))) / q
                t = (depth * sample_ray(sx, sy, h, w, fc)[2]).astype(F)
                valid = inside & (t > 0) & (t < np.inf)
            key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(k)
            pixel = ((sy + PAD) >> 8) * w + ((sx + PAD) >> 8)              # the offsets lie in [-96, 96]: the pixel of a sample
            j = np.broadcast_to(np.arange(S), sx.shape)
            vis[c, pixel[valid], j[valid]] = np.minimum(vis[c, pixel[valid], j[valid]], key[valid])
    return vis


def interp_normals(tri_hit, status, x, vertices, triangles, vertex_normal, normal):
    """tdgp_mesh_interp_normals at the hit points x (fp32 [rays,3]), array-wise -> the new normal (a copy)."""
    v, tri = np.asarray(vertices, F).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    vn = np.asarray(vertex_normal, F).reshape(-1, 3).astype(D)
    out = np.array(normal, F).reshape(-1, 3).copy()
    sel = np.flatnonzero(np.asarray(status).reshape(-1) == 1)            # a hit of `resolve`: its triangle and indices are in range
    if len(sel) == 0:
        return out
    idx = tri[np.asarray(tri_hit).reshape(-1)[sel]]
    P = v[idx].astype(D)
    with np.errstate(all='ignore'):
        b0, b1, b2 = TR.bary_weights(P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], x[sel])
        m = (b0[:, None] * vn[idx[:, 0]] + b1[:, None] * vn[idx[:, 1]]) + b2[:, None] * vn[idx[:, 2]]
        q = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        ok = (q > 0) & (q < np.inf)
        n = (m / np.sqrt(q)[:, None]).astype(F)
    out[sel[ok]] = n[ok]
    return out


def resolve_ms(vis, vertices, triangles, c2w, focal, h, w, t_miss, vertex_normal=None, vertex_rgb=None, image=None, atlas=None, filter='bilinear',
               mode='shaded', **shade_kw):
    """-> dict(rgb [P,3], coverage [P], status int32 [P], depth [P], tri int32 [P], normal [P,3]) with P = C*h*w, and the per-sample arrays
    (sample_rgb [P,S,3], sample_status [P,S]) they were formed from."""
    vis = np.asarray(vis).view(np.uint64)
    C, R, S = vis.shape
    Pn = C * R
    o, d = (a.reshape(-1, 3) for a in sample_rays(c2w, focal, h, w, S))
    s = MR.resolve(vis.reshape(-1), vertices, triangles, o, d, 0.0, t_miss, vertex_rgb)
    normal, colour = s['normal'], s['colour']
    with np.errstate(all='ignore'):
        x = o + d * s['t_hit'][:, None]
    if vertex_normal is not None:
        normal = interp_normals(s['tri'], s['status'], x, vertices, triangles, vertex_normal, normal)
    if image is not None:
        colour = TR.sample_texture(s['tri'], s['status'], s['t_hit'], o, d, vertices, triangles, image, atlas, filter)
    rgb_s = MR.shade(normal, s['status'], d, colour, mode, **shade_kw).reshape(Pn, S, 3)
    hit, th = (s['status'] == 1).reshape(Pn, S), s['t_hit'].reshape(Pn, S)
    acc = np.zeros((Pn, 3), D)
    for j in range(S):
        acc = acc + rgb_s[:, j].astype(D)
    rgb = (acc / D(S)).astype(F)
    hits = hit.sum(axis=1)
    best, best_t = np.full(Pn, -1, np.int64), np.zeros(Pn, F)
    for j in range(S):
        take = hit[:, j] & ((best < 0) | (th[:, j] < best_t))
        best, best_t = np.where(take, j, best), np.where(take, th[:, j], best_t).astype(F)
    any_hit = best >= 0
    b = np.maximum(best, 0)
    rows = np.arange(Pn)
    return dict(rgb=rgb, coverage=(hits.astype(F) / F(S)).astype(F), status=any_hit.astype(np.int32),
                depth=np.where(any_hit, best_t, F(t_miss)).astype(F), tri=np.where(any_hit, s['tri'].reshape(Pn, S)[rows, b], -1).astype(np.int32),
                normal=np.where(any_hit[:, None], normal.reshape(Pn, S, 3)[rows, b], F(0)).astype(F), sample_rgb=rgb_s, sample_status=hit)


def frames_ms(vertices, triangles, c2w, focal, h, w, S, near, cull, t_miss, **resolve_kw):
    """The two contracts in a row -> the dict of `resolve_ms` plus vis [C, h*w, S]."""
    vis = visibility_ms(vertices, triangles, c2w, focal, h, w, S, near, cull)
    out = resolve_ms(vis, vertices, triangles, c2w, focal, h, w, t_miss, **resolve_kw)
    out['vis'] = vis
    return out


# ---- exact areas -------------------------------------------------------------------------------------------------------------------------

def _clip(poly, axis, bound, keep_less):
    """Sutherland-Hodgman against one axis-aligned half plane, float64."""
    out = []
    for i in range(len(poly)):
        p, q = poly[i], poly[(i + 1) % len(poly)]
        pin = p[axis] <= bound if keep_less else p[axis] >= bound
        qin = q[axis] <= bound if keep_less else q[axis] >= bound
        if pin:
            out.append(p)
        if pin != qin:
            t = (bound - p[axis]) / (q[axis] - p[axis])
            out.append(p + t * (q - p))
    return out


def exact_coverage(X, Y, h, w):
    """The area of the triangle (vertices in 1/256 pixel) inside the unit square centred on every pixel, in pixels -> float64 [h, w]."""
    tri = [np.array([D(X[i]) / 256.0, D(Y[i]) / 256.0]) for i in range(3)]
    out = np.zeros((h, w), D)
    for r in range(h):
        for c in range(w):
            poly = tri
            for axis, bound, less in ((0, c - 0.5, False), (0, c + 0.5, True), (1, r - 0.5, False), (1, r + 0.5, True)):
                poly = _clip(poly, axis, bound, less) if poly else poly
            if len(poly) >= 3:
                p = np.array(poly)
                out[r, c] = 0.5 * abs(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]))
    return out


def coverage_error(X, Y, h, w, S):
    """The mean absolute error of hits / S against the exact area, over the pixels the triangle touches (exact area > 0)."""
    exact = exact_coverage(X, Y, h, w)
    got = hit_counts(X, Y, h, w, S).astype(D) / D(S)
    touched = exact > 0
    return float(np.abs(got - exact)[touched].mean())

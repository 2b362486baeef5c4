"""The yardstick of the mesh-surface tests: the contracts of tdgp_mesh_corner_table / _vertex_normals / _boundary_vertices / _smooth_step /
_interp_normals (include/tdgp.h) restated in numpy with plain loops in table order -- float64 scalars whose every operation numpy rounds
once (never fusing a multiply into an add, `/` and `sqrt` correctly rounded) -- plus `smooth`, the Taubin driver, and the meshes the tests
share.  Written from the contract, for these tests."""
import numpy as np

import mesh_raster_reference as MR

F = np.float32
D = np.float64
INF = D(np.inf)


def _tris(triangles):
    return np.asarray(triangles, np.int64).reshape(-1, 3)


def _ok(tri, V):
    return bool(np.all((tri >= 0) & (tri < V)))


def corner_table(triangles, V):
    """-> (start int32 [V+1], corner int32 [start[V]], degree int32 [V]): per vertex, its corners 3t + i in ascending corner id."""
    tri = _tris(triangles)
    lists = [[] for _ in range(V)]
    for t in range(len(tri)):
        if _ok(tri[t], V):
            for i in range(3):
                lists[tri[t, i]].append(3 * t + i)                     # visited in ascending corner id
    degree = np.array([len(l) for l in lists], np.int32).reshape(V)
    start = np.zeros(V + 1, np.int32)
    start[1:] = np.cumsum(degree)
    corner = np.array([c for l in lists for c in l], np.int32).reshape(-1)
    return start, corner, degree


def _range(start, v, V, T):
    n = min(max(int(start[V]), 0), 3 * T)
    s = min(max(int(start[v]), 0), n)
    e = min(max(int(start[v + 1]), s), n)
    return s, e


def _corner(tri, V, c):
    """corner id -> (the triangle's three indices, slot) or None for an id outside [0, 3T) or a skipped triangle."""
    c = int(c)
    if c < 0 or c >= 3 * len(tri):
        return None
    t = c // 3
    return (tri[t], c - 3 * t) if _ok(tri[t], V) else None


def _cross(v, idx):
    v0, v1, v2 = (v[idx[i]].astype(D) for i in range(3))
    a, b = v1 - v0, v2 - v0
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], D)


def _unit(s):
    """(s / sqrt((s0*s0 + s1*s1) + s2*s2)) as fp32, or None when the squared length is not in (0, inf)."""
    with np.errstate(all='ignore'):
        q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        if not (q > 0 and q < INF):
            return None
        return (s / np.sqrt(q)).astype(F)


def vertex_normals(vertices, triangles, start, corner, weight=0):
    v, tri = np.asarray(vertices, F).reshape(-1, 3), _tris(triangles)
    V = len(v)
    out = np.zeros((V, 3), F)
    for x in range(V):
        s = np.zeros(3, D)
        for j in range(*_range(start, x, V, len(tri))):
            ct = _corner(tri, V, corner[j])
            if ct is None:
                continue
            with np.errstate(all='ignore'):
                g = _cross(v, ct[0])
                if weight == 0:
                    s = s + g
                else:
                    q = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
                    if q > 0 and q < INF:
                        s = s + g / np.sqrt(q)
        n = _unit(s)
        if n is not None:
            out[x] = n
    return out


def boundary_vertices(triangles, V, start, corner):
    tri = _tris(triangles)
    rim = np.zeros(V, np.uint8)
    for x in range(V):
        s, e = _range(start, x, V, len(tri))
        # one walk over x's corners counts, for every neighbour w at once, the triangles that name w next to x: what the kernel counts per
        # candidate (a corner is passed over when its triangle was the last one counted for that w)
        count, last = {}, {}
        for j in range(s, e):
            ct = _corner(tri, V, corner[j])
            if ct is None:
                continue
            idx, slot = ct
            t = int(corner[j]) // 3
            for w in {int(idx[(slot + 1) % 3]), int(idx[(slot + 2) % 3])} - {x}:
                if last.get(w) != t:
                    count[w], last[w] = count.get(w, 0) + 1, t
        rim[x] = 1 if any(c == 1 for c in count.values()) else 0
    return rim


def smooth_step(vertices, triangles, start, corner, factor, pinned=None):
    v, tri = np.asarray(vertices, F).reshape(-1, 3), _tris(triangles)
    V = len(v)
    out = v.copy()
    factor = D(factor)
    for x in range(V):
        s0, e0 = _range(start, x, V, len(tri))
        d = e0 - s0
        if d == 0 or (pinned is not None and pinned[x]):
            continue
        s = np.zeros(3, D)
        for j in range(s0, e0):
            ct = _corner(tri, V, corner[j])
            if ct is None:
                continue
            idx, slot = ct
            with np.errstate(all='ignore'):
                s = s + v[idx[(slot + 1) % 3]].astype(D)
                s = s + v[idx[(slot + 2) % 3]].astype(D)
        with np.errstate(all='ignore'):
            m = s / D(2 * d)
            xd = v[x].astype(D)
            out[x] = (xd + factor * (m - xd)).astype(F)
    return out


def smooth(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, pinned=None, table=None):
    v = np.asarray(vertices, F).reshape(-1, 3).copy()
    V = len(v)
    if iterations == 0 or V == 0:
        return v
    start, corner, _ = corner_table(triangles, V) if table is None else table
    pin = None if pinned is None else np.asarray(pinned).astype(np.uint8)
    if fix_boundary:
        rim = boundary_vertices(triangles, V, start, corner)
        pin = rim if pin is None else pin | rim
    for _ in range(iterations):
        for f in ([lam] if mu is None else [lam, mu]):
            v = smooth_step(v, triangles, start, corner, f, pin)
    return v


def interp_normals(tri_hit, status, t_hit, ray_o, ray_d, vertices, triangles, vertex_normal, normal):
    """-> the new normal [rays,3] (a copy): tdgp_mesh_resolve's colour weights applied to the vertex normals, normalised."""
    v, tri = np.asarray(vertices, F).reshape(-1, 3), _tris(triangles)
    vn = np.asarray(vertex_normal, F).reshape(-1, 3).astype(D)
    o, d, th = np.asarray(ray_o, F).reshape(-1, 3), np.asarray(ray_d, F).reshape(-1, 3), np.asarray(t_hit, F).reshape(-1)
    out = np.array(normal, F).reshape(-1, 3).copy()
    V = len(v)
    dot = lambda u, w: (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]      # noqa: E731
    for r in np.flatnonzero(np.asarray(status).reshape(-1) == 1):
        k = int(tri_hit[r])
        if k < 0 or k >= len(tri) or not _ok(tri[k], V):
            continue
        idx = tri[k]
        with np.errstate(all='ignore'):
            x = o[r] + d[r] * th[r]                                    # fp32
            v0 = v[idx[0]].astype(D)
            a, b = v[idx[1]].astype(D) - v0, v[idx[2]].astype(D) - v0
            e = x.astype(D) - v0
            d11, d12, d22, e1, e2 = dot(a, a), dot(a, b), dot(b, b), dot(e, a), dot(e, b)
            den = d11 * d22 - d12 * d12
            b1, b2 = (d22 * e1 - d12 * e2) / den, (d11 * e2 - d12 * e1) / den
            b1 = b1 if b1 >= 0 else D(0)
            b2 = b2 if b2 >= 0 else D(0)
            sm = b1 + b2
            if sm > 1:
                b1, b2 = b1 / sm, b2 / sm
            b0 = (D(1) - b1) - b2
            m = (b0 * vn[idx[0]] + b1 * vn[idx[1]]) + b2 * vn[idx[2]]
        n = _unit(m)
        if n is not None:
            out[r] = n
    return out


def frames(vertices, triangles, c2w, focal, ray_o, ray_d, h, w, near, cull, step, t_miss, vertex_normal, vertex_rgb=None, mode='shaded', **shade_kw):
    """resolve -> interp -> shade: the frames of render_mesh_views(normals='vertex') -> dict as mesh_raster_reference.frames."""
    vis, _ = MR.visibility(vertices, triangles, c2w, focal, ray_d, h, w, near, cull)
    out = MR.resolve(vis, vertices, triangles, ray_o, ray_d, step, t_miss, vertex_rgb)
    out['face_normal'] = out['normal']
    out['normal'] = interp_normals(out['tri'], out['status'], out['t_hit'], ray_o, ray_d, vertices, triangles, vertex_normal, out['normal'])
    out['rgb'] = MR.shade(out['normal'], out['status'], ray_d, out['colour'], mode, **shade_kw)
    return out


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
TETRA_V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F)
TETRA_T = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)             # outward winding


def lattice(n=6):
    """An n x n integer lattice in the plane z = 0, every cell split into two triangles by alternating diagonals (so that every interior
    vertex's umbrella is symmetric about it) -> (vertices fp32 [n*n,3], triangles int32 [2*(n-1)^2,3], border bool [n*n])."""
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing='ij'), -1).reshape(-1, 2)
    v = np.concatenate([ij, np.zeros((n * n, 1))], 1).astype(F)
    tris = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    border = (ij == 0).any(1) | (ij == n - 1).any(1)
    return v, np.array(tris, np.int32), border


def fan(n=4096):
    """n triangles round vertex 0 on a closed ring of n vertices (a cone: the apex above the ring's plane) -> (vertices, triangles)."""
    ang = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.5]], ring]).astype(F)
    k = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], 1).astype(np.int32)

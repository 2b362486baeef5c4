"""The mesh-ray contract of include/tdgp.h in IEEE doubles, every operation rounded once in the order written (numpy float64: one ufunc per
operation, nothing fused): the yardstick the kernels of csrc/mesh_rays.hip are compared with bit for bit.  The ray-triangle function on
[rays, triangles] arrays, the scan over all valid triangles, the walk through the grid of tests/mesh_distance_reference.py ray by ray, the
direction tables and ambient occlusion; and the rays the tests cast."""
import collections
import math

import numpy as np

import mesh_distance_reference as MD

F = np.float32
D = np.float64
Hits = collections.namedtuple('Hits', ['t', 'depth', 'triangle', 'bary', 'side'])
Ray = collections.namedtuple('Ray', ['kx', 'ky', 'kz', 'Sx', 'Sy', 'Sz', 'ox', 'oy', 'oz'])
SLACK = 2.0 ** -48
NONE = 2 ** 31 - 1
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def setup(o, d):
    """Rays (o, d float64 [R,3], finite, d != 0) -> Ray of [R] arrays."""
    o, d = np.asarray(o, D).reshape(-1, 3), np.asarray(d, D).reshape(-1, 3)
    rows = np.arange(len(d))
    kz = np.argmax(np.abs(d), axis=1)                                                              # the first of equals
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    dz = d[rows, kz]
    kx, ky = np.where(dz < 0, ky, kx), np.where(dz < 0, kx, ky)
    return Ray(kx, ky, kz, d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz, o[rows, kx], o[rows, ky], o[rows, kz])


def ray_triangle(ray, a, b, c, t_min, t_max):
    """Ray of [R] arrays against corners float64 [T,3] -> (accepted bool, t, U, V, W, det), each [R,T]."""
    def frame(p):
        pz = p[:, ray.kz].T - ray.oz[:, None]
        px = p[:, ray.kx].T - ray.ox[:, None]
        py = p[:, ray.ky].T - ray.oy[:, None]
        return px - ray.Sx[:, None] * pz, py - ray.Sy[:, None] * pz, ray.Sz[:, None] * pz

    with np.errstate(all='ignore'):
        ax, ay, az = frame(a)
        bx, by, bz = frame(b)
        cx, cy, cz = frame(c)
        U = cx * by - cy * bx
        V = ax * cy - ay * cx
        W = bx * ay - by * ax
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        t = ((U * az + V * bz) + W * cz) / det
        ok = ~mixed & (det != 0.0) & (t >= t_min) & (t <= t_max)
    return ok, t, U, V, W, det


def _corners(grid, ids):
    return MD._corners(grid.vertices, grid.triangles, np.asarray(ids, np.int64))


def good_rays(origins, directions):
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def _empty(N):
    return Hits(np.full(N, np.nan, D), np.full(N, np.nan, F), np.full(N, -1, np.int32), np.full((N, 2), np.nan, F), np.zeros(N, np.int8))


def _report(out, rows, t, U, V, W, det, tri):
    """Fill the rows of a Hits from the winner's numbers."""
    with np.errstate(all='ignore'):
        out.t[rows], out.depth[rows], out.triangle[rows] = t, t.astype(F), tri
        out.bary[rows] = np.stack([(V / det).astype(F), (W / det).astype(F)], 1)
        out.side[rows] = np.where(det > 0, 1, -1)


def scan_rays(origins, directions, grid, t_min=0.0, t_max=np.inf, chunk=128, double_rays=False):
    """The scan over all valid triangles for many rays at once -> Hits.  double_rays: origins / directions are float64 already."""
    kind = D if double_rays else F
    o, d = np.asarray(origins, kind).reshape(-1, 3), np.asarray(directions, kind).reshape(-1, 3)
    N, ids = len(o), np.flatnonzero(grid.valid)
    out = _empty(N)
    with np.errstate(invalid='ignore'):
        good = np.flatnonzero(np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1))
    out.t[good], out.depth[good] = np.inf, np.inf
    if len(ids) == 0:
        return out
    a, b, c = _corners(grid, ids)
    for s in range(0, len(good), chunk):
        rows = good[s:s + chunk]
        ok, t, U, V, W, det = ray_triangle(setup(o[rows].astype(D), d[rows].astype(D)), a, b, c, t_min, t_max)
        j = np.argmin(np.where(ok, t, np.inf), axis=1)                                              # the first of equals: ids ascend
        pick = np.arange(len(rows))
        hit = ok[pick, j]
        pick, j = pick[hit], j[hit]
        _report(out, rows[hit], t[pick, j], U[pick, j], V[pick, j], W[pick, j], det[pick, j], ids[j])
    return out


def _floorcell(v, cell, n):
    c = math.floor(v / cell)
    return 0 if not c > 0 else min(int(c), n - 1)


def cast_ray(o, d, grid, t_min=0.0, t_max=np.inf, brute_force=False, any_hit=False, stats=None):
    """One ray (o, d float64 [3], finite, d != 0) -> (t, triangle) of the first hit, (inf, -1) for a miss; any_hit: leaves at the first
    accepted triangle.  stats: a dict that receives `evaluated` and `cells`."""
    o, d = np.asarray(o, D), np.asarray(d, D)
    ray = setup(o[None], d[None])
    best = [np.inf, NONE]
    count = {'evaluated': 0, 'cells': 0}

    def fold(ids):
        """-> True when any_hit and one is accepted."""
        if len(ids) == 0:
            return False
        ids = np.asarray(ids, np.int64)
        count['evaluated'] += len(ids)
        ok, t, *_ = ray_triangle(ray, *_corners(grid, ids), t_min, t_max)
        ok, t = ok[0], t[0]
        if not ok.any():
            return False
        if any_hit:
            count['evaluated'] -= len(ids) - 1 - int(np.argmax(ok))                                 # the kernel leaves at the first one
            best[0], best[1] = 0.0, 0
            return True
        m = t[ok].min()
        tri = int(ids[ok & (t == m)].min())
        if m < best[0] or (m == best[0] and tri < best[1]):
            best[0], best[1] = float(m), tri
        return False

    def cell_list(cid):
        count['cells'] += 1
        return fold(grid.pair_triangle[grid.cell_start[cid]:grid.cell_start[cid + 1]])

    def walk():
        if len(grid.pair_triangle) == 0:
            return
        dims = grid.dims
        if dims[0] * dims[1] * dims[2] == 1:
            cell_list(0)
            return
        cell = float(grid.cell)
        k = [int(ray.kx[0]), int(ray.ky[0]), int(ray.kz[0])]
        stride = [(1, dims[0], dims[0] * dims[1])[c] for c in k]
        n = [dims[c] for c in k]
        lo = [float(grid.lo[c]) for c in k]
        oc = [float(o[c]) for c in k]
        dd = [float(d[c]) for c in k]
        a = [oc[c] - lo[c] for c in range(3)]
        top = [float(n[c]) * cell for c in range(3)]
        mag = 0.0
        for c in range(3):
            mag = mag + ((abs(oc[c]) + abs(lo[c])) + top[c])
        slack = mag * SLACK
        t0, t1 = float(t_min), float(t_max)
        for c in range(3):
            p0, p1 = -slack, top[c] + slack
            if dd[c] == 0.0:
                if not (p0 <= a[c] <= p1):
                    return
            else:
                with np.errstate(all='ignore'):
                    ta, tb = float(D(p0 - a[c]) / D(dd[c])), float(D(p1 - a[c]) / D(dd[c]))
                t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
        if not t0 <= t1:
            return
        Sz = float(ray.Sz[0])
        up = dd[2] > 0.0
        z0, z1 = a[2] + t0 * dd[2], a[2] + t1 * dd[2]
        s = _floorcell(z0 - slack if up else z0 + slack, cell, n[2])
        last = _floorcell(z1 + slack if up else z1 - slack, cell, n[2])
        for _ in range(n[2]):
            if not 0 <= s < n[2]:
                return
            ta, tb = ((float(s) * cell - slack) - a[2]) * Sz, ((float(s + 1) * cell + slack) - a[2]) * Sz
            te, tx = max(min(ta, tb), t0), min(max(ta, tb), t1)
            if te > best[0]:
                return
            if te <= tx:
                xa, xb, ya, yb = a[0] + te * dd[0], a[0] + tx * dd[0], a[1] + te * dd[1], a[1] + tx * dd[1]
                x0, x1 = _floorcell(min(xa, xb) - slack, cell, n[0]), _floorcell(max(xa, xb) + slack, cell, n[0])
                y0, y1 = _floorcell(min(ya, yb) - slack, cell, n[1]), _floorcell(max(ya, yb) + slack, cell, n[1])
                for y in range(y0, y1 + 1):
                    for x in range(x0, x1 + 1):
                        if cell_list(s * stride[2] + y * stride[1] + x * stride[0]):
                            return
            if s == last:
                return
            s += 1 if up else -1

    if brute_force:
        ids = np.flatnonzero(grid.valid)
        fold(ids)
    else:
        walk()
    if stats is not None:
        stats.update(count)
    return (best[0], best[1]) if best[1] != NONE else (np.inf, -1)


def first_hits(origins, directions, grid, t_min=0.0, t_max=np.inf, brute_force=False, evaluated=None, cells=None):
    """Ray by ray, the walk (or the scan) as the kernel takes it -> Hits."""
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    out = _empty(len(o))
    good = good_rays(o, d)
    for i in np.flatnonzero(good):
        stats = {}
        t, tri = cast_ray(o[i].astype(D), d[i].astype(D), grid, t_min, t_max, brute_force, stats=stats)
        if evaluated is not None:
            evaluated.append(stats['evaluated'])
        if cells is not None:
            cells.append(stats['cells'])
        out.t[i], out.depth[i] = np.inf, np.inf
        if tri >= 0:
            ok, t, U, V, W, det = ray_triangle(setup(o[i:i + 1].astype(D), d[i:i + 1].astype(D)), *_corners(grid, [tri]), t_min, t_max)
            assert ok[0, 0]
            _report(out, np.array([i]), t[0], U[0], V[0], W[0], det[0], tri)
    return out


def occluded(origins, directions, grid, t_min=0.0, t_max=np.inf, walk=False):
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    if not walk:
        return (scan_rays(o, d, grid, t_min, t_max).triangle >= 0).astype(np.uint8)
    good = good_rays(o, d)
    return np.array([good[i] and cast_ray(o[i].astype(D), d[i].astype(D), grid, t_min, t_max, any_hit=True)[1] >= 0 for i in range(len(o))], np.uint8)


# ------------------------------------------------------------------------------------------------ ambient occlusion
def ao_tables(rays, rotations=16):
    """fp32 [K,R,3]: a cosine-weighted spiral, u = (k + 1/2) / R, phi = k * golden angle + 2 pi j / K, (sqrt(u) cos, sqrt(u) sin, sqrt(1 - u))."""
    k = np.arange(rays, dtype=D)[None, :]
    j = np.arange(rotations, dtype=D)[:, None]
    u = (k + 0.5) / D(rays)
    phi = k * GOLDEN_ANGLE + ((2.0 * math.pi) * j) / D(rotations)
    r = np.sqrt(u)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.broadcast_to(np.sqrt(1.0 - u), phi.shape)], -1).astype(F)


def ao_rays(points, normals, tables, bias):
    """-> (ok bool [N], origins float64 [N,R,3], directions float64 [N,R,3])."""
    p, nr = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    tables = np.asarray(tables, F)
    K, R = tables.shape[:2]
    N = len(p)
    log2k = K.bit_length() - 1
    ok = np.isfinite(p).all(1) & np.isfinite(nr).all(1) & (nr != 0).any(1)
    j = np.array([0 if log2k == 0 else ((i * 2654435761) & 0xFFFFFFFF) >> (32 - log2k) for i in range(N)], np.int64)
    w = tables[j].astype(D) if N else np.zeros((0, R, 3))                                           # [N,R,3]
    with np.errstate(all='ignore'):
        n = nr.astype(D)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        nx, ny, nz = n[:, 0] / ln, n[:, 1] / ln, n[:, 2] / ln
        sg = np.where(nz >= 0.0, 1.0, -1.0)
        a = -1.0 / (sg + nz)
        b = (nx * ny) * a
        T = np.stack([1.0 + ((sg * nx) * nx) * a, sg * b, (-sg) * nx], 1)
        B = np.stack([b, sg + (ny * ny) * a, -ny], 1)
        Nn = np.stack([nx, ny, nz], 1)
        d = (w[..., 0:1] * T[:, None, :] + w[..., 1:2] * B[:, None, :]) + w[..., 2:3] * Nn[:, None, :]
        o = np.broadcast_to(p.astype(D)[:, None, :] + D(F(bias)) * Nn[:, None, :], d.shape)
    return ok, o, d


def ambient_occlusion(points, normals, grid, tables, bias, radius=np.inf, walk=False):
    """-> fp32 [N]: unoccluded / R.  The any-hit answer is `some valid triangle is accepted`: the scan says it for all rays at once;
    walk=True takes the kernel's walk ray by ray."""
    ok, o, d = ao_rays(points, normals, tables, bias)
    N, R = o.shape[:2]
    out = np.full(N, np.nan, F)
    rows = np.flatnonzero(ok)
    if len(rows) == 0:
        return out
    oo, dd = o[rows].reshape(-1, 3), d[rows].reshape(-1, 3)
    radius = float(D(F(radius)))
    if walk:
        fine = np.isfinite(oo).all(1) & np.isfinite(dd).all(1) & (dd != 0).any(1)
        hit = np.array([bool(fine[i]) and cast_ray(oo[i], dd[i], grid, 0.0, radius, any_hit=True)[1] >= 0 for i in range(len(oo))])
    else:
        hit = scan_rays(oo, dd, grid, 0.0, radius, double_rays=True).triangle >= 0
    free = (~hit).reshape(len(rows), R).sum(1)
    out[rows] = free.astype(F) / F(R)
    return out


# ------------------------------------------------------------------------------------------------ the rays of the tests
def _unit(rs, n):
    d = rs.randn(n, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def adversarial_rays(grid, seed=3):
    """254 rays against the mesh of `grid` (take the finest grid of a mesh) -> (origins, directions) fp32 [254,3]: origins inside the box and
    up to 4x outside it, rays that miss the box, axis-parallel rays, rays lying in a cell face, through cell corners and along cell edges,
    aimed at vertices and at fp32-rounded edge midpoints, and starting on the surface."""
    rs = np.random.RandomState(seed)
    lo, hi = np.array(grid.lo, D), np.array(grid.hi, D)
    ext = np.maximum(hi - lo, 1.0)
    cell = grid.cell if math.isfinite(grid.cell) else 1.0
    dims = np.array(grid.dims)
    v = np.asarray(grid.vertices, F)
    ids = np.flatnonzero(grid.valid)
    tri = np.asarray(grid.triangles, np.int64)[ids]
    O, Dr = [], []

    def add(o, d):
        O.append(np.asarray(o, D).reshape(-1, 3).astype(F))
        Dr.append(np.asarray(d, D).reshape(-1, 3).astype(F))

    def inside(n):
        return lo + rs.rand(n, 3) * (hi - lo)

    def outside(n):
        return lo - 4 * ext + rs.rand(n, 3) * 9 * ext

    def corners(n):
        return (lo + np.floor(rs.rand(n, 3) * (dims + 1)) * cell).astype(F).astype(D)

    add(inside(40), _unit(rs, 40) * (0.25 + 4 * rs.rand(40, 1)))
    o = outside(40).astype(F).astype(D)
    add(o, inside(40) - o)                                                                      # aimed into the box
    o = outside(16).astype(F).astype(D)
    add(o, (o - (lo + hi) / 2) + _unit(rs, 16) * 0.1)                                            # pointing away from it
    axis = np.eye(3)[rs.randint(0, 3, 24)] * np.where(rs.rand(24, 1) < 0.5, -1.0, 1.0) * (2.0 ** rs.randint(-2, 3, (24, 1)))
    o = np.concatenate([inside(12), outside(12)])
    o[12:] = np.where(axis[12:] != 0, o[12:], inside(12))                                        # outside along the ray's own axis only
    add(o, axis)
    o, d, k = corners(20), _unit(rs, 20), rs.randint(0, 3, 20)                                   # in a cell face: one coordinate on a plane, no motion along it
    free = rs.rand(20, 3) < 0.5
    o = np.where(free & (np.arange(3)[None] != k[:, None]), inside(20), o)
    d[np.arange(20), k] = 0.0
    add(o, d)
    o = outside(20).astype(F).astype(D)
    add(o, corners(20) - o)                                                                     # through a cell corner
    add(corners(16), np.eye(3)[rs.randint(0, 3, 16)] * np.where(rs.rand(16, 1) < 0.5, -1.0, 1.0))     # along a cell edge
    if len(tri):
        target = v[tri[rs.randint(0, len(tri), 30), rs.randint(0, 3, 30)]].astype(D)
        step = rs.randint(-8, 9, (30, 3)) * 0.25
        step[(step == 0).all(1)] = (0.25, -0.5, 1.0)
        o = np.where(np.arange(30)[:, None] < 15, (target - step).astype(F).astype(D), outside(30).astype(F).astype(D))
        add(o, target - o)                                                                      # at a vertex (the first 15: an offset of few bits, d exact)
        t = tri[rs.randint(0, len(tri), 20)]
        e = rs.randint(0, 3, 20)
        mid = ((v[t[np.arange(20), e]].astype(D) + v[t[np.arange(20), (e + 1) % 3]].astype(D)) / 2.0).astype(F).astype(D)
        o = np.concatenate([inside(10), outside(10)]).astype(F).astype(D)
        add(o, mid - o)                                                                         # at an edge midpoint
        t = tri[rs.randint(0, len(tri), 28)]
        w = rs.dirichlet((1, 1, 1), 28)
        on = (v[t].astype(D) * w[:, :, None]).sum(1)
        on[:10] = v[t[:10, 0]]                                                                  # on a vertex; the others on a face, rounded
        add(on, _unit(rs, 28))                                                                  # starting on the surface
    else:
        add(inside(78), _unit(rs, 78))
    o, d = np.concatenate(O), np.concatenate(Dr)
    assert o.shape == d.shape == (254, 3)
    zero = (d == 0).all(1)
    d[zero] = (1.0, 0.0, 0.0)
    return o, d

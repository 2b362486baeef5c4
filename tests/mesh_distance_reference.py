"""The mesh-distance contract of include/tdgp.h in IEEE doubles, every operation rounded once in the order written (numpy float64 arrays:
elementwise operations, one ufunc per operation, so nothing is fused): the yardstick the kernels of csrc/mesh_distance.hip are compared with
bit for bit.  Arrays over the triangles stand for the loop over them; the minimum with ties to the smallest index makes the order irrelevant."""
import collections
import math

import numpy as np

F = np.float32
D = np.float64
TriangleGrid = collections.namedtuple('TriangleGrid', ['vertices', 'triangles', 'valid', 'lo', 'hi', 'cell', 'dims', 'cell_start', 'pair_triangle', 'valid_count'])
Closest = collections.namedtuple('Closest', ['sqdist', 'distance', 'triangle', 'point'])
Samples = collections.namedtuple('Samples', ['points', 'weight', 'triangle'])
Stats = collections.namedtuple('Stats', ['max', 'mean', 'rms', 'area', 'argmax_sample', 'samples'])
MeshDistance = collections.namedtuple('MeshDistance', ['a_to_b', 'b_to_a', 'hausdorff', 'mean', 'rms'])
CELLS_MAX, PAIRS_MAX, K_MAX, BLOCK = 1 << 24, 2 ** 31 - 1, 64, 256


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2], x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def _edge(p, x, y, d2, q):
    e = y - x
    ee = dot(e, e)
    with np.errstate(invalid='ignore', divide='ignore'):
        t = np.where(ee != 0.0, dot(p - x, e) / ee, 0.0)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    r = x + t[..., None] * e
    d = p - r
    dd = dot(d, d)
    take = dd < d2
    return np.where(take, dd, d2), np.where(take[..., None], r, q)


def point_triangle(p, a, b, c):
    """d2 and the closest point of p [..,3] to the triangles (a, b, c) [..,3], all float64 (broadcast against each other)."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, D) for x in (p, a, b, c)))
    ab, ac, ap = b - a, c - a, p - a
    n = cross(ab, ac)
    nn = dot(n, n)
    s0 = dot(cross(c - b, p - b), n)
    s1 = dot(cross(a - c, p - c), n)
    s2 = dot(cross(ab, ap), n)
    face = (nn > 0.0) & (s0 >= 0.0) & (s1 >= 0.0) & (s2 >= 0.0)
    s = dot(ap, n)
    with np.errstate(invalid='ignore', divide='ignore'):
        f = s / nn
        qf = p - n * f[..., None]
        df = s * s / nn
    d2 = np.full(nn.shape, np.inf)
    q = np.zeros(p.shape)
    for x, y in ((a, b), (b, c), (c, a)):
        d2, q = _edge(p, x, y, d2, q)
    return np.where(face, df, d2), np.where(face[..., None], qf, q)


def valid_triangles(vertices, triangles):
    v, t = np.asarray(vertices, F), np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    safe = np.where(ok[:, None], t, 0)
    if len(v):
        ok &= np.isfinite(v[safe]).all((1, 2))
    return ok


def _corners(vertices, triangles, ids):
    v = np.asarray(vertices, F).astype(D)
    t = np.asarray(triangles, np.int64)[ids]
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def prepare(vertices, triangles):
    """-> (valid bool [T], box fp32 [T,6], area float64 [T])."""
    ok = valid_triangles(vertices, triangles)
    T = len(ok)
    box, area = np.zeros((T, 6), F), np.zeros(T, D)
    ids = np.flatnonzero(ok)
    if len(ids):
        c = np.asarray(vertices, F)[np.asarray(triangles, np.int64)[ids]]                      # [n,3 corners,3]
        box[ids, :3], box[ids, 3:] = c.min(1), c.max(1)
        a, b, cc = _corners(vertices, triangles, ids)
        n = cross(b - a, cc - a)
        area[ids] = 0.5 * np.sqrt(dot(n, n))
    return ok, box, area


def _tree(x):
    """[rows, 256] -> [rows]: slot i takes slot i + s for s = 128 .. 1."""
    x = x.copy()
    s = BLOCK // 2
    while s >= 1:
        x[:, :s] = x[:, :s] + x[:, s:2 * s]
        s //= 2
    return x[:, 0]


def fixed_sum(x):
    """The sum of tdgp_mesh_distance_reduce: blocks of 256 as trees, then slot t adds block results t, t + 256, ... from 0, then the tree."""
    x = np.asarray(x, D)
    nb = -(-len(x) // BLOCK)
    if nb == 0:
        return 0.0
    part = _tree(np.concatenate([x, np.zeros(nb * BLOCK - len(x))]).reshape(nb, BLOCK))
    rows = -(-nb // BLOCK)
    part = np.concatenate([part, np.zeros(rows * BLOCK - nb)]).reshape(rows, BLOCK)
    acc = np.zeros(BLOCK)
    for r in range(rows):
        acc = acc + part[r]
    return float(_tree(acc[None])[0])


def reduce(weight, distance):
    """-> (sum w, sum w d, sum w (d d), max d, argmax)."""
    w = np.asarray(weight, D)
    d32 = np.asarray(distance, F)
    d = d32.astype(D)
    with np.errstate(invalid='ignore', over='ignore'):
        sums = fixed_sum(w), fixed_sum(w * d), fixed_sum(w * (d * d))
    ok = ~np.isnan(d32)
    if not ok.any():
        return sums + (0.0, -1)
    m = d32[ok].max()
    return sums + (float(m), int(np.flatnonzero(ok & (d32 == m))[0]))


def default_cell(vertices, triangles):
    ok, _, area = prepare(vertices, triangles)
    n = int(ok.sum())
    if n == 0:
        return 1.0
    c = float(F(2.0 * math.sqrt(fixed_sum(area) / n)))
    return c if math.isfinite(c) and c > 0 else 1.0


def cell_of(x, lo, cell, n):
    """floor((x - lo) / cell) clamped into [0, n - 1], on float64 arrays."""
    with np.errstate(invalid='ignore', over='ignore'):
        v = np.floor((np.asarray(x, D) - lo) / cell)
    return np.where(~(v > 0.0), 0, np.where(v >= n - 1, n - 1, v)).astype(np.int64)


def build_grid(vertices, triangles, cell=None):
    vertices, triangles = np.ascontiguousarray(vertices, F), np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    ok, box, area = prepare(vertices, triangles)
    count = int(ok.sum())
    cell = default_cell(vertices, triangles) if cell is None else float(F(cell))
    assert cell > 0
    if count == 0:
        return TriangleGrid(vertices, triangles, ok.astype(np.uint8), (0.0,) * 3, (0.0,) * 3, cell, (1, 1, 1), np.zeros(2, np.int32), np.zeros(0, np.int32), 0)
    ids = np.flatnonzero(ok)
    lo = tuple(float(x) for x in box[ids, :3].min(0))
    hi = tuple(float(x) for x in box[ids, 3:].max(0))
    while True:
        dims = tuple(int(math.floor((h - l) / cell)) + 1 for l, h in zip(lo, hi))
        if dims[0] * dims[1] * dims[2] <= CELLS_MAX:
            c0 = np.stack([cell_of(box[ids, k].astype(D), lo[k], cell, dims[k]) for k in range(3)], 1)
            c1 = np.maximum(np.stack([cell_of(box[ids, 3 + k].astype(D), lo[k], cell, dims[k]) for k in range(3)], 1), c0)
            if int((c1 - c0 + 1).prod(1).sum()) <= PAIRS_MAX:
                break
        with np.errstate(over='ignore'):
            cell = float(F(cell) * F(2))
    lists = collections.defaultdict(list)
    for t, a, b in zip(ids.tolist(), c0.tolist(), c1.tolist()):                                     # ascending t: every list ascends
        for z in range(a[2], b[2] + 1):
            for y in range(a[1], b[1] + 1):
                for x in range(a[0], b[0] + 1):
                    lists[(z * dims[1] + y) * dims[0] + x].append(t)
    cells = dims[0] * dims[1] * dims[2]
    sizes = np.zeros(cells, np.int64)
    for c, l in lists.items():
        sizes[c] = len(l)
    cell_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pairs = np.array([t for c in sorted(lists) for t in lists[c]], np.int32)
    return TriangleGrid(vertices, triangles, ok.astype(np.uint8), lo, hi, cell, dims, cell_start, pairs, count)


def _best(p, grid, ids, best):
    """Fold the triangles `ids` into the running (d2, id)."""
    if len(ids) == 0:
        return best
    ids = np.asarray(ids, np.int64)
    a, b, c = _corners(grid.vertices, grid.triangles, ids)
    d2, _ = point_triangle(p, a, b, c)
    m = d2.min()
    t = int(ids[d2 == m].min())
    if m < best[0] or (m == best[0] and t < best[1]):
        return float(m), t
    return best


def _finish(p, grid, best):
    if best[1] < 0:
        return np.inf, F(np.inf), -1, np.full(3, np.nan, F)
    a, b, c = _corners(grid.vertices, grid.triangles, np.array([best[1]]))
    d2, q = point_triangle(p, a, b, c)
    return float(d2[0]), F(math.sqrt(d2[0])), best[1], q[0].astype(F)


NONE = (np.inf, 2 ** 31 - 1)


def closest_point(p32, grid, brute_force=False, evaluated=None):
    """One point -> (sqdist, distance fp32, triangle, point fp32 [3]); evaluated: a list that receives the number of d2 evaluations."""
    p32 = np.asarray(p32, F)
    if not np.isfinite(p32).all():
        return np.nan, F(np.nan), -1, np.full(3, np.nan, F)
    p = p32.astype(D)
    best, count = NONE, 0
    if brute_force:
        ids = np.flatnonzero(grid.valid)
        best, count = _best(p, grid, ids, best), len(ids)
    elif len(grid.pair_triangle):
        lo, n, cell = grid.lo, grid.dims, grid.cell
        c = [int(cell_of(p[k], lo[k], cell, n[k])) for k in range(3)]
        a = [float(p[k] - lo[k]) for k in range(3)]
        for r in range(max(n)):
            rng = [range(max(c[k] - r, 0), min(c[k] + r, n[k] - 1) + 1) for k in range(3)]
            for z in rng[2]:
                for y in rng[1]:
                    for x in rng[0]:
                        if max(abs(x - c[0]), abs(y - c[1]), abs(z - c[2])) != r:
                            continue
                        cid = (z * n[1] + y) * n[0] + x
                        ids = grid.pair_triangle[grid.cell_start[cid]:grid.cell_start[cid + 1]]
                        best, count = _best(p, grid, ids, best), count + len(ids)
            lb, is_open = np.inf, False
            for k in range(3):
                if c[k] - r > 0:
                    mc = float(c[k] - r) * cell
                    d = (a[k] - mc) - (abs(a[k]) + mc) * 2.0 ** -48
                    lb, is_open = min(lb, d if d > 0.0 else 0.0), True
                if c[k] + r < n[k] - 1:
                    mc = float(c[k] + r + 1) * cell
                    d = (mc - a[k]) - (abs(a[k]) + mc) * 2.0 ** -48
                    lb, is_open = min(lb, d if d > 0.0 else 0.0), True
            if not is_open:
                break
            if (lb * lb) * (1.0 - 2.0 ** -40) > best[0]:
                break
    if evaluated is not None:
        evaluated.append(count)
    return _finish(p, grid, best if best[1] != NONE[1] else (np.inf, -1))


def scan_points(points, grid, chunk=256):
    """The scan over all valid triangles for many points at once (the same elementwise operations, [points, triangles] arrays)."""
    points = np.asarray(points, F).reshape(-1, 3)
    N, ids = len(points), np.flatnonzero(grid.valid)
    out = Closest(np.full(N, np.nan, D), np.full(N, np.nan, F), np.full(N, -1, np.int32), np.full((N, 3), np.nan, F))
    finite = np.flatnonzero(np.isfinite(points).all(1))
    if len(ids) == 0:
        out.sqdist[finite], out.distance[finite] = np.inf, np.inf
        return out
    a, b, c = _corners(grid.vertices, grid.triangles, ids)
    for s in range(0, len(finite), chunk):
        rows = finite[s:s + chunk]
        p = points[rows].astype(D)[:, None, :]
        d2, q = point_triangle(p, a[None], b[None], c[None])
        j = np.argmin(d2, axis=1)                                                                   # the first of equals: ids ascend
        pick = np.arange(len(rows))
        out.sqdist[rows], out.triangle[rows] = d2[pick, j], ids[j]
        out.distance[rows], out.point[rows] = np.sqrt(d2[pick, j]).astype(F), q[pick, j].astype(F)
    return out


def closest_points(points, grid, brute_force=False, evaluated=None):
    points = np.asarray(points, F).reshape(-1, 3)
    if brute_force and evaluated is None:
        return scan_points(points, grid)
    rows = [closest_point(p, grid, brute_force, evaluated) for p in points]
    return Closest(np.array([r[0] for r in rows], D), np.array([r[1] for r in rows], F), np.array([r[2] for r in rows], np.int32),
                   np.array([r[3] for r in rows], F).reshape(-1, 3))


def subdivisions(a, b, c, spacing):
    l2 = max(float(dot(b - a, b - a)), float(dot(c - b, c - b)), float(dot(a - c, a - c)))
    k = math.ceil(math.sqrt(l2) / spacing)
    return 1 if not k > 1 else min(int(k), K_MAX)


def sample_surface(vertices, triangles, spacing=None):
    vertices, triangles = np.asarray(vertices, F), np.asarray(triangles, np.int32).reshape(-1, 3)
    spacing = default_cell(vertices, triangles) if spacing is None else float(F(spacing))
    pts, wts, ids = [], [], []
    for t in np.flatnonzero(valid_triangles(vertices, triangles)).tolist():
        a, b, c = (vertices[i].astype(D) for i in triangles[t])
        k = subdivisions(a, b, c, spacing)
        ab, ac = b - a, c - a
        n = cross(ab, ac)
        w = (0.5 * math.sqrt(float(dot(n, n)))) / float(k * k)
        for i in triangles[t]:
            pts.append(vertices[i])
            wts.append(0.0)
        for third, less in ((1.0 / 3.0, 0), (2.0 / 3.0, 1)):
            for i in range(k - less):
                for j in range(k - less - i):
                    u, v = (float(i) + third) / float(k), (float(j) + third) / float(k)
                    pts.append(((a + u * ab) + v * ac).astype(F))
                    wts.append(w)
        ids += [t] * (k * k + 3)
    return Samples(np.array(pts, F).reshape(-1, 3), np.array(wts, D), np.array(ids, np.int32))


def stats_from_sums(sum_w, sum_wd, sum_wdd, d_max, argmax, samples):
    mean = sum_wd / sum_w if sum_w > 0 else float('nan')
    rms = math.sqrt(sum_wdd / sum_w) if sum_w > 0 and sum_wdd >= 0 else float('nan')
    return Stats(d_max if argmax >= 0 else float('nan'), mean, rms, sum_w, argmax, samples)


def one_sided(samples, grid, brute_force=False):
    c = closest_points(samples.points, grid, brute_force)
    return stats_from_sums(*reduce(samples.weight, c.distance), len(samples.points))


def pool(a, b):
    area = a.area + b.area
    if not area > 0:
        return float('nan'), float('nan')
    return (a.mean * a.area + b.mean * b.area) / area, math.sqrt(((a.rms * a.rms) * a.area + (b.rms * b.rms) * b.area) / area)


def mesh_distance(va, ta, vb, tb, spacing=None, symmetric=True, brute_force=False):
    ab = one_sided(sample_surface(va, ta, spacing), build_grid(vb, tb), brute_force)
    if not symmetric:
        return MeshDistance(ab, None, ab.max, ab.mean, ab.rms)
    ba = one_sided(sample_surface(vb, tb, spacing), build_grid(va, ta), brute_force)
    mean, rms = pool(ab, ba)
    worst = [m for m in (ab.max, ba.max) if not math.isnan(m)]
    return MeshDistance(ab, ba, max(worst) if worst else float('nan'), mean, rms)


# ------------------------------------------------------------------------------------------------ meshes of the tests
def soup(T=120, seed=0, extent=4.0):
    """Random triangles over [0, extent]^3 with a collinear one, one with two coincident vertices, an index out of range, a repeated index
    and a vertex that is not finite -> (vertices fp32 [3T + 1, 3], triangles int32 [T,3])."""
    rs = np.random.RandomState(seed)
    centre = rs.rand(T, 1, 3) * extent
    v = (centre + (rs.rand(T, 3, 3) - 0.5) * (extent / 4)).reshape(-1, 3).astype(F)
    t = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    v[15:18] = [[1, 1, 1], [1.5, 1.25, 1], [2, 1.5, 1]]                                         # triangle 5: collinear, exactly
    v[3 * 9 + 1] = v[3 * 9]                                                                     # triangle 9: two vertices coincide
    t[12] = (3, 3 * T + 7, 5)                                                                   # out of range
    t[13] = (40, 40, 41)                                                                        # a repeated index
    v = np.concatenate([v, np.array([[np.nan, 0, 0]], F)])
    t[14] = (0, 1, 3 * T)                                                                       # names the vertex that is not finite
    t[15] = (-1, 2, 3)
    return v, t


def query_points(grid, seed=1, n=40):
    """Points inside the box, up to 4x outside it, on vertices and exactly on cell faces -> fp32 [.,3]."""
    rs = np.random.RandomState(seed)
    lo, hi = np.array(grid.lo), np.array(grid.hi)
    ext = np.maximum(hi - lo, 1.0)
    inside = lo + rs.rand(n, 3) * (hi - lo)
    outside = lo - 4 * ext + rs.rand(n, 3) * 9 * ext
    ids = np.flatnonzero(grid.valid)
    on_vertices = grid.vertices[grid.triangles[ids[rs.randint(0, len(ids), n // 2)], rs.randint(0, 3, n // 2)]] if len(ids) else np.zeros((0, 3))
    faces = lo + np.floor(rs.rand(n // 2, 3) * np.array(grid.dims)) * (grid.cell if math.isfinite(grid.cell) else 0.0)
    return np.concatenate([inside, outside, on_vertices, faces]).astype(F)

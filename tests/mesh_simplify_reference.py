"""The yardstick of the mesh-simplification tests: the contracts of tdgp_mesh_cluster_keys / _ids / _triangles_relabel / _triangles_count /
_triangles_emit / _place / _attribute (include/tdgp.h) restated in numpy, operation for operation -- float64 scalars and element-wise
arrays whose every operation numpy rounds once (never fusing a multiply into an add, `/`, `floor` and `sqrt` correctly rounded), sums in
plain loops in the contract's order -- plus `simplify`, the driver, the ladder of `cell_for_triangles`, and the box the tests share.
Written from the contract, for these tests."""
import collections

import numpy as np

import mesh_surface_reference as SR

F = np.float32
D = np.float64
K_HALF = 2 ** 20
K_BITS = 21

Simplified = collections.namedtuple('Simplified', ['vertices', 'triangles', 'attributes', 'cluster', 'triangle_map', 'order', 'start', 'key', 'fallback'])


def grid(cell, origin=(0, 0, 0)):
    cell = np.array(cell if isinstance(cell, (tuple, list)) else (cell,) * 3, D)
    return cell, np.array(origin, D)


def cell_keys(vertices, cell, origin=(0, 0, 0)):
    """-> key int64 [V]: ((q2 + 2^20) * 2^21 + (q1 + 2^20)) * 2^21 + (q0 + 2^20), or -1."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    cell, origin = grid(cell, origin)
    with np.errstate(all='ignore'):
        q = np.floor((v.astype(D) - origin) / cell)
        ok = ((q >= -K_HALF) & (q < K_HALF)).all(axis=1)                   # false for NaN
    k = np.where(ok[:, None], q, 0).astype(np.int64) + K_HALF
    key = (((k[:, 2] << K_BITS) + k[:, 1]) << K_BITS) + k[:, 0]
    return np.where(ok, key, -1).astype(np.int64)


def cluster_vertices(vertices, cell, origin=(0, 0, 0)):
    """-> (cluster int32 [V], order int32 [V], start int32 [C+1], key int64 [C])."""
    key = cell_keys(vertices, cell, origin)
    V = len(key)
    order = np.argsort(key, kind='stable').astype(np.int32)
    cluster = np.full(V, -1, np.int32)
    start, ckey = [], []
    for i in range(V):
        k = key[order[i]]
        if k < 0:
            continue
        if i == 0 or key[order[i - 1]] != k:
            start.append(i)
            ckey.append(k)
        cluster[order[i]] = len(ckey) - 1
    start.append(V)
    return cluster, order, np.array(start, np.int32), np.array(ckey, np.int64).reshape(-1)


def rotate(triple):
    a, b, c = (int(x) for x in triple)
    s = 0 if (a < b and a < c) else (1 if b < c else 2)
    t = (a, b, c)
    return t[s], t[(s + 1) % 3], t[(s + 2) % 3]


def cluster_triangles(triangles, V, cluster, dedup=True):
    """-> (cluster_triangles int32 [T,3], out_triangles int32 [T',3], triangle_map int32 [T'])."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    ct = np.full((len(tri), 3), -1, np.int32)
    out, tmap, seen = [], [], set()
    for t in range(len(tri)):
        if not ((tri[t] >= 0) & (tri[t] < V)).all():
            continue
        c = np.maximum(cluster[tri[t]], -1)
        ct[t] = c
        if (c < 0).any() or c[0] == c[1] or c[1] == c[2] or c[0] == c[2]:
            continue
        r = rotate(c)
        if dedup and r in seen:
            continue
        seen.add(r)
        out.append(c)
        tmap.append(t)
    return ct, np.array(out, np.int32).reshape(-1, 3), np.array(tmap, np.int32).reshape(-1)


def count_triangles(vertices, triangles, cell, origin=(0, 0, 0), dedup=True):
    v = np.asarray(vertices, F).reshape(-1, 3)
    return len(cluster_triangles(triangles, len(v), cluster_vertices(v, cell, origin)[0], dedup)[2])


def _jacobi_rotate(a, u, p, q, r):
    apq = a[p][q]
    if apq == 0:
        return
    theta = (a[q][q] - a[p][p]) / (D(2) * apq)
    den = np.abs(theta) + np.sqrt(theta * theta + D(1))
    t = (D(1) if theta >= 0 else D(-1)) / den
    c = D(1) / np.sqrt(t * t + D(1))
    s = t * c
    a[p][p] = a[p][p] - t * apq
    a[q][q] = a[q][q] + t * apq
    a[p][q] = a[q][p] = D(0)
    arp, arq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for k in range(3):
        ukp, ukq = u[k][p], u[k][q]
        u[k][p] = c * ukp - s * ukq
        u[k][q] = s * ukp + c * ukq


def cell_centres(key, cell, origin):
    mask = (1 << K_BITS) - 1
    key = np.asarray(key, np.int64)
    k = np.stack([(key & mask) - K_HALF, ((key >> K_BITS) & mask) - K_HALF, ((key >> (2 * K_BITS)) & mask) - K_HALF], axis=-1)
    return origin + (k.astype(D) + D(0.5)) * cell


def place(vertices, triangles, order, start, key, cell, origin=(0, 0, 0), corner_start=None, corner=None, placement='quadric', rank_tol=1e-3):
    """-> (out fp32 [C,3], fallback uint8 [C])."""
    v, tri = np.asarray(vertices, F).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T, C = len(v), len(tri), len(key)
    cell, origin = grid(cell, origin)
    centre = cell_centres(key, cell, origin).reshape(C, 3)
    out, fallback = np.zeros((C, 3), F), np.zeros(C, np.uint8)
    rank_tol = D(rank_tol)
    with np.errstate(all='ignore'):
        for cl in range(C):
            ce = centre[cl]
            s, members = np.zeros(3, D), 0
            for j in range(int(start[cl]), int(start[cl + 1])):
                s = s + (v[order[j]].astype(D) - ce)
                members += 1
            m = s / D(members) if members else s
            x = m.copy()
            if placement == 'quadric':
                A = [[D(0)] * 3 for _ in range(3)]
                b = [D(0)] * 3
                corners = 0
                for j in range(*SR._range(corner_start, cl, C, T)):
                    cid = int(corner[j])
                    if cid < 0 or cid >= 3 * T:
                        continue
                    idx = tri[cid // 3]
                    if not ((idx >= 0) & (idx < V)).all():
                        continue
                    p0 = v[idx[0]].astype(D) - ce
                    e1 = (v[idx[1]].astype(D) - ce) - p0
                    e2 = (v[idx[2]].astype(D) - ce) - p0
                    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                    d = -((n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2])
                    for r in range(3):
                        for c in range(r, 3):
                            A[r][c] = A[r][c] + n[r] * n[c]
                        b[r] = b[r] + n[r] * d
                    corners += 1
                if corners:
                    A[1][0], A[2][0], A[2][1] = A[0][1], A[0][2], A[1][2]
                    r_ = [-b[c] - ((A[c][0] * m[0] + A[c][1] * m[1]) + A[c][2] * m[2]) for c in range(3)]
                    a = [list(row) for row in A]
                    u = [[D(1 if i == j else 0) for j in range(3)] for i in range(3)]
                    for _ in range(8):
                        _jacobi_rotate(a, u, 0, 1, 2)
                        _jacobi_rotate(a, u, 0, 2, 1)
                        _jacobi_rotate(a, u, 1, 2, 0)
                    lmax = a[0][0]
                    lmax = a[1][1] if a[1][1] > lmax else lmax
                    lmax = a[2][2] if a[2][2] > lmax else lmax
                    floor_l = rank_tol * lmax
                    for i in range(3):
                        if a[i][i] > floor_l:
                            coef = ((u[0][i] * r_[0] + u[1][i] * r_[1]) + u[2][i] * r_[2]) / a[i][i]
                            for c in range(3):
                                x[c] = x[c] + u[c][i] * coef
                    half = cell * D(0.5)
                    if not all(x[c] >= -half[c] and x[c] <= half[c] for c in range(3)):
                        fallback[cl] = 1
                        x = m.copy()
            out[cl] = (ce + x).astype(F)
    return out, fallback


def attribute_means(attribute, order, start):
    a = np.asarray(attribute, F)
    C = len(start) - 1
    out = np.zeros((C, a.shape[1]), F)
    for cl in range(C):
        s, members = np.zeros(a.shape[1], D), 0
        for j in range(int(start[cl]), int(start[cl + 1])):
            s = s + a[order[j]].astype(D)
            members += 1
        if members:
            out[cl] = (s / D(members)).astype(F)
    return out


def simplify(vertices, triangles, cell, origin=(0, 0, 0), placement='quadric', rank_tol=1e-3, dedup=True, attributes=()):
    v = np.asarray(vertices, F).reshape(-1, 3)
    cluster, order, start, key = cluster_vertices(v, cell, origin)
    ct, out_t, tmap = cluster_triangles(triangles, len(v), cluster, dedup)
    cstart, ccorner = SR.corner_table(ct, len(key))[:2] if placement == 'quadric' else (None, None)
    out_v, fallback = place(v, triangles, order, start, key, cell, origin, cstart, ccorner, placement, rank_tol)
    return Simplified(out_v, out_t, tuple(attribute_means(a, order, start) for a in attributes), cluster, tmap, order, start, key, fallback)


def ladder(cell_min=1.0, steps=12):
    return [float(cell_min) * 2.0 ** (j / 2.0) for j in range(steps)]


def cell_for_triangles(vertices, triangles, max_triangles, cell_min=1.0, steps=12, origin=(0, 0, 0)):
    """-> (cell, the counts of the rungs walked)."""
    counts = []
    for cell in ladder(cell_min, steps):
        counts.append(count_triangles(vertices, triangles, cell, origin))
        if counts[-1] <= max_triangles:
            return cell, counts
    return None, counts


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def box(n=12, shift=(0.5, 0.5, 0.5)):
    """The surface of the cube [0, n]^3 + shift, every unit square two triangles wound outward -> (vertices fp32 [V,3], triangles int32
    [12 n^2, 3], lo, hi).  With the default shift every coordinate is exact in fp32 and no vertex lies on a lattice plane of cell 4."""
    ids, verts, tris = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def pt(a, b):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, a, b
                        return vid(tuple(p))
                    q = [pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)]          # counter-clockwise seen from +axis
                    if side == 0:
                        q = q[::-1]
                    tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    lo = np.array(shift, D)
    return (np.array(verts, D) + lo).astype(F), np.array(tris, np.int32), lo, lo + n


def box_surface_distance(points, lo, hi):
    """Distance of every point from the surface of the axis-aligned box [lo, hi], in float64."""
    p = np.asarray(points, D).reshape(-1, 3)
    outside = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    d_out = np.sqrt((outside ** 2).sum(1))
    d_in = np.minimum(p - lo, hi - p).min(1)
    return np.where(d_out > 0, d_out, np.abs(d_in))

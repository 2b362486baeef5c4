"""The yardstick of the mesh-decimation tests: the contracts of tdgp_mesh_decimate_quadrics / _candidates / _claim / _select / _apply / _gather
(include/tdgp.h) and the driver `mesh_decimate.decimate` restated operation for operation.  The scalar chains are Python floats -- IEEE
doubles whose every `+ - * /` and `math.sqrt` is rounded once, never fused -- in the contract's order; `np.float32(x)` rounds to nearest
even.  A candidate's verdict depends only on the state of {a, b} u N(a) u N(b) (not on the numbering of the triangles: only the key's
tie-break reads the corner id), so `cache=True` re-evaluates an edge only when a collapse of the previous round touched that neighbourhood;
`cache=False` evaluates every edge every round, and the tests hold the two against each other.  Written from the contract, for these tests."""
import collections
import math

import numpy as np

import mesh_components_reference as CR
import mesh_surface_reference as SR

F = np.float32
D = np.float64
NONE = (1 << 64) - 1
INF = float('inf')

Decimated = collections.namedtuple('Decimated', ['vertices', 'triangles', 'attributes', 'vertex_map', 'triangle_map', 'rounds', 'stopped'])


def mix(h):
    h &= 0xffffffff
    h ^= h >> 16
    h = (h * 0x7feb352d) & 0xffffffff
    h ^= h >> 15
    h = (h * 0x846ca68b) & 0xffffffff
    return h ^ (h >> 16)


def max_collapses(T, target):
    return max(0, (T - target + 1) // 2)


def _div(a, b):
    """a / b as IEEE rounds it, a zero divisor included."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return float('nan')
    return math.copysign(INF, a) * math.copysign(1.0, b)


def _cross(p0, p1, p2):
    e1 = (p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2])
    e2 = (p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2])
    return (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])


def _jacobi_rotate(a, u, p, q, r):
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = _div(a[q][q] - a[p][p], 2.0 * apq)
    den = abs(theta) + math.sqrt(theta * theta + 1.0)
    t = _div(1.0 if theta >= 0.0 else -1.0, den)
    c = _div(1.0, math.sqrt(t * t + 1.0))
    s = t * c
    a[p][p] = a[p][p] - t * apq
    a[q][q] = a[q][q] + t * apq
    a[p][q] = a[q][p] = 0.0
    arp, arq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for k in range(3):
        ukp, ukq = u[k][p], u[k][q]
        u[k][p] = c * ukp - s * ukq
        u[k][q] = s * ukp + c * ukq


def minimise(A, bv, m, rank_tol):
    """csrc/quadric_solve.h: the rank-limited minimiser of x^T A x + 2 bv^T x started from m."""
    r = [-bv[c] - ((A[c][0] * m[0] + A[c][1] * m[1]) + A[c][2] * m[2]) for c in range(3)]
    a = [list(row) for row in A]
    u = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(8):
        _jacobi_rotate(a, u, 0, 1, 2)
        _jacobi_rotate(a, u, 0, 2, 1)
        _jacobi_rotate(a, u, 1, 2, 0)
    lmax = a[0][0]
    lmax = a[1][1] if a[1][1] > lmax else lmax
    lmax = a[2][2] if a[2][2] > lmax else lmax
    floor_l = rank_tol * lmax
    x = list(m)
    for i in range(3):
        l = a[i][i]
        if l > floor_l:
            coef = _div((u[0][i] * r[0] + u[1][i] * r[1]) + u[2][i] * r[2], l)
            for c in range(3):
                x[c] = x[c] + u[c][i] * coef
    return x


def _corners(tri, V):
    """Per vertex its corners (t, slot) in ascending corner id: the table of tdgp_mesh_corner_table on triangles that are all valid."""
    corners = [[] for _ in range(V)]
    for t, idx in enumerate(tri):
        for i in range(3):
            corners[idx[i]].append((t, i))
    return corners


def quadrics(pos, tri, corners):
    V = len(pos)
    Q, W = [[0.0] * 10 for _ in range(V)], [0.0] * V
    for v in range(V):
        q10, w = Q[v], 0.0
        for t, _ in corners[v]:
            p0, p1, p2 = (pos[i] for i in tri[t])
            n = _cross(p0, p1, p2)
            s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            l = math.sqrt(s) if s >= 0.0 else float('nan')
            if not (l > 0.0 and l < INF):
                continue
            q = [n[0] / l, n[1] / l, n[2] / l, 0.0]
            q[3] = -((q[0] * p0[0] + q[1] * p0[1]) + q[2] * p0[2])
            g = l * 0.5
            o = 0
            for r in range(4):
                for c in range(r, 4):
                    q10[o] = q10[o] + (g * q[r]) * q[c]
                    o += 1
            w = w + g
        W[v] = w
    return Q, W


def _no_flip(pos, tri, corners, v, other, x):
    for t, slot in corners[v]:
        idx = tri[t]
        if other in idx:
            continue
        p = [pos[i] for i in idx]
        q = list(p)
        q[slot] = x
        n0, n1 = _cross(*p), _cross(*q)
        if not ((n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2] > 0.0):
            return False
    return True


def evaluate(a, b, st, max_error, rank_tol):
    """The verdict on the edge a < b -> None or (cost, x, c, d)."""
    pos, tri, corners, N, rim, opp = st['pos'], st['tri'], st['corners'], st['N'], st['rim'], st['opp']
    rim_a, rim_b = bool(rim[a]), bool(rim[b])
    if rim_a and rim_b:
        return None
    third = opp[(a, b)]
    if len(third) != 2 or third[0] == third[1]:
        return None
    c, d = third
    if len(corners[c]) <= 3 or len(corners[d]) <= 3:
        return None
    if (N[a] - {a, b, c, d}) & N[b]:
        return None
    Qa, Qb = st['Q'][a], st['Q'][b]
    Q = [Qa[i] + Qb[i] for i in range(10)]
    w = st['W'][a] + st['W'][b]
    pa, pb = pos[a], pos[b]
    A = [[Q[0], Q[1], Q[2]], [Q[1], Q[4], Q[5]], [Q[2], Q[5], Q[7]]]
    bv = [Q[3], Q[6], Q[8]]
    if rim_a or rim_b:
        x = list(pa if rim_a else pb)
    else:
        mid = [(pa[i] + pb[i]) * 0.5 for i in range(3)]
        x = minimise(A, bv, mid, rank_tol)
        if not all(math.isfinite(xc) for xc in x):
            x = mid
    Ax = [(A[i][0] * x[0] + A[i][1] * x[1]) + A[i][2] * x[2] for i in range(3)]
    xAx = (x[0] * Ax[0] + x[1] * Ax[1]) + x[2] * Ax[2]
    bx = (bv[0] * x[0] + bv[1] * x[1]) + bv[2] * x[2]
    cost = (xAx + 2.0 * bx) + Q[9]
    if cost != cost:
        return None
    cost = cost if cost > 0.0 else 0.0
    if max_error > 0.0 and not (cost <= (max_error * max_error) * w):
        return None
    if not _no_flip(pos, tri, corners, a, b, x) or not _no_flip(pos, tri, corners, b, a, x):
        return None
    return cost, x, c, d


def cost_bits(cost):
    with np.errstate(all='ignore'):
        return int(np.array([cost], D).astype(F).view(np.uint32)[0])


def clean_triangles(triangles, V):
    """In front of round 0: a triangle with an index outside [0, V) or a repeated index is dropped -> (list of tuples, list of input ids)."""
    tri, tmap = [], []
    for t, idx in enumerate(np.asarray(triangles, np.int64).reshape(-1, 3)):
        a, b, c = (int(i) for i in idx)
        if min(a, b, c) < 0 or max(a, b, c) >= V or a == b or b == c or a == c:
            continue
        tri.append((a, b, c))
        tmap.append(t)
    return tri, tmap


def round_tables(st):
    """corners, N and, per directed pair (a, w), the third vertices of a's triangles that name w, in a's table order."""
    tri, V = st['tri'], len(st['pos'])
    st['corners'] = corners = _corners(tri, V)
    N, opp = [set() for _ in range(V)], collections.defaultdict(list)
    for a in range(V):
        for t, slot in corners[a]:
            idx = tri[t]
            nx, pv = idx[(slot + 1) % 3], idx[(slot + 2) % 3]
            N[a].add(nx)
            N[a].add(pv)
            opp[(a, nx)].append(pv)
            opp[(a, pv)].append(nx)
    st['N'], st['opp'] = N, opp


def decimate(vertices, triangles, target_triangles=None, max_error=None, max_rounds=256, rank_tol=1e-3, fix_boundary=True, attributes=(), cache=True,
             trace=None):
    """-> Decimated, numpy arrays.  trace: a list that receives, per round, dict(selected=[(k, a, b, c, d, key)...] after the trim, all=[...]
    before it, N=the neighbour sets of the round, T=the triangle count in front of it)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    V = len(v)
    attrs = [np.asarray(a, F) for a in attributes]
    channels = [a.shape[1] for a in attrs]
    attr = [[float(x) for a in attrs for x in a[i]] for i in range(V)]
    pos = [[float(x) for x in p] for p in v]
    tri, tmap = clean_triangles(triangles, V)
    max_error = 0.0 if max_error is None else float(max_error)
    rank_tol = float(rank_tol)
    st = dict(pos=pos, tri=tri)
    round_tables(st)
    rim = [0] * V
    if fix_boundary and tri and V:
        table = SR.corner_table(np.array(tri, np.int32).reshape(-1, 3), V)
        rim = [int(r) for r in SR.boundary_vertices(np.array(tri, np.int32).reshape(-1, 3), V, table[0], table[1])]
    st['rim'] = rim
    st['Q'], st['W'] = quadrics(pos, tri, st['corners'])
    parent = list(range(V))
    memo, stale, fresh = {}, None, True
    rounds = 0
    while True:
        T = len(tri)
        if target_triangles is not None and T <= target_triangles:
            stopped = 'target'
            break
        if rounds >= max_rounds:
            stopped = 'max_rounds'
            break
        if T == 0 or V == 0:
            stopped = 'exhausted'
            break
        if not fresh:
            round_tables(st)
        fresh = False
        N = st['N']
        if stale is not None:                                      # every vertex whose neighbourhood holds a vertex the last round changed
            stale = stale | {u for s in stale for u in N[s]}
        keys, verdicts, new_memo = {}, {}, {}
        for t, idx in enumerate(tri):
            for i in range(3):
                a, b = idx[i], idx[(i + 1) % 3]
                if not a < b:
                    continue
                if cache and stale is not None and (a, b) in memo and a not in stale and b not in stale:
                    res = memo[(a, b)]
                else:
                    res = evaluate(a, b, st, max_error, rank_tol)
                new_memo[(a, b)] = res
                if res is not None:
                    k = 3 * t + i
                    keys[k] = (cost_bits(res[0]) << 32) | mix(k)
                    verdicts[k] = (a, b) + tuple(res)
        memo = new_memo
        best = {}
        for k, key in keys.items():
            a, b = verdicts[k][:2]
            for u in {a, b} | N[a] | N[b]:
                if key < best.get(u, NONE):
                    best[u] = key
        chosen = [k for k in sorted(keys) if all(best[u] == keys[k] for u in (verdicts[k][0], verdicts[k][1], verdicts[k][4], verdicts[k][5]))]
        rounds += 1
        everything = list(chosen)
        if not chosen:
            stopped = 'exhausted'
            if trace is not None:
                trace.append(dict(selected=[], all=[], N=N, T=T))
            break
        if target_triangles is not None and len(chosen) > max_collapses(T, target_triangles):
            chosen = sorted(chosen, key=lambda k: keys[k])[:max_collapses(T, target_triangles)]
        if trace is not None:
            rec = lambda ks: [(k, verdicts[k][0], verdicts[k][1], verdicts[k][4], verdicts[k][5], keys[k]) for k in ks]      # noqa: E731
            trace.append(dict(selected=rec(chosen), all=rec(everything), N=N, T=T))
        changed = set()
        for k in chosen:
            a, b, _, x, _, _ = verdicts[k]
            keep_b = (not rim[a]) and bool(rim[b])
            s, r = (b, a) if keep_b else (a, b)
            pa, pb = pos[a], pos[b]
            if attr and attr[0]:
                d = [pb[i] - pa[i] for i in range(3)]
                num = ((x[0] - pa[0]) * d[0] + (x[1] - pa[1]) * d[1]) + (x[2] - pa[2]) * d[2]
                den = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                tt = _div(num, den)
                tt = tt if tt > 0.0 else 0.0
                tt = 1.0 if tt > 1.0 else tt
                u = 1.0 - tt
                attr[s] = [u * va + tt * vb for va, vb in zip(attr[a], attr[b])]
            st['Q'][s] = [st['Q'][a][i] + st['Q'][b][i] for i in range(10)]
            st['W'][s] = st['W'][a] + st['W'][b]
            pos[s] = list(x)
            parent[r] = s
            changed |= {a, b} | N[a] | N[b]
        stale = changed
        kept = [(t, tuple(parent[i] for i in idx)) for t, idx in enumerate(tri)]
        kept = [(t, idx) for t, idx in kept if idx[0] != idx[1] and idx[1] != idx[2] and idx[0] != idx[2]]
        tmap = [tmap[t] for t, _ in kept]
        st['tri'] = tri = [idx for _, idx in kept]
    alive = [u for u in range(V) if parent[u] == u]
    index = {u: j for j, u in enumerate(alive)}
    vmap = np.full(V, -1, np.int32)
    for u in range(V):
        r = u
        while parent[r] != r:
            r = parent[r]
        vmap[u] = index[r]
    out_v = np.array([pos[u] for u in alive], D).reshape(-1, 3).astype(F)
    out_a, at = [], 0
    flat = np.array([attr[u] for u in alive], D).reshape(len(alive), sum(channels)).astype(F)
    for c in channels:
        out_a.append(np.ascontiguousarray(flat[:, at:at + c]))
        at += c
    out_t = np.array([[vmap[i] for i in idx] for idx in tri], np.int32).reshape(-1, 3)
    return Decimated(out_v, out_t, tuple(out_a), vmap, np.array(tmap, np.int32).reshape(-1), rounds, stopped)


# ---- meshes and measures -----------------------------------------------------------------------------------------------------------------
def band(V, rows=4):
    """A lattice of `rows` rows and V // rows columns with a gentle relief, every cell two triangles, plus V % rows vertices that no
    triangle names -> (vertices fp32 [V,3], triangles int32): open, two inner rows free to collapse, any V."""
    n = V // rows
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(rows), indexing='ij'), -1).reshape(-1, 2)
    z = 0.25 * np.sin(0.7 * ij[:, 0]) * np.cos(1.3 * ij[:, 1])
    v = np.concatenate([ij.astype(D), z[:, None]], 1)
    v = np.concatenate([v, np.full((V - n * rows, 3), -3.0)])
    tris = []
    for i in range(n - 1):
        for j in range(rows - 1):
            a, b, c, d = i * rows + j, (i + 1) * rows + j, (i + 1) * rows + j + 1, i * rows + j + 1
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return v.astype(F), np.array(tris, np.int32).reshape(-1, 3)


def soup():
    """A closed octahedron-like fan whose one edge a third triangle also uses, then indices out of range, degenerate triangles and duplicates,
    on top of random triples -> (vertices fp32 [48,3], triangles int32, the non-manifold edge)."""
    rs = np.random.RandomState(5)
    v = (rs.randn(48, 3) * 2).astype(F)
    t = CR.soup(40, 50, 7)
    ring = [(40, 42 + i, 42 + (i + 1) % 5) for i in range(5)] + [(41, 42 + (i + 1) % 5, 42 + i) for i in range(5)]      # a bipyramid on vertices 40 .. 46
    extra = [(42, 43, 47), (0, 1, 48), (3, -1, 5), (2 ** 31 - 1, 0, 1), (7, 7, 9), (11, 11, 11), (4, 9, 4), tuple(t[5]), tuple(t[5][[1, 2, 0]]), tuple(t[5][::-1])]
    v[40], v[41] = (0, 0, 1.5), (0, 0, -1.5)
    ang = 2 * np.pi * np.arange(5) / 5
    v[42:47] = np.stack([np.cos(ang), np.sin(ang), np.zeros(5)], 1)
    v[47] = (2.5, 1.0, 0.0)
    return v, np.concatenate([t[:25], np.array(ring + extra, np.int32), t[25:]]).astype(np.int32), (42, 43)


def directed_edges_matched(tris):
    """Every directed edge occurs once and so does its reverse: a closed, consistently oriented surface."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = [(int(a), int(b)) for a, b in np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])]
    s = set(e)
    return len(s) == len(e) and all((b, a) in s for a, b in e)


def euler(vertices_used, tris):
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
    return int(vertices_used) - len(e) + len(t)


def signed_volume(vertices, tris):
    p = np.asarray(vertices, D)[np.asarray(tris, np.int64).reshape(-1, 3)]
    return float((np.cross(p[:, 0], p[:, 1]) * p[:, 2]).sum() / 6.0)

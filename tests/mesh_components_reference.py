"""Test-side mesh components: a numpy union-find giving min-index labels, float64 per-component measurements by the formulas of include/tdgp.h,
the order-preserving compaction, and the meshes both test files use."""
import numpy as np


def labels(tris, V):
    """label[v] = the smallest vertex index of v's component.  Two vertices are connected when a triangle names both."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    parent = np.arange(V, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in tris:
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)              # the root of a set stays its minimum
    return np.array([find(v) for v in range(V)], dtype=np.int32)


def component_ids(label):
    """Dense ids 0 .. K-1 ordered by the components' smallest vertices -> (component int32 [V], K)."""
    label = np.asarray(label, np.int64)
    roots = np.flatnonzero(label == np.arange(len(label)))
    rank = np.full(len(label), -1, np.int64)
    rank[roots] = np.arange(len(roots))
    return rank[label].astype(np.int32), len(roots)


def triangle_terms(verts, tris):
    """(area, volume) term of every triangle in float64 from the fp32 vertices: 0.5 * |cross(b - a, c - a)| and dot(a, cross(b, c)) / 6."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = np.cross(b - a, c - a)
    return 0.5 * np.sqrt((n * n).sum(1)), (a * np.cross(b, c)).sum(1) / 6.0


def stats(verts, tris, component, K):
    """dict(triangles int64 [K], vertices int64 [K], area, volume float64 [K], abs_area, abs_volume (the sums of |term|, for error bounds),
    bbox_min, bbox_max fp32 [K,3]).  A triangle belongs to the component of its first vertex."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    component = np.asarray(component, np.int64)
    key = component[tris[:, 0]] if len(tris) else np.zeros(0, np.int64)
    at, vt = triangle_terms(verts, tris)
    out = dict(triangles=np.bincount(key, minlength=K).astype(np.int64), vertices=np.bincount(component, minlength=K).astype(np.int64))
    for name, term in (('area', at), ('volume', vt)):
        out[name] = np.array([term[key == k].sum() for k in range(K)], np.float64)
        out['abs_' + name] = np.array([np.abs(term[key == k]).sum() for k in range(K)], np.float64)
    out['bbox_min'] = np.stack([verts[component == k].min(0) for k in range(K)]).astype(np.float32) if K else np.zeros((0, 3), np.float32)
    out['bbox_max'] = np.stack([verts[component == k].max(0) for k in range(K)]).astype(np.float32) if K else np.zeros((0, 3), np.float32)
    return out


def compact(verts, tris, component, keep, attributes=()):
    """-> (vertices', triangles' int32, [attributes'], vertex_map int32): kept vertices and triangles in their original order, re-indexed."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    keep = np.asarray(keep).astype(bool)
    kv = keep[np.asarray(component, np.int64)] if len(verts) else np.zeros(0, bool)
    vmap = np.where(kv, np.cumsum(kv) - 1, -1).astype(np.int32)
    kt = kv[tris[:, 0]] if len(tris) else np.zeros(0, bool)
    return verts[kv], vmap[tris[kt]].astype(np.int32).reshape(-1, 3), [np.asarray(a, np.float32)[kv] for a in attributes], vmap


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def strip(T, V=None, numbering=None):
    """A triangle strip: triangle i names positions (i, i + 1, i + 2) of a line of T + 2 vertices, then `numbering` (a permutation of the
    vertex ids; None: identity) is applied.  V > T + 2 appends unreferenced vertices.  One component (plus the singletons)."""
    n = T + 2
    V = n if V is None else V
    assert V >= n
    t = np.arange(T)[:, None] + np.arange(3)[None, :]
    if numbering is not None:
        t = np.asarray(numbering)[t]
    return t.astype(np.int32).reshape(-1, 3), V


def soup(V, T, seed):
    return np.random.RandomState(seed).randint(0, V, size=(T, 3)).astype(np.int32)


CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)          # vertex 4 x + 2 y + z
# outward winding (counter-clockwise seen from outside): signed volume +1
CUBE_T = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)


def speck_volume(n=24):
    """[n, n, n] fp32: two spheres of different radius (distance fields, level 0) and three single-voxel specks: five closed components."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1)
    ball = lambda c, r: r - np.sqrt(((g - np.array(c)) ** 2).sum(-1))                      # noqa: E731
    vol = np.maximum(ball((7.2, 7.9, 8.1), 5.3), ball((17.1, 16.2, 15.8), 3.4))
    for p in ((2, 20, 3), (20, 3, 4), (3, 3, 20)):
        vol[p] = 0.7
    return vol.astype(np.float32)


def edges_used_twice(tris):
    """Every undirected edge of the triangles is used exactly twice (a closed surface)."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all())

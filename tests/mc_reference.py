"""Test-side marching cubes: a plain per-cell numpy loop driven by the same case table as the HIP kernels (tools/gen_mc_table.py), and the
mesh checks both geometry test files use.  Global id of a grid edge: 3 * (index of its lower grid point) + axis; the documented vertex
order of `geometry.marching_cubes` is ascending in that id."""
import numpy as np


def inside(vol, thresh):
    return np.asarray(vol, np.float32) >= np.float32(thresh)


def crossing_edge_ids(vol, thresh):
    """Sorted global ids of the sign-changing edges of the volume."""
    D, H, W = vol.shape
    s = inside(vol, thresh)
    idx = np.arange(D * H * W, dtype=np.int64).reshape(D, H, W)
    ids = [3 * idx[:-1][s[1:] != s[:-1]] + 0, 3 * idx[:, :-1][s[:, 1:] != s[:, :-1]] + 1, 3 * idx[:, :, :-1][s[:, :, 1:] != s[:, :, :-1]] + 2]
    return np.sort(np.concatenate([i.ravel() for i in ids]))


def count_crossing_edges(vol, thresh):
    s = inside(vol, thresh)
    return int((s[1:] != s[:-1]).sum() + (s[:, 1:] != s[:, :-1]).sum() + (s[:, :, 1:] != s[:, :, :-1]).sum())


def edge_vertices(vol, thresh, ids):
    """fp32 position of the vertex on each edge of `ids`: p0 + (thresh - v0) / (v1 - v0) along the edge's axis."""
    vol = np.asarray(vol, np.float32)
    D, H, W = vol.shape
    pt, axis = ids // 3, ids % 3
    p = np.stack(np.unravel_index(pt, (D, H, W)), 1)
    q = p.copy()
    q[np.arange(len(ids)), axis] += 1
    v0, v1 = vol[p[:, 0], p[:, 1], p[:, 2]], vol[q[:, 0], q[:, 1], q[:, 2]]
    t = (np.float32(thresh) - v0) / (v1 - v0)
    out = p.astype(np.float32)
    out[np.arange(len(ids)), axis] += t
    return out


def marcher(vol, thresh, table, edge_info):
    """-> triangles [T,3] of global edge ids, cell by cell (ascending cell index), table order inside a cell."""
    D, H, W = vol.shape
    s = inside(vol, thresh)
    info = [edge_info(e) for e in range(12)]
    tris = []
    for d in range(D - 1):
        for h in range(H - 1):
            for w in range(W - 1):
                case = 0
                for k in range(8):
                    if s[d + ((k >> 2) & 1), h + ((k >> 1) & 1), w + (k & 1)]:
                        case |= 1 << k
                for t in table[case]:
                    tri = []
                    for e in t:
                        axis, (dd, dh, dw) = info[e]
                        tri.append(3 * (((d + dd) * H + (h + dh)) * W + (w + dw)) + axis)
                    tris.append(tri)
    return np.array(tris, dtype=np.int64).reshape(-1, 3)


def canonical(tris):
    """Each triangle rotated so that its smallest entry comes first (winding kept), rows sorted."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    if not len(tris):
        return tris
    k = tris.argmin(1)
    rot = np.stack([tris[np.arange(len(tris)), (k + i) % 3] for i in range(3)], 1)
    return rot[np.lexsort((rot[:, 2], rot[:, 1], rot[:, 0]))]


def assert_closed_oriented(tris):
    """Every mesh edge is shared by exactly two triangles that run through it in opposite directions.  -> number of (undirected) edges."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    assert (tris[:, 0] != tris[:, 1]).all() and (tris[:, 1] != tris[:, 2]).all() and (tris[:, 0] != tris[:, 2]).all(), 'degenerate triangle'
    a = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]])
    b = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 0]])
    n = int(max(a.max(), b.max())) + 1
    fwd, bwd = a * n + b, b * n + a
    uf, cf = np.unique(fwd, return_counts=True)
    assert (cf == 1).all(), f'{int((cf > 1).sum())} directed edges used more than once'
    assert np.array_equal(uf, np.unique(bwd)), 'an edge lacks its opposite: open or inconsistently oriented mesh'
    return len(uf) // 2


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    return float(np.einsum('ij,ij->i', v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def smooth_noise(shape, seed, passes=2):
    """Seeded uniform noise, lightly smoothed (box filter over the 6-neighbourhood), range roughly [0, 1]."""
    v = np.random.RandomState(seed).rand(*shape)
    for _ in range(passes):
        v = (v + sum(np.roll(v, s, a) for a in range(3) for s in (-1, 1))) / 7.0
    return v.astype(np.float32)


def sphere(n, r):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1) - (n - 1) / 2.0 + np.array([0.13, -0.21, 0.07])
    return (r - np.sqrt((g ** 2).sum(-1))).astype(np.float32)


def torus(shape, R, r):
    D, H, W = shape
    g = np.stack(np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij'), -1)
    g = g - (np.array(shape) - 1) / 2.0 + np.array([0.11, 0.23, -0.17])
    ring = np.sqrt(g[..., 1] ** 2 + g[..., 2] ** 2) - R
    return (r - np.sqrt(ring ** 2 + g[..., 0] ** 2)).astype(np.float32)

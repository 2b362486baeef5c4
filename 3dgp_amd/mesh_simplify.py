"""Mesh simplification: vertex clustering on a uniform grid, each cluster's representative placed by its error quadric (Rossignac-Borrel
1993; Lindstrom, "Out-of-core simplification", 2000), for the indexed mesh `geometry.marching_cubes` leaves on the device (DESIGN.md 5.22;
csrc/mesh_simplify.hip, contract in include/tdgp.h).

    cl = cluster_vertices(vertices, cell)                      # Clusters(cluster [V], order [V], start [C+1], key [C]): dense ids by ascending cell
    s = simplify(vertices, triangles, cell)                    # Simplified(vertices [C,3], triangles [T',3], attributes, cluster [V], triangle_map [T'])
    cell = cell_for_triangles(vertices, triangles, 100_000)    # the first cell of the ladder cell_min * 2^(j/2) that leaves at most so many

A marching-cubes mesh is made of voxel-sized triangles; a cell of 2-4 voxels takes it to a tenth or less.  No priority queue, no
data-dependent iteration count: every output is a pure function of the arrays as given -- the same bytes on every run.  The quadric sums are
sequential in corner-table order, so they are NOT invariant under a permutation of the triangles; the clusters and the 'mean' placement are.
Clustering does not preserve topology: sheets closer than a cell merge, and the output can hold non-manifold edges and opposite-facing pairs.
The host reads back two numbers, C and T' (and the corner table's total under 'quadric').  GPU only: the kernels have no CPU path.
"""
import collections
import ctypes
import math

import torch

from . import _lib
from . import mesh_surface as _mesh_surface

Clusters = collections.namedtuple('Clusters', ['cluster', 'order', 'start', 'key'])
Simplified = collections.namedtuple('Simplified', ['vertices', 'triangles', 'attributes', 'cluster', 'triangle_map'])
PLACEMENTS = {'mean': 0, 'quadric': 1}
K_HALF = 2 ** 20                      # cell indices lie in [-2^20, 2^20); a key is ((kz + 2^20) * 2^21 + (ky + 2^20)) * 2^21 + (kx + 2^20)
ATTRIBUTE_CHANNELS_MAX = 64


def _triple(x, what, positive):
    try:
        t = tuple(float(c) for c in x) if isinstance(x, (tuple, list)) else (float(x),) * 3
    except (TypeError, ValueError):
        raise ValueError(f'{what} must be a float or three of them, got {x!r}') from None
    if len(t) != 3 or not all(math.isfinite(c) and (c > 0 or not positive) for c in t):
        raise ValueError(f'{what} must be {"positive and " if positive else ""}finite, one float or three, got {x!r}')
    return t


def _grid(cell, origin):
    """-> (cell, origin) as two ctypes double[3] (and the tuples they hold)."""
    c, o = _triple(cell, 'cell', True), _triple(origin, 'origin', False)
    return (ctypes.c_double * 3)(*c), (ctypes.c_double * 3)(*o)


def _check_vertices(vertices):
    if not isinstance(vertices, torch.Tensor):
        raise TypeError(f'vertices must be a tensor, got {type(vertices).__name__}')
    if vertices.dtype != torch.float32 or vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f'vertices must be fp32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}')
    if vertices.shape[0] > _mesh_surface.V_MAX:
        raise ValueError(f'V = {vertices.shape[0]} is more than the 2^31 - 2 vertices the kernels index')
    _lib.require_cuda(vertices, 'vertices')
    return vertices.contiguous()


def _cluster(vertices, grid):
    dev, V = vertices.device, int(vertices.shape[0])
    key = torch.empty([V], dtype=torch.int64, device=dev)
    cluster = torch.empty([V], dtype=torch.int32, device=dev)
    start = torch.empty([V + 1], dtype=torch.int32, device=dev)
    ckey = torch.empty([V], dtype=torch.int64, device=dev)
    ws, need = _lib.byte_workspace('tdgp_mesh_cluster_ids_workspace_bytes', (V,), dev, ValueError(f'cluster_vertices: V = {V} is more than the 2^31 - 2 it indexes'))
    with torch.cuda.device(dev):
        stream = _lib.stream_of(vertices)
        _lib.call('tdgp_mesh_cluster_keys', vertices.data_ptr(), V, grid[0], grid[1], key.data_ptr(), stream)
        skey, perm = torch.sort(key, stable=True)                                      # grouping is plumbing; heads, ranks and start are the kernel's
        order = perm.to(torch.int32)
        _lib.call('tdgp_mesh_cluster_ids', skey.data_ptr(), order.data_ptr(), V, cluster.data_ptr(), start.data_ptr(), ckey.data_ptr(), ws.data_ptr(), need, stream)
    C = int(ws[:8].view(torch.int64).cpu())                                            # the one number read back
    return Clusters(cluster, order, start[:C + 1], ckey[:C])


def cluster_vertices(vertices, cell, origin=(0, 0, 0)):
    """vertices fp32 [V,3] on the device -> Clusters(cluster int32 [V], order int32 [V], start int32 [C+1], key int64 [C]).
    Per vertex and axis k = floor((double(v) - origin) / cell); the vertices of one cell are one cluster, numbered by ascending cell key
    ((kz + 2^20) * 2^21 + (ky + 2^20)) * 2^21 + (kx + 2^20); cluster c's members are order[start[c]:start[c+1]], ascending vertex id.
    A vertex with a non-finite coordinate or a k outside [-2^20, 2^20) has cluster -1; those vertices are order[:start[0]]."""
    grid = _grid(cell, origin)
    return _cluster(_check_vertices(vertices), grid)


def _check_clusters(clusters, vertices):
    V = int(vertices.shape[0])
    if not (isinstance(clusters, tuple) and len(clusters) == 4):
        raise TypeError(f'clusters must be the Clusters `cluster_vertices` returns, got {type(clusters).__name__}')
    cluster, order, start, key = clusters
    for t, what, dt, n in ((cluster, 'cluster', torch.int32, V), (order, 'order', torch.int32, V), (start, 'start', torch.int32, None), (key, 'key', torch.int64, None)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.ndim != 1 or (n is not None and t.shape[0] != n):
            raise ValueError(f'clusters.{what} must be {dt} [{"C" if n is None else n}], got {getattr(t, "dtype", type(t).__name__)} {tuple(getattr(t, "shape", ()))}')
        if t.device != vertices.device:
            raise ValueError(f'clusters.{what} must be on {vertices.device}, got {t.device}')
    if start.shape[0] != key.shape[0] + 1 or key.shape[0] > V:
        raise ValueError(f'clusters.start must have one entry more than clusters.key, at most V + 1 = {V + 1}: got {start.shape[0]} and {key.shape[0]}')
    return Clusters(cluster.contiguous(), order.contiguous(), start.contiguous(), key.contiguous())


def _relabel(triangles, V, cluster):
    T = int(triangles.shape[0])
    ct = torch.empty([T, 3], dtype=torch.int32, device=triangles.device)
    rotated = torch.empty([T, 3], dtype=torch.int32, device=triangles.device)
    with torch.cuda.device(triangles.device):
        _lib.call('tdgp_mesh_cluster_triangles_relabel', triangles.data_ptr(), T, V, cluster.data_ptr(), ct.data_ptr(), rotated.data_ptr(), _lib.stream_of(triangles))
    return ct, rotated


def _count(rotated, dedup):
    """-> (keep uint8 [T], workspace, its size, T'): the survivors flagged and counted; T' is the one number read back."""
    dev, T = rotated.device, int(rotated.shape[0])
    keep = torch.empty([T], dtype=torch.uint8, device=dev)
    ws, need = _lib.byte_workspace('tdgp_mesh_cluster_triangles_workspace_bytes', (T,), dev, ValueError(f'simplify: 3 T = {3 * T} is more than the 2^31 - 1 it indexes'))
    perm = None
    if dedup and T > 0:                                                                # equal triples side by side, each group by ascending triangle: three stable sorts
        p = torch.sort(rotated[:, 2], stable=True).indices
        p = p[torch.sort(rotated[p, 1], stable=True).indices]
        perm = p[torch.sort(rotated[p, 0], stable=True).indices].to(torch.int32)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_cluster_triangles_count', rotated.data_ptr(), _lib.ptr(perm), T, keep.data_ptr(), ws.data_ptr(), need, _lib.stream_of(rotated))
    return keep, ws, need, int(ws[:8].view(torch.int64).cpu())


def _check_attributes(attributes, vertices):
    out = []
    for k, a in enumerate(tuple(attributes)):
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.ndim != 2 or a.shape[0] != vertices.shape[0] or not 1 <= a.shape[1] <= ATTRIBUTE_CHANNELS_MAX:
            raise ValueError(f'attributes[{k}] must be fp32 [{vertices.shape[0]}, 1..{ATTRIBUTE_CHANNELS_MAX}], got {getattr(a, "dtype", type(a).__name__)} '
                             f'{tuple(getattr(a, "shape", ()))}')
        _lib.require_cuda(a, f'attributes[{k}]')
        if a.device != vertices.device:
            raise ValueError(f'attributes[{k}] must be on {vertices.device}, got {a.device}')
        out.append(a.contiguous())
    return out


def simplify(vertices, triangles, cell, origin=(0, 0, 0), placement='quadric', rank_tol=1e-3, dedup=True, attributes=(), clusters=None):
    """-> Simplified(vertices fp32 [C,3], triangles int32 [T',3], attributes (fp32 [C,c], ...), cluster int32 [V], triangle_map int32 [T']).
    The vertices of every cell of side `cell` (a float or three; the lattice starts at `origin`) become one vertex.  A triangle survives when
    its three clusters exist and differ; dedup: and no triangle of lower index has the same triple up to rotation (the flip is another
    triangle and stays).  Survivors keep their order; triangle_map[j] is the input index of output triangle j.
    placement='quadric': the point that minimises the sum of squared distances to the planes of every triangle with a corner in the cluster,
    restricted to the eigen-directions whose eigenvalue exceeds rank_tol times the largest and started from the members' mean; the mean itself
    when that point leaves the cell (include/tdgp.h has the operations, in order).  Creases and corners stay where plain means round them
    off.  'mean': the members' mean.  attributes: fp32 [V,c] arrays (colours, ...), each averaged over a cluster's members.
    clusters: the Clusters of these vertices for this cell and origin, when the caller has them."""
    if placement not in PLACEMENTS:
        raise ValueError(f'placement must be one of {sorted(PLACEMENTS)}, got {placement!r}')
    rank_tol = float(rank_tol)
    if not (math.isfinite(rank_tol) and rank_tol >= 0):
        raise ValueError(f'rank_tol must be finite and not negative, got {rank_tol!r}')
    grid = _grid(cell, origin)
    vertices, triangles = _mesh_surface._check_mesh(vertices, triangles)
    attributes = _check_attributes(attributes, vertices)
    cl = _cluster(vertices, grid) if clusters is None else _check_clusters(clusters, vertices)
    V, C = int(vertices.shape[0]), int(cl.key.shape[0])
    ct, rotated = _relabel(triangles, V, cl.cluster)
    out_t, tri_map = _emit(ct, *_count(rotated, dedup))
    table = _mesh_surface._corner_table(ct, C) if placement == 'quadric' and C > 0 else None
    out_v = _place(vertices, triangles, cl, grid, table, rank_tol)
    return Simplified(out_v, out_t, tuple(_attribute(a, cl) for a in attributes), cl.cluster, tri_map)


def _emit(ct, keep, ws, need, T_out):
    """The kept triangles, re-indexed to clusters, in input order -> (triangles int32 [T',3], triangle_map int32 [T'])."""
    dev, T = ct.device, int(ct.shape[0])
    out_t = torch.empty([T_out, 3], dtype=torch.int32, device=dev)
    tri_map = torch.empty([T_out], dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_cluster_triangles_emit', ct.data_ptr(), T, keep.data_ptr(), ws.data_ptr(), need, out_t.data_ptr(), T_out, tri_map.data_ptr(), _lib.stream_of(ct))
    return out_t, tri_map


def _place(vertices, triangles, cl, grid, table, rank_tol=1e-3):
    """tdgp_mesh_cluster_place: table = the corner table of the relabelled triangles (quadric), or None (mean) -> vertices fp32 [C,3]."""
    dev, V, T, C = vertices.device, int(vertices.shape[0]), int(triangles.shape[0]), int(cl.key.shape[0])
    out_v = torch.empty([C, 3], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_cluster_place', vertices.data_ptr(), V, cl.order.data_ptr(), cl.start.data_ptr(), cl.key.data_ptr(), C, grid[0], grid[1],
                  triangles.data_ptr(), T, _lib.ptr(None if table is None else table.start), _lib.ptr(None if table is None else table.corner),
                  0 if table is None else 1, float(rank_tol), out_v.data_ptr(), _lib.stream_of(vertices))
    return out_v


def _attribute(a, cl):
    C = int(cl.key.shape[0])
    out = torch.empty([C, a.shape[1]], dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.call('tdgp_mesh_cluster_attribute', a.data_ptr(), int(a.shape[1]), int(a.shape[0]), cl.order.data_ptr(), cl.start.data_ptr(), C, out.data_ptr(), _lib.stream_of(a))
    return out


def ladder(cell_min=1.0, steps=12):
    """The cells `cell_for_triangles` tries: cell_min * 2^(j/2), j = 0 .. steps-1."""
    cell_min = float(cell_min)
    if not (math.isfinite(cell_min) and cell_min > 0):
        raise ValueError(f'cell_min must be positive and finite, got {cell_min!r}')
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError(f'steps must be a positive int, got {steps!r}')
    return [cell_min * 2.0 ** (j / 2.0) for j in range(steps)]


def count_triangles(vertices, triangles, cell, origin=(0, 0, 0), dedup=True):
    """T' of `simplify` for this cell: keys -> ids -> triangle count; nothing is placed or emitted."""
    grid = _grid(cell, origin)
    vertices, triangles = _mesh_surface._check_mesh(vertices, triangles)
    cl = _cluster(vertices, grid)
    return _count(_relabel(triangles, int(vertices.shape[0]), cl.cluster)[1], dedup)[3]


def cell_for_triangles(vertices, triangles, max_triangles, cell_min=1.0, steps=12, origin=(0, 0, 0)):
    """The first cell of the ladder cell_min * 2^(j/2), j = 0 .. steps-1, whose surviving-triangle count is <= max_triangles.  ValueError
    naming the last count if none is.  Each rung runs keys -> ids -> triangle count only."""
    if isinstance(max_triangles, bool) or not isinstance(max_triangles, int) or max_triangles < 0:
        raise ValueError(f'max_triangles must be a non-negative int, got {max_triangles!r}')
    cells = ladder(cell_min, steps)
    _grid(1.0, origin)
    count = None
    for cell in cells:
        count = count_triangles(vertices, triangles, cell, origin)
        if count <= max_triangles:
            return cell
    raise ValueError(f'cell_for_triangles: no cell of the ladder {cells[0]:g} .. {cells[-1]:g} leaves at most {max_triangles} triangles; the last leaves {count}')


def apply(vertices, triangles, options, attributes=()):
    """The `simplify=` argument of geometry.extract_geometry / mesh.render_mesh_frames: a dict of `simplify` keyword arguments with either
    `cell` or `max_triangles` (then cell_min / steps choose the ladder) -> Simplified."""
    kw = check_options(options)
    if 'max_triangles' in kw:
        ladder_kw = {k: kw.pop(k) for k in ('cell_min', 'steps') if k in kw}
        kw['cell'] = cell_for_triangles(vertices, triangles, kw.pop('max_triangles'), origin=kw.get('origin', (0, 0, 0)), **ladder_kw)
    return simplify(vertices, triangles, attributes=attributes, **kw)


def check_options(options):
    """A `simplify=` dict, checked without a device -> a copy."""
    if not isinstance(options, dict):
        raise TypeError(f'simplify must be None or a dict of mesh_simplify.simplify arguments, got {type(options).__name__}')
    kw = dict(options)
    known = {'cell', 'max_triangles', 'cell_min', 'steps', 'origin', 'placement', 'rank_tol', 'dedup'}
    if set(kw) - known:
        raise ValueError(f'simplify: unknown options {sorted(set(kw) - known)}; known: {sorted(known)}')
    if ('cell' in kw) == ('max_triangles' in kw):
        raise ValueError('simplify takes exactly one of cell and max_triangles')
    if 'cell' in kw:
        if 'cell_min' in kw or 'steps' in kw:
            raise ValueError('simplify: cell_min and steps belong to max_triangles')
        _triple(kw['cell'], 'cell', True)
    else:
        ladder(kw.get('cell_min', 1.0), kw.get('steps', 12))
        if isinstance(kw['max_triangles'], bool) or not isinstance(kw['max_triangles'], int) or kw['max_triangles'] < 0:
            raise ValueError(f'max_triangles must be a non-negative int, got {kw["max_triangles"]!r}')
    if kw.get('placement', 'quadric') not in PLACEMENTS:
        raise ValueError(f'placement must be one of {sorted(PLACEMENTS)}, got {kw["placement"]!r}')
    _triple(kw.get('origin', (0, 0, 0)), 'origin', False)
    return kw

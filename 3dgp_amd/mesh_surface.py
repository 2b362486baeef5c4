"""Mesh surfaces: vertex normals, Laplacian / Taubin smoothing and the open rim of the indexed mesh `geometry.marching_cubes` leaves on the
device (csrc/mesh_surface.hip, contract in include/tdgp.h).

All three are gathers over ONE structure, the vertex -> triangle incidence in a defined order:

    table = corner_table(triangles, V)                      # CornerTable(start [V+1], corner [start[V]], degree [V]): per vertex, its corners ascending
    n = vertex_normals(vertices, triangles, table=table)    # area- or uniformly weighted, fp64 sums in table order, unit fp32 (0 for a lone vertex)
    rim = boundary_vertices(triangles, V, table=table)      # bool [V]: on an edge that exactly one triangle uses
    v2 = smooth(vertices, triangles, iterations=10)         # Taubin lambda | mu steps of the umbrella operator; the rim is held by default

The reference's users do this on a host copy of the mesh (trimesh, MeshLab); here the mesh stays on the device between `clean_mesh` and
`grid_to_world`.  Every output is a pure function of the arrays as given -- the same bytes on every run; the fp64 sums are sequential in table
order, so they are NOT invariant under a permutation of the triangles.  A triangle naming an index outside [0, V) is skipped.  The one
host read-back is the table's total.  GPU only: the kernels have no CPU path.
"""
import collections

import torch

from . import _lib

CornerTable = collections.namedtuple('CornerTable', ['start', 'corner', 'degree'])
WEIGHTS = {'area': 0, 'uniform': 1}
T_MAX = (2 ** 31 - 1) // 3
V_MAX = 2 ** 31 - 2


def _check_triangles(triangles, num_vertices):
    if not isinstance(triangles, torch.Tensor):
        raise TypeError(f'triangles must be a tensor, got {type(triangles).__name__}')
    if triangles.dtype != torch.int32 or triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f'triangles must be int32 [T,3], got {triangles.dtype} {tuple(triangles.shape)}')
    V = int(num_vertices)
    if V < 0 or V > V_MAX or triangles.shape[0] > T_MAX:
        raise ValueError(f'num_vertices = {V} must lie in [0, 2^31 - 2] and 3 T = {3 * triangles.shape[0]} in [0, 2^31 - 1]')
    _lib.require_cuda(triangles, 'triangles')
    return triangles.contiguous()


def _check_mesh(vertices, triangles):
    if not isinstance(vertices, torch.Tensor):
        raise TypeError(f'vertices must be a tensor, got {type(vertices).__name__}')
    if vertices.dtype != torch.float32 or vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f'vertices must be fp32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}')
    triangles = _check_triangles(triangles, vertices.shape[0])
    _lib.require_cuda(vertices, 'vertices')
    if triangles.device != vertices.device:
        raise ValueError(f'vertices and triangles must share a device, got {vertices.device} and {triangles.device}')
    return vertices.contiguous(), triangles


def _check_table(table, triangles, V):
    """A caller's table: dtypes, shapes and device (its contents are the kernels' business: they clamp and skip)."""
    if not isinstance(table, CornerTable) and not (isinstance(table, tuple) and len(table) == 3):
        raise TypeError(f'table must be the CornerTable `corner_table` returns, got {type(table).__name__}')
    start, corner = table[0], table[1]
    for t, what, n in ((start, 'start', V + 1), (corner, 'corner', None)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.ndim != 1 or (n is not None and t.shape[0] != n):
            raise ValueError(f'table.{what} must be int32 [{"start[V]" if n is None else n}], got {getattr(t, "dtype", type(t).__name__)} {tuple(getattr(t, "shape", ()))}')
        if t.device != triangles.device:
            raise ValueError(f'table.{what} must be on {triangles.device}, got {t.device}')
    if corner.shape[0] > 3 * triangles.shape[0]:
        raise ValueError(f'table.corner has {corner.shape[0]} entries, more than the 3 T = {3 * triangles.shape[0]} corners of the mesh')
    return CornerTable(start.contiguous(), corner.contiguous(), table[2])


def _corner_table(triangles, V):
    dev, T = triangles.device, int(triangles.shape[0])
    degree = torch.empty([V], dtype=torch.int32, device=dev)
    start = torch.empty([V + 1], dtype=torch.int32, device=dev)
    corner = torch.empty([3 * T], dtype=torch.int32, device=dev)
    ws, need = _lib.byte_workspace('tdgp_mesh_corner_table_workspace_bytes', (T, V), dev, ValueError(f'corner_table: T = {T}, V = {V} are more than it indexes'))
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_corner_table', triangles.data_ptr(), T, V, degree.data_ptr(), start.data_ptr(), corner.data_ptr(), ws.data_ptr(), need,
                  _lib.stream_of(triangles))
    total = int(ws[:8].view(torch.int64).cpu())                                        # the one number read back
    return CornerTable(start, corner[:total], degree)


def corner_table(triangles, num_vertices):
    """triangles int32 [T,3] on the device -> CornerTable(start int32 [V+1], corner int32 [start[V]], degree int32 [V]).  Corner 3t + i is slot i
    of triangle t; vertex v's corners are corner[start[v]:start[v+1]], in ascending corner id; degree[v] is their number.  A triangle with
    an index outside [0, V) contributes no corner.  A pure function of `triangles`."""
    return _corner_table(_check_triangles(triangles, num_vertices), int(num_vertices))


def _table_of(table, triangles, V):
    return _corner_table(triangles, V) if table is None else _check_table(table, triangles, V)


def vertex_normals(vertices, triangles, weight='area', table=None):
    """Unit vertex normals [V,3] fp32: the sum over the vertex's corners, in table order and in double, of the triangles' cross products
    ('area': each counts by its area) or of their unit normals ('uniform'), normalised; 0 for a vertex no triangle names or whose sum vanishes.
    They follow the stored winding (marching cubes: toward lower density)."""
    if weight not in WEIGHTS:
        raise ValueError(f'weight must be one of {sorted(WEIGHTS)}, got {weight!r}')
    vertices, triangles = _check_mesh(vertices, triangles)
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    table = _table_of(table, triangles, V)
    out = torch.empty([V, 3], dtype=torch.float32, device=vertices.device)
    with torch.cuda.device(vertices.device):
        _lib.call('tdgp_mesh_vertex_normals', vertices.data_ptr(), triangles.data_ptr(), T, V, table.start.data_ptr(), table.corner.data_ptr(), WEIGHTS[weight],
                  out.data_ptr(), _lib.stream_of(vertices))
    return out


def _boundary(triangles, V, table):
    rim = torch.empty([V], dtype=torch.uint8, device=triangles.device)
    with torch.cuda.device(triangles.device):
        _lib.call('tdgp_mesh_boundary_vertices', triangles.data_ptr(), int(triangles.shape[0]), V, table.start.data_ptr(), table.corner.data_ptr(), rim.data_ptr(),
                  _lib.stream_of(triangles))
    return rim


def boundary_vertices(triangles, num_vertices, table=None):
    """bool [V]: the vertices on an edge that exactly one triangle uses -- the open rims a crop or the grid boundary cuts into a level set."""
    triangles = _check_triangles(triangles, num_vertices)
    V = int(num_vertices)
    return _boundary(triangles, V, _table_of(table, triangles, V)).bool()


def smooth(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, pinned=None, table=None):
    """Taubin smoothing -> new vertices [V,3] fp32 (the input is not written).  One iteration is a step of factor `lam` (shrinks) then one of
    factor `mu` (inflates: Taubin's lambda | mu, which keeps the volume a plain Laplacian loses); mu=None: `lam` steps only.  A step moves every
    free vertex by factor * (mean of its corners' two neighbours - itself), in double, rounded once.  fix_boundary: the rim (`boundary_vertices`)
    does not move; pinned: bool / uint8 [V] of further vertices that do not.  iterations=0 returns the input's bytes.  The table is built once
    and every step reads it; steps ping-pong between two buffers."""
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
        raise ValueError(f'iterations must be a non-negative int, got {iterations!r}')
    factors = [float(lam)] if mu is None else [float(lam), float(mu)]
    if not all(f == f and abs(f) != float('inf') for f in factors):
        raise ValueError(f'lam and mu must be finite, got {lam!r}, {mu!r}')
    vertices, triangles = _check_mesh(vertices, triangles)
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    if pinned is not None:
        if not isinstance(pinned, torch.Tensor) or pinned.dtype not in (torch.bool, torch.uint8) or tuple(pinned.shape) != (V,):
            raise ValueError(f'pinned must be bool [{V}], got {getattr(pinned, "dtype", type(pinned).__name__)} {tuple(getattr(pinned, "shape", ()))}')
        _lib.require_cuda(pinned, 'pinned')
        pinned = pinned.to(torch.uint8).contiguous()
    if table is not None:
        table = _check_table(table, triangles, V)
    if iterations == 0 or V == 0:
        return vertices.clone()
    table = _corner_table(triangles, V) if table is None else table
    if fix_boundary:
        rim = _boundary(triangles, V, table)
        pinned = rim if pinned is None else pinned | rim
    steps = factors * iterations
    bufs = [torch.empty_like(vertices) for _ in range(min(2, len(steps)))]             # the caller's tensor is never a destination
    src = vertices
    with torch.cuda.device(vertices.device):
        stream = _lib.stream_of(vertices)
        for k, f in enumerate(steps):
            dst = bufs[k % 2]
            _lib.call('tdgp_mesh_smooth_step', src.data_ptr(), triangles.data_ptr(), T, V, table.start.data_ptr(), table.corner.data_ptr(), f, _lib.ptr(pinned),
                      dst.data_ptr(), stream)
            src = dst
    return src


def interp_normals(tri, status, t_hit, ray_o, ray_d, vertices, triangles, vertex_normal, normal):
    """tdgp_mesh_interp_normals: the face normals `mesh.mesh_resolve` wrote into `normal` [rays,3] are replaced IN PLACE, on the rays that hit,
    by the barycentric interpolation of `vertex_normal` [V,3] at the hit, normalised.  -> normal."""
    vertices, triangles = _check_mesh(vertices, triangles)
    rays = int(status.numel())
    if not isinstance(vertex_normal, torch.Tensor) or vertex_normal.dtype != torch.float32 or tuple(vertex_normal.shape) != tuple(vertices.shape):
        raise ValueError(f'vertex_normals must be fp32 {tuple(vertices.shape)}, got {getattr(vertex_normal, "dtype", type(vertex_normal).__name__)} '
                         f'{tuple(getattr(vertex_normal, "shape", ()))}')
    for t, what, dt, n in ((tri, 'tri', torch.int32, rays), (status, 'status', torch.int32, rays), (t_hit, 't_hit', torch.float32, rays),
                           (ray_o, 'ray_o', torch.float32, rays * 3), (ray_d, 'ray_d', torch.float32, rays * 3), (normal, 'normal', torch.float32, rays * 3)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError(f'interp_normals: {what} must be contiguous {dt} with {n} elements, got {t.dtype} {tuple(t.shape)}')
        _lib.require_cuda(t, what)
    _lib.require_cuda(vertex_normal, 'vertex_normals')
    vertex_normal = vertex_normal.contiguous()
    with torch.cuda.device(vertices.device):
        _lib.call('tdgp_mesh_interp_normals', tri.data_ptr(), status.data_ptr(), t_hit.data_ptr(), ray_o.data_ptr(), ray_d.data_ptr(), rays, vertices.data_ptr(),
                  vertices.shape[0], triangles.data_ptr(), triangles.shape[0], vertex_normal.data_ptr(), normal.data_ptr(), _lib.stream_of(vertices))
    return normal

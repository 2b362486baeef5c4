"""Mesh rays: what a ray hits on a mesh, on the device (csrc/mesh_rays.hip, contract in include/tdgp.h).

    grid = mesh_distance.build_grid(vertices, triangles)       # the triangle grid of mesh_distance, as it is
    h = first_hits(origins, directions, grid)                  # Hits(t float64 [N], depth fp32 [N], triangle int32 [N], bary fp32 [N,2], side int8 [N])
    blocked = occluded(origins, directions, grid, t_max=5.0)   # uint8 [N]: any hit inside the window
    seen = segment_visible(p, q, grid)                         # uint8 [N]: nothing between p and q
    ao = vertex_occlusion(vertices, triangles, rays=32)        # fp32 [V] in [0, 1]: 1 = open sky, fits save_ply(colours=) / render_mesh_views(vertex_occlusion=)

The ray-triangle function is one pure function in double (the watertight translate / shear / scale form: no ray passes between two triangles
that share an edge), and the hit is the accepted triangle with the smallest t, ties to the smallest triangle index -- so the walk through
the grid returns the bits of the scan over all triangles (`brute_force=True`, the yardstick), and every array is the same bytes on every
run.  Ambient occlusion casts R cosine-weighted directions per point in any-hit mode and counts the unoccluded ones: an integer over R.
Not differentiable.  GPU only: a CPU tensor is refused with a ValueError before any launch."""
import collections
import math

import numpy as np
import torch

from . import _lib
from .mesh_distance import PAIRS_MAX, TriangleGrid, _c_grid, _check_grid, _check_mesh, build_grid

Hits = collections.namedtuple('Hits', ['t', 'depth', 'triangle', 'bary', 'side'])
RAYS = (16, 32, 64)
ROTATIONS_MAX = 64
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def _check_rays(x, name, device):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f'{name} must be a tensor, got {type(x).__name__}')
    if x.dtype != torch.float32 or x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f'{name} must be fp32 [N,3], got {x.dtype} {tuple(x.shape)}')
    if not x.is_cuda or x.device != device:
        raise ValueError(f'{name} must reside on the GPU of the grid (got {x.device}); mesh_rays has no CPU path')
    if x.shape[0] > PAIRS_MAX:
        raise ValueError('N must not exceed 2^31 - 1')
    return x.contiguous()


def _check_pair(a, b, names, grid):
    grid = _check_grid(grid)
    a = _check_rays(a, names[0], grid.vertices.device)
    b = _check_rays(b, names[1], grid.vertices.device)
    if a.shape != b.shape:
        raise ValueError(f'{names[0]} and {names[1]} must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}')
    return a, b, grid


def _check_number(x, name):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.floating, np.integer)):
        raise TypeError(f'{name} must be a float, got {type(x).__name__}')
    return float(x)


def _check_window(t_min, t_max):
    t_min, t_max = _check_number(t_min, 't_min'), _check_number(t_max, 't_max')
    if not math.isfinite(t_min) or math.isnan(t_max) or not t_min <= t_max:
        raise ValueError(f'need a finite t_min <= t_max (t_max may be inf), got {t_min!r} and {t_max!r}')
    return t_min, t_max


def _check_count(rays):
    if isinstance(rays, bool) or not isinstance(rays, (int, np.integer)) or int(rays) not in RAYS:
        raise ValueError(f'rays must be one of {RAYS}, got {rays!r}')
    return int(rays)


def _check_rotations(rotations):
    if isinstance(rotations, bool) or not isinstance(rotations, (int, np.integer)) or not 1 <= int(rotations) <= ROTATIONS_MAX or int(rotations) & (int(rotations) - 1):
        raise ValueError(f'rotations must be a power of two in [1, {ROTATIONS_MAX}], got {rotations!r}')
    return int(rotations)


def _fp32(x, name, low_open):
    """A bias (>= 0, finite) or a radius (> 0, inf allowed) -> the fp32 number as a Python float."""
    x = _check_number(x, name)
    with np.errstate(over='ignore'):
        f = float(np.float32(x)) if not math.isnan(x) else x
    if math.isnan(f) or (f <= 0 if low_open else (f < 0 or math.isinf(f))):
        raise ValueError(f'{name} must be ' + ('greater than 0' if low_open else 'finite and not negative') + f' in fp32, got {x!r}')
    return f


def _cast(origins, directions, grid, t_min, t_max, brute_force, any_hit, return_evaluated):
    dev, N = origins.device, int(origins.shape[0])
    evaluated = torch.empty([N], dtype=torch.int32, device=dev) if return_evaluated else None
    if any_hit:
        hit = torch.empty([N], dtype=torch.uint8, device=dev)
        outs = [None] * 5
    else:
        hit = None
        outs = [torch.empty([N], dtype=torch.float64, device=dev), torch.empty([N], dtype=torch.float32, device=dev), torch.empty([N], dtype=torch.int32, device=dev),
                torch.empty([N, 2], dtype=torch.float32, device=dev), torch.empty([N], dtype=torch.int8, device=dev)]
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_rays_cast', origins.data_ptr(), directions.data_ptr(), N, t_min, t_max, grid.vertices.data_ptr(), grid.triangles.data_ptr(),
                  int(grid.triangles.shape[0]), int(grid.vertices.shape[0]), grid.valid.data_ptr(), c_lo, grid.cell, c_dims, grid.cell_start.data_ptr(),
                  grid.pair_triangle.data_ptr(), int(grid.pair_triangle.shape[0]), int(brute_force), int(any_hit), *[_lib.ptr(x) for x in outs], _lib.ptr(hit),
                  _lib.ptr(evaluated), _lib.stream_of(origins))
    return (hit if any_hit else Hits(*outs)), evaluated


def first_hits(origins, directions, grid, t_min=0.0, t_max=math.inf, brute_force=False, *, return_evaluated=False):
    """-> Hits(t float64 [N], depth fp32 [N] = t rounded once, triangle int32 [N], bary fp32 [N,2] = the weights of the triangle's second and
    third corner, side int8 [N]): per ray o + t d the valid triangle with the smallest t in [t_min, t_max], ties to the smallest triangle
    index.  side = +1 when the ray meets the side the stored winding's normal points to, -1 otherwise.  A ray with a component that is not
    finite or with d = 0: NaN, NaN, -1, NaN, 0; a miss: +inf, +inf, -1, NaN, 0.  brute_force: the scan over all triangles with the same
    per-triangle function -- the same bits, the yardstick.  return_evaluated: also int32 [N], the triangle tests per ray."""
    origins, directions, grid = _check_pair(origins, directions, ('origins', 'directions'), grid)
    t_min, t_max = _check_window(t_min, t_max)
    if not isinstance(brute_force, bool):
        raise TypeError(f'brute_force must be a bool, got {type(brute_force).__name__}')
    out, evaluated = _cast(origins, directions, grid, t_min, t_max, brute_force, False, return_evaluated)
    return (out, evaluated) if return_evaluated else out


def occluded(origins, directions, grid, t_min=0.0, t_max=math.inf):
    """-> uint8 [N]: 1 iff the ray meets a valid triangle inside [t_min, t_max] -- by definition `first_hits(...).triangle >= 0`, found by a
    walk that leaves at the first accepted triangle."""
    origins, directions, grid = _check_pair(origins, directions, ('origins', 'directions'), grid)
    t_min, t_max = _check_window(t_min, t_max)
    return _cast(origins, directions, grid, t_min, t_max, False, True, False)[0]


def segment_visible(p, q, grid, bias=1e-4):
    """-> uint8 [N]: 1 iff no valid triangle meets the segment from p to q between the fractions `bias` and 1 - `bias` of it (so both ends may
    lie on the surface): `occluded` with d = q - p (one fp32 subtraction) negated.  p == q counts as visible."""
    p, q, grid = _check_pair(p, q, ('p', 'q'), grid)
    bias = _check_number(bias, 'bias')
    if not 0.0 <= bias < 0.5:
        raise ValueError(f'bias must lie in [0, 0.5), got {bias!r}')
    return 1 - _cast(p, q - p, grid, bias, 1.0 - bias, False, True, False)[0]


def _tables(rays, rotations):
    k = np.arange(rays, dtype=np.float64)[None, :]
    j = np.arange(rotations, dtype=np.float64)[:, None]
    u = (k + 0.5) / np.float64(rays)
    phi = k * GOLDEN_ANGLE + ((2.0 * math.pi) * j) / np.float64(rotations)
    r = np.sqrt(u)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.broadcast_to(np.sqrt(1.0 - u), phi.shape)], -1).astype(np.float32)


def ao_tables(rays, rotations=16, device='cuda'):
    """-> fp32 [rotations, rays, 3] on the device: per table j a cosine-weighted spiral round +z, u = (k + 1/2) / rays, phi = k * golden angle
    + 2 pi j / rotations, direction (sqrt(u) cos phi, sqrt(u) sin phi, sqrt(1 - u)); built on the host in float64, rounded once.  Cosine
    weighting makes all weights equal: occlusion is a count."""
    return torch.from_numpy(_tables(_check_count(rays), _check_rotations(rotations))).to(device)


def ambient_occlusion(points, normals, grid, rays=32, radius=None, bias=None, rotations=16, *, tables=None):
    """-> fp32 [N] in [0, 1]: the fraction of `rays` cosine-weighted directions round the normal that leave the point unoccluded within
    `radius` (None: +inf), cast from p + bias * n (bias None: 1e-3 of the grid's cell, as an fp32 number).  Point i uses table
    ((uint32)i * 2654435761) >> (32 - log2 rotations).  NaN for a point or normal that is not finite and for a zero normal; 1 on a grid
    without valid triangles.  tables: the result of `ao_tables(rays, rotations)` to reuse."""
    points, normals, grid = _check_pair(points, normals, ('points', 'normals'), grid)
    rays, rotations = _check_count(rays), _check_rotations(rotations)
    radius = math.inf if radius is None else _fp32(radius, 'radius', True)
    if bias is None:
        with np.errstate(over='ignore'):
            bias = float(np.float32(1e-3) * np.float32(grid.cell))
        bias = bias if math.isfinite(bias) else 0.0
    else:
        bias = _fp32(bias, 'bias', False)
    dev, N = points.device, int(points.shape[0])
    if tables is None:
        tables = ao_tables(rays, rotations, dev)
    if not isinstance(tables, torch.Tensor) or tables.dtype != torch.float32 or tuple(tables.shape) != (rotations, rays, 3) or tables.device != dev:
        raise ValueError(f'tables must be fp32 [{rotations},{rays},3] on {dev}')
    tables = tables.contiguous()
    out = torch.empty([N], dtype=torch.float32, device=dev)
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_rays_ao', points.data_ptr(), normals.data_ptr(), N, tables.data_ptr(), rotations, rays, bias, radius, grid.vertices.data_ptr(),
                  grid.triangles.data_ptr(), int(grid.triangles.shape[0]), int(grid.vertices.shape[0]), c_lo, grid.cell, c_dims, grid.cell_start.data_ptr(),
                  grid.pair_triangle.data_ptr(), int(grid.pair_triangle.shape[0]), out.data_ptr(), _lib.stream_of(points))
    return out


def vertex_occlusion(vertices, triangles, rays=32, radius=None, bias=None, grid=None, vertex_normals=None, rotations=16):
    """-> fp32 [V] in [0, 1]: `ambient_occlusion` at the vertices of a mesh along its vertex normals (`mesh_surface.vertex_normals` unless
    given), against the mesh itself (`build_grid` unless given); 1 where it is NaN (a vertex no triangle names has no normal)."""
    vertices, triangles = _check_mesh(vertices, triangles)
    _check_count(rays)
    if grid is None:
        grid = build_grid(vertices, triangles)
    if vertex_normals is None:
        from . import mesh_surface
        vertex_normals = mesh_surface.vertex_normals(vertices, triangles)
    ao = ambient_occlusion(vertices, vertex_normals, grid, rays, radius, bias, rotations)
    return torch.nan_to_num(ao, nan=1.0)

"""Mesh distance: how far one mesh is from another, on the device (csrc/mesh_distance.hip, contract in include/tdgp.h).

    d = mesh_distance(va, ta, vb, tb)                  # MeshDistance(a_to_b, b_to_a, hausdorff, mean, rms, samples)
    grid = build_grid(vb, tb)                          # TriangleGrid: a uniform grid over the valid triangles
    c = closest_points(points, grid)                   # Closest(sqdist float64 [N], distance fp32 [N], triangle int32 [N], point fp32 [N,3])
    colours = error_colours(vertex_distances(va, grid).distance, d.hausdorff)

The measure every simplification tool is judged by: sample the surface of A (`sample_surface`: the vertices and the centroids of k*k congruent
sub-triangles per triangle, area weights), take every sample's distance to the closest point of B (`closest_points`: a walk through the
shells of a uniform grid that stops when no unseen cell can hold anything nearer), and reduce (`one_sided`: the maximum, the area-weighted
mean and RMS); then the other way round.  The maximum over both directions is the sampled Hausdorff distance: a LOWER bound of the true one
whose resolution is `spacing`.  The point-triangle distance is one pure function in double, and ties go to the smallest triangle index, so
the grid walk returns the bits of the scan over all triangles (`brute_force=True`); sums are taken in one fixed order; every array is the
same bytes on every run.  Unsigned, not differentiable.  GPU only: a CPU tensor is refused with a ValueError before any launch.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib

TriangleGrid = collections.namedtuple('TriangleGrid', ['vertices', 'triangles', 'valid', 'lo', 'hi', 'cell', 'dims', 'cell_start', 'pair_triangle', 'valid_count'])
Closest = collections.namedtuple('Closest', ['sqdist', 'distance', 'triangle', 'point'])
Samples = collections.namedtuple('Samples', ['points', 'weight', 'triangle'])
Stats = collections.namedtuple('Stats', ['max', 'mean', 'rms', 'area', 'argmax_sample', 'samples'])
MeshDistance = collections.namedtuple('MeshDistance', ['a_to_b', 'b_to_a', 'hausdorff', 'mean', 'rms', 'samples'], defaults=(None,))
CELLS_MAX = 1 << 24
PAIRS_MAX = 2 ** 31 - 1
SAMPLES_MAX = 1 << 27
K_MAX = 64
RAMP = ((0.0, (0.0, 0.0, 0.5)), (0.25, (0.0, 0.5, 1.0)), (0.5, (0.0, 1.0, 0.0)), (0.75, (1.0, 1.0, 0.0)), (1.0, (1.0, 0.0, 0.0)))


def _check_mesh(vertices, triangles, what=''):
    if not isinstance(vertices, torch.Tensor) or not isinstance(triangles, torch.Tensor):
        raise TypeError(f'{what}vertices and triangles must be tensors, got {type(vertices).__name__} and {type(triangles).__name__}')
    if vertices.dtype != torch.float32 or vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f'{what}vertices must be fp32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}')
    if triangles.dtype != torch.int32 or triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f'{what}triangles must be int32 [T,3], got {triangles.dtype} {tuple(triangles.shape)}')
    if not vertices.is_cuda or triangles.device != vertices.device:
        raise ValueError(f'{what}vertices and triangles must reside on one GPU (got {vertices.device} and {triangles.device}); mesh_distance has no CPU path')
    if max(vertices.shape[0], triangles.shape[0]) > PAIRS_MAX:
        raise ValueError(f'{what}V and T must not exceed 2^31 - 1')
    return vertices.contiguous(), triangles.contiguous()


def _check_length(x, name):
    """A cell size or a spacing -> the fp32 number as a Python float."""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.floating)):
        raise TypeError(f'{name} must be a float, got {type(x).__name__}')
    f = float(np.float32(x)) if math.isfinite(float(x)) and abs(float(x)) < 3.0e38 else float('nan')
    if not (math.isfinite(f) and f > 0):
        raise ValueError(f'{name} must be positive and finite in fp32, got {x!r}')
    return f


def _check_points(points, device):
    if not isinstance(points, torch.Tensor):
        raise TypeError(f'points must be a tensor, got {type(points).__name__}')
    if points.dtype != torch.float32 or points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f'points must be fp32 [N,3], got {points.dtype} {tuple(points.shape)}')
    if not points.is_cuda or (device is not None and points.device != device):
        raise ValueError(f'points must reside on the GPU of the grid (got {points.device}); mesh_distance has no CPU path')
    if points.shape[0] > PAIRS_MAX:
        raise ValueError('N must not exceed 2^31 - 1')
    return points.contiguous()


def _check_grid(grid):
    if not isinstance(grid, TriangleGrid):
        raise TypeError(f'grid must be the TriangleGrid `build_grid` returns, got {type(grid).__name__}')
    return grid


def _reduce(weight, distance):
    """tdgp_mesh_distance_reduce -> the workspace whose first 40 bytes hold (sum w, sum w d, sum w d d, max d, argmax)."""
    N = int(weight.shape[0])
    ws, need = _lib.byte_workspace('tdgp_mesh_distance_reduce_workspace_bytes', (N,), weight.device, ValueError(f'mesh_distance: {N} elements are more than 2^31 - 1'))
    with torch.cuda.device(weight.device):
        _lib.call('tdgp_mesh_distance_reduce', weight.data_ptr(), _lib.ptr(distance), N, ws.data_ptr(), need, _lib.stream_of(weight))
    return ws


def _prepare(vertices, triangles):
    """-> (valid uint8 [T], box fp32 [T,6], area float64 [T], valid count, area sum, lo, hi): ONE read-back."""
    dev, T, V = vertices.device, int(triangles.shape[0]), int(vertices.shape[0])
    valid = torch.empty([T], dtype=torch.uint8, device=dev)
    box = torch.empty([T, 6], dtype=torch.float32, device=dev)
    area = torch.empty([T], dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_distance_prepare', vertices.data_ptr(), triangles.data_ptr(), T, V, valid.data_ptr(), box.data_ptr(), area.data_ptr(), _lib.stream_of(vertices))
    if T == 0:
        return valid, box, area, 0, 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    ws = _reduce(area, None)
    keep = valid.bool()[:, None]
    inf = torch.full([], float('inf'), dtype=torch.float32, device=dev)
    lo = torch.where(keep, box[:, :3], inf).amin(0)                         # minima and maxima are exact in any order: plumbing
    hi = torch.where(keep, box[:, 3:], -inf).amax(0)
    host = torch.cat([ws[:8].view(torch.float64), valid.sum(dtype=torch.int64).double()[None], lo.double(), hi.double()]).cpu().tolist()
    count = int(host[1])
    if count == 0:
        return valid, box, area, 0, 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    return valid, box, area, count, host[0], tuple(host[2:5]), tuple(host[5:8])


def _default_cell(count, area_sum):
    """Twice the root of the mean triangle area as an fp32 number; 1 for a mesh without area."""
    if count == 0:
        return 1.0
    with np.errstate(over='ignore'):
        c = float(np.float32(2.0 * math.sqrt(area_sum / count)))
    return c if math.isfinite(c) and c > 0 else 1.0


def default_cell(vertices, triangles):
    """The cell `build_grid` starts from without `cell`, and the spacing `sample_surface` uses without `spacing`."""
    vertices, triangles = _check_mesh(vertices, triangles)
    _, _, _, count, area_sum, _, _ = _prepare(vertices, triangles)
    return _default_cell(count, area_sum)


def grid_dims(lo, hi, cell):
    """n_k = floor((hi_k - lo_k) / cell) + 1 in double on the fp32 numbers."""
    return tuple(int(math.floor((h - l) / cell)) + 1 for l, h in zip(lo, hi))


def _c_grid(lo, dims):
    return (ctypes.c_float * 3)(*lo), (ctypes.c_int * 3)(*dims)


def build_grid(vertices, triangles, cell=None):
    """-> TriangleGrid(vertices, triangles, valid uint8 [T], lo, hi, cell, dims, cell_start int32 [cells + 1], pair_triangle int32 [P],
    valid_count).  lo / hi: the fp32 box of the valid triangles; dims_k = floor(extent_k / cell) + 1; cell_start[c] .. cell_start[c + 1] is the
    list of cell c = (cz*dims_1 + cy)*dims_0 + cx in pair_triangle, ascending in triangle id.  `cell` (default: twice the root of the mean
    triangle area) is doubled until the grid has at most 2^24 cells and the lists at most 2^31 - 1 entries; `.cell` is the one used."""
    vertices, triangles = _check_mesh(vertices, triangles)
    if cell is not None:
        cell = _check_length(cell, 'cell')
    dev, T = vertices.device, int(triangles.shape[0])
    valid, box, _, count, area_sum, lo, hi = _prepare(vertices, triangles)
    cell = _default_cell(count, area_sum) if cell is None else cell
    if count == 0:
        return TriangleGrid(vertices, triangles, valid, lo, hi, cell, (1, 1, 1), torch.zeros([2], dtype=torch.int32, device=dev), torch.zeros([0], dtype=torch.int32, device=dev), 0)
    counts = torch.empty([T], dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.stream_of(vertices)
        while True:
            dims = grid_dims(lo, hi, cell)
            if dims[0] * dims[1] * dims[2] <= CELLS_MAX:
                c_lo, c_dims = _c_grid(lo, dims)
                _lib.call('tdgp_mesh_distance_grid_count', box.data_ptr(), valid.data_ptr(), T, c_lo, cell, c_dims, counts.data_ptr(), stream)
                P = int(counts.sum(dtype=torch.int64).cpu())                    # the one read-back per try
                if P <= PAIRS_MAX:
                    break
            with np.errstate(over='ignore'):
                cell = float(np.float32(cell) * np.float32(2))                  # inf in the end: one cell
        cells = dims[0] * dims[1] * dims[2]
        pair_cell = torch.empty([P], dtype=torch.int32, device=dev)
        pair_tri = torch.empty([P], dtype=torch.int32, device=dev)
        ws, need = _lib.byte_workspace('tdgp_mesh_distance_scan_workspace_bytes', (T,), dev, ValueError(f'build_grid: T = {T} is more than 2^31 - 1'))
        _lib.call('tdgp_mesh_distance_grid_emit', box.data_ptr(), counts.data_ptr(), T, c_lo, cell, c_dims, ws.data_ptr(), need, pair_cell.data_ptr(), pair_tri.data_ptr(), P,
                  stream)
        key, order = torch.sort(pair_cell, stable=True)                         # plumbing: the pairs were written in triangle order
        pair_tri = pair_tri[order].contiguous()
        key = key.contiguous()
        cell_start = torch.empty([cells + 1], dtype=torch.int32, device=dev)
        _lib.call('tdgp_mesh_distance_cell_start', key.data_ptr(), P, cells, cell_start.data_ptr(), stream)
    return TriangleGrid(vertices, triangles, valid, lo, hi, cell, dims, cell_start, pair_tri, count)


def closest_points(points, grid, brute_force=False, *, return_evaluated=False):
    """-> Closest(sqdist float64 [N], distance fp32 [N] = sqrt(sqdist) rounded once, triangle int32 [N], point fp32 [N,3]): per point the
    closest point of the grid's mesh, ties to the smallest triangle index.  A point with a coordinate that is not finite: NaN, NaN, -1, NaN; a
    grid without valid triangles: +inf, +inf, -1, NaN.  brute_force: the scan over all triangles with the same per-triangle function -- the
    same bits, the yardstick.  return_evaluated: also int32 [N], the triangles evaluated per point."""
    grid = _check_grid(grid)
    points = _check_points(points, grid.vertices.device)
    if not isinstance(brute_force, bool):
        raise TypeError(f'brute_force must be a bool, got {type(brute_force).__name__}')
    dev, N = points.device, int(points.shape[0])
    sqdist = torch.empty([N], dtype=torch.float64, device=dev)
    distance = torch.empty([N], dtype=torch.float32, device=dev)
    triangle = torch.empty([N], dtype=torch.int32, device=dev)
    point = torch.empty([N, 3], dtype=torch.float32, device=dev)
    evaluated = torch.empty([N], dtype=torch.int32, device=dev) if return_evaluated else None
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_distance_closest', points.data_ptr(), N, grid.vertices.data_ptr(), grid.triangles.data_ptr(), int(grid.triangles.shape[0]),
                  int(grid.vertices.shape[0]), grid.valid.data_ptr(), c_lo, grid.cell, c_dims, grid.cell_start.data_ptr(),
                  grid.pair_triangle.data_ptr(), int(grid.pair_triangle.shape[0]), int(brute_force), sqdist.data_ptr(), distance.data_ptr(), triangle.data_ptr(),
                  point.data_ptr(), _lib.ptr(evaluated), _lib.stream_of(points))
    out = Closest(sqdist, distance, triangle, point)
    return (out, evaluated) if return_evaluated else out


def vertex_distances(vertices, grid):
    """`closest_points` on the vertices of a mesh: the per-vertex error map (`error_colours` turns `.distance` into colours)."""
    return closest_points(vertices, grid)


def sample_surface(vertices, triangles, spacing=None):
    """-> Samples(points fp32 [S,3], weight float64 [S], triangle int32 [S]).  Per valid triangle, k = ceil(longest edge / spacing) clamped
    into [1, 64]: its three vertices with weight 0 (they count in the maximum only), then the centroids of its k*k congruent sub-triangles
    with weight area / k^2 (the upright ones row by row, then the inverted ones).  spacing: default `default_cell` of this mesh."""
    vertices, triangles = _check_mesh(vertices, triangles)
    if spacing is not None:
        spacing = _check_length(spacing, 'spacing')
    dev, T, V = vertices.device, int(triangles.shape[0]), int(vertices.shape[0])
    valid, _, _, count, area_sum, _, _ = _prepare(vertices, triangles)
    spacing = _default_cell(count, area_sum) if spacing is None else spacing
    counts = torch.empty([T], dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.stream_of(vertices)
        _lib.call('tdgp_mesh_distance_sample_count', vertices.data_ptr(), triangles.data_ptr(), T, V, valid.data_ptr(), spacing, counts.data_ptr(), stream)
        S = int(counts.sum(dtype=torch.int64).cpu()) if T else 0
        if S > SAMPLES_MAX:
            raise ValueError(f'sample_surface: spacing = {spacing!r} gives {S} samples, more than 2^27; use a larger spacing')
        points = torch.empty([S, 3], dtype=torch.float32, device=dev)
        weight = torch.empty([S], dtype=torch.float64, device=dev)
        triangle = torch.empty([S], dtype=torch.int32, device=dev)
        ws, need = _lib.byte_workspace('tdgp_mesh_distance_scan_workspace_bytes', (T,), dev, ValueError(f'sample_surface: T = {T} is more than 2^31 - 1'))
        _lib.call('tdgp_mesh_distance_sample_emit', vertices.data_ptr(), triangles.data_ptr(), T, V, counts.data_ptr(), spacing, ws.data_ptr(), need, points.data_ptr(),
                  weight.data_ptr(), triangle.data_ptr(), S, stream)
    return Samples(points, weight, triangle)


def stats_from_sums(sum_w, sum_wd, sum_wdd, d_max, argmax, samples):
    """The five numbers of the reduction -> Stats: mean = sum w d / sum w, rms = sqrt(sum w d^2 / sum w) (NaN without area)."""
    mean = sum_wd / sum_w if sum_w > 0 else float('nan')
    rms = math.sqrt(sum_wdd / sum_w) if sum_w > 0 and sum_wdd >= 0 else float('nan')
    return Stats(d_max if argmax >= 0 else float('nan'), mean, rms, sum_w, argmax, samples)


def one_sided(samples, grid, *, return_distances=False):
    """-> Stats(max, mean, rms, area, argmax_sample, samples): the distances of the samples to the grid's mesh.  max: the largest fp32
    distance, at the lowest sample index among equals; mean and rms weigh by area (the sums in double in the one order include/tdgp.h
    states); area = the sum of the weights; samples = their number.  One read-back."""
    if not isinstance(samples, Samples):
        raise TypeError(f'samples must be the Samples `sample_surface` returns, got {type(samples).__name__}')
    c = closest_points(samples.points, grid)
    ws = _reduce(samples.weight, c.distance)
    head = ws[:40].cpu()
    s = head[:32].view(torch.float64).tolist()
    st = stats_from_sums(s[0], s[1], s[2], s[3], int(head[32:40].view(torch.int64)), int(samples.points.shape[0]))
    return (st, c.distance) if return_distances else st


def pool(a, b):
    """Two one-sided Stats pooled by area -> (mean, rms)."""
    area = a.area + b.area
    if not area > 0:
        return float('nan'), float('nan')
    return (a.mean * a.area + b.mean * b.area) / area, math.sqrt(((a.rms * a.rms) * a.area + (b.rms * b.rms) * b.area) / area)


def mesh_distance(va, ta, vb, tb, spacing=None, symmetric=True, return_samples=False):
    """-> MeshDistance(a_to_b, b_to_a, hausdorff, mean, rms, samples).  a_to_b: `one_sided` of the samples of A against B; b_to_a (None unless
    symmetric) the other way round, each mesh sampled at `spacing` (default: its own `default_cell`).  hausdorff = the larger maximum; mean and
    rms pool both directions by area.  return_samples: samples = ((distance fp32 [S], weight float64 [S]) of A, the same of B or None), for
    quantiles (`renderer.quantile_select`).  A sampled LOWER bound of the true Hausdorff distance; its resolution is the spacing."""
    va, ta = _check_mesh(va, ta, 'A: ')
    vb, tb = _check_mesh(vb, tb, 'B: ')
    if va.device != vb.device:
        raise ValueError(f'both meshes must reside on one GPU, got {va.device} and {vb.device}')
    if spacing is not None:
        spacing = _check_length(spacing, 'spacing')
    if not isinstance(symmetric, bool) or not isinstance(return_samples, bool):
        raise TypeError('symmetric and return_samples must be bools')
    sa = sample_surface(va, ta, spacing)
    ab, da = one_sided(sa, build_grid(vb, tb), return_distances=True)
    kept = [(da, sa.weight), None]
    if not symmetric:
        return MeshDistance(ab, None, ab.max, ab.mean, ab.rms, tuple(kept) if return_samples else None)
    sb = sample_surface(vb, tb, spacing)
    ba, db = one_sided(sb, build_grid(va, ta), return_distances=True)
    kept[1] = (db, sb.weight)
    mean, rms = pool(ab, ba)
    worst = [m for m in (ab.max, ba.max) if not math.isnan(m)]
    return MeshDistance(ab, ba, max(worst) if worst else float('nan'), mean, rms, tuple(kept) if return_samples else None)


def error_colours(d, d_max):
    """Distances [V] -> colours fp32 [V,3] in [0, 1]: a fixed ramp (dark blue, light blue, green, yellow, red) over d / d_max clamped into
    [0, 1]; what is not finite shows as red.  Fits geometry.save_ply(colours=) and mesh.render_mesh_views(mode='colour', vertex_colours=)."""
    if not isinstance(d, torch.Tensor) or d.ndim != 1:
        raise ValueError('d must be a tensor [V]')
    d_max = float(d_max)
    if not (math.isfinite(d_max) and d_max >= 0):
        raise ValueError(f'd_max must be finite and not negative, got {d_max!r}')
    x = d.float() / d_max if d_max > 0 else torch.zeros_like(d, dtype=torch.float32)
    x = torch.nan_to_num(x, nan=1.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    out = torch.zeros([d.shape[0], 3], dtype=torch.float32, device=d.device)
    for (x0, c0), (x1, c1) in zip(RAMP[:-1], RAMP[1:]):
        t = ((x - x0) / (x1 - x0)).clamp(0.0, 1.0)[:, None]
        seg = torch.tensor(c0, dtype=torch.float32, device=d.device) * (1 - t) + torch.tensor(c1, dtype=torch.float32, device=d.device) * t
        inside = ((x >= x0) & ((x < x1) | (x1 == 1.0)))[:, None]
        out = torch.where(inside, seg, out)
    return out

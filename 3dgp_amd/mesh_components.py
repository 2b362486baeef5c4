"""Mesh components: the connected components of the indexed mesh `geometry.marching_cubes` leaves on the device, their measurements, and
an order-preserving filter (csrc/mesh_components.hip, contract in include/tdgp.h).

The raw level set holds the object and every disconnected speck of density above the threshold.  The reference's users split the mesh on
the host with `trimesh` and keep the largest piece; here the mesh never leaves the device:

    comps = components(vertices, triangles)            # labels -> dense ids -> counts, area, signed volume, bounding box per component
    mask = select(comps, keep=1)                       # plain tensor logic: which components stay
    v, t, attrs, vmap = keep_components(vertices, triangles, comps, mask, attributes=(colours,))
    v, t, attrs, vmap = clean_mesh(vertices, triangles, attributes=(colours,), keep=1)      # the three in a row

Connectivity: two vertices are connected when a triangle names both, so triangles sharing one vertex are in one component; a vertex no
triangle names is a component of its own (with zero triangles: `select` never keeps it).  Components are numbered by their smallest vertex.
Every integer output is a pure function of the mesh and every fp64 output the same bytes on every run.  Host read-backs: the index range
of the triangles (one pair, for validation), K, and (V', T').  GPU only: the kernels have no CPU path; `select` alone also runs on CPU tensors.
"""
import collections
import ctypes

import torch

from . import _lib

Components = collections.namedtuple('Components', ['component', 'triangles', 'vertices', 'area', 'volume', 'bbox_min', 'bbox_max'])
BY = ('triangles', 'area')


def _check_triangle_shape(triangles, num_vertices):
    if not isinstance(triangles, torch.Tensor):
        raise TypeError(f'triangles must be a tensor, got {type(triangles).__name__}')
    if triangles.dtype != torch.int32 or triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f'triangles must be int32 [T,3], got {triangles.dtype} {tuple(triangles.shape)}')
    V = int(num_vertices)
    if V < 0 or V > 2 ** 31 - 1 or triangles.shape[0] > 2 ** 31 - 1:
        raise ValueError(f'num_vertices = {V} and T = {triangles.shape[0]} must lie in [0, 2^31 - 1]')


def _check_triangles(triangles, num_vertices):
    """Shape and dtype, then the device, then -- before any launch -- the index range: one amin / amax read-back."""
    _check_triangle_shape(triangles, num_vertices)
    _lib.require_cuda(triangles, 'triangles')
    triangles = triangles.contiguous()
    if triangles.shape[0] > 0:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(triangles)).cpu())
        if lo < 0 or hi >= int(num_vertices):
            raise ValueError(f'triangles index vertices {lo} .. {hi}, outside [0, {int(num_vertices)})')
    return triangles


def _check_mesh(vertices, triangles):
    if not isinstance(vertices, torch.Tensor):
        raise TypeError(f'vertices must be a tensor, got {type(vertices).__name__}')
    if vertices.dtype != torch.float32 or vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f'vertices must be fp32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}')
    _check_triangle_shape(triangles, vertices.shape[0])
    _lib.require_cuda(vertices, 'vertices')
    triangles = _check_triangles(triangles, vertices.shape[0])
    if triangles.device != vertices.device:
        raise ValueError(f'vertices and triangles must share a device, got {vertices.device} and {triangles.device}')
    return vertices.contiguous(), triangles


def _workspace(query, *sizes, device):
    return _lib.byte_workspace(query, sizes, device, ValueError(f'{query}{sizes}: sizes outside [0, 2^31 - 1]'))


def _labels(triangles, V, return_retries=False):
    dev = triangles.device
    T = int(triangles.shape[0])
    label = torch.empty([V], dtype=torch.int32, device=dev)
    ws, need = _workspace('tdgp_mesh_labels_workspace_bytes', T, V, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_labels', triangles.data_ptr(), T, V, label.data_ptr(), ws.data_ptr(), need, _lib.stream_of(triangles))
    return (label, int(ws[:8].view(torch.int64).cpu())) if return_retries else label


def vertex_labels(triangles, num_vertices, return_retries=False):
    """triangles int32 [T,3] on the device -> label int32 [V]: label[v] is the smallest vertex index of v's component.
    return_retries=True: also the number of compare-and-swaps the union pass had to repeat (a diagnostic; one more read-back)."""
    triangles = _check_triangles(triangles, num_vertices)
    return _labels(triangles, int(num_vertices), return_retries)


def _component_ids(label):
    dev, V = label.device, int(label.shape[0])
    component = torch.empty([V], dtype=torch.int32, device=dev)
    ws, need = _workspace('tdgp_mesh_component_ids_workspace_bytes', V, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_component_ids', label.data_ptr(), V, component.data_ptr(), ws.data_ptr(), need, _lib.stream_of(label))
    return component, int(ws[:8].view(torch.int64).cpu())                               # K: the one number read back


def components(vertices, triangles):
    """vertices fp32 [V,3], triangles int32 [T,3] on the device -> Components(component int32 [V] -- the dense id of every vertex, ids ordered by
    the components' smallest vertices --, triangles int64 [K], vertices int64 [K], area fp64 [K], volume fp64 [K] (signed: positive for a blob
    of high density under `marching_cubes`' winding), bbox_min / bbox_max fp32 [K,3]).  A triangle belongs to the component of its first vertex."""
    return _components(*_check_mesh(vertices, triangles))


def _components(vertices, triangles):
    dev = vertices.device
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    component, K = _component_ids(_labels(triangles, V))
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)                      # noqa: E731
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)                    # noqa: E731
    tri_count, vert_count, area, volume = i64(K), i64(K), f64(K), f64(K)
    bbox_min, bbox_max = (torch.empty([K, 3], dtype=torch.float32, device=dev) for _ in range(2))
    tri_key = torch.empty([T], dtype=torch.int32, device=dev)
    area_term, vol_term = f64(T), f64(T)
    with torch.cuda.device(dev):
        stream = _lib.stream_of(vertices)
        _lib.call('tdgp_mesh_component_stats', vertices.data_ptr(), triangles.data_ptr(), T, V, component.data_ptr(), K, tri_count.data_ptr(),
                  vert_count.data_ptr(), bbox_min.data_ptr(), bbox_max.data_ptr(), tri_key.data_ptr(), area_term.data_ptr(), vol_term.data_ptr(), stream)
        # grouping is plumbing: a stable sort keeps the triangle order inside every component, the prefix of the counts finds the groups
        order = torch.sort(tri_key, stable=True).indices if T else i64(0)
        start = torch.cumsum(tri_count, 0) - tri_count
        _lib.call('tdgp_mesh_component_sums', order.data_ptr(), start.data_ptr(), tri_count.data_ptr(), K, T, area_term.data_ptr(), vol_term.data_ptr(),
                  area.data_ptr(), volume.data_ptr(), stream)
    return Components(component, tri_count, vert_count, area, volume, bbox_min, bbox_max)


def select(comps, keep=1, by='triangles', min_triangles=0, min_fraction=0.0):
    """Which components stay -> bool [K] on the tensors' device (plain tensor logic, no read-back; CPU tensors work too).
    A component is kept when ALL of these hold: it has at least one triangle; it is among the `keep` largest by `by` ('triangles' or
    'area'; ties go to the lower id; keep='all' or keep >= K: no limit); it has at least `min_triangles` triangles; its measure is at least
    `min_fraction` of the largest component's."""
    if by not in BY:
        raise ValueError(f'by must be one of {BY}, got {by!r}')
    if keep != 'all' and (isinstance(keep, bool) or not isinstance(keep, int) or keep < 0):
        raise ValueError(f"keep must be a non-negative int or 'all', got {keep!r}")
    if int(min_triangles) < 0 or not 0.0 <= float(min_fraction) <= 1.0:
        raise ValueError(f'min_triangles must be >= 0 and min_fraction in [0, 1], got {min_triangles!r}, {min_fraction!r}')
    tris = comps.triangles
    K = int(tris.shape[0])
    if K == 0:
        return torch.zeros([0], dtype=torch.bool, device=tris.device)
    measure = tris.to(torch.float64) if by == 'triangles' else comps.area.to(torch.float64)
    ok = (tris > 0) & (tris >= int(min_triangles)) & (measure >= float(min_fraction) * measure.max())
    if keep != 'all' and keep < K:
        order = torch.sort(measure, descending=True, stable=True).indices           # stable: equal measures stay in id order
        rank = torch.empty_like(order)
        rank[order] = torch.arange(K, dtype=order.dtype, device=order.device)
        ok &= rank < keep
    return ok


def _check_attributes(attributes, vertices):
    out = []
    for i, a in enumerate(attributes):
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.ndim != 2 or a.shape[0] != vertices.shape[0] or a.shape[1] < 1:
            raise ValueError(f'attribute {i} must be fp32 [{vertices.shape[0]}, C], got {getattr(a, "dtype", type(a).__name__)} {tuple(getattr(a, "shape", ()))}')
        _lib.require_cuda(a, f'attribute {i}')
        out.append(a.contiguous())
    return out


def keep_components(vertices, triangles, comps, mask, attributes=()):
    """The mesh without the components whose `mask` entry (bool / uint8 [K]) is false -> (vertices' [V',3], triangles' int32 [T',3],
    attributes' (a tuple of [V',C] for every fp32 [V,C] given), vertex_map int32 [V]: the new index of every vertex, or -1).  Kept vertices
    and kept triangles stay in their original order; positions come from scans, so the outputs are the same bytes on every run.  The only
    read-back is (V', T')."""
    vertices, triangles = _check_mesh(vertices, triangles)
    return _keep_components(vertices, triangles, comps, mask, _check_attributes(attributes, vertices))


def _keep_components(vertices, triangles, comps, mask, attributes):
    dev = vertices.device
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    component = comps.component
    K = int(comps.triangles.shape[0])
    if not isinstance(component, torch.Tensor) or component.dtype != torch.int32 or tuple(component.shape) != (V,) or component.device != dev:
        raise ValueError(f'comps.component must be int32 [{V}] on {dev} (the Components of THIS mesh)')
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (K,):
        raise ValueError(f'mask must be bool [{K}], got {getattr(mask, "dtype", type(mask).__name__)} {tuple(getattr(mask, "shape", ()))}')
    _lib.require_cuda(mask, 'mask')
    component = component.contiguous()
    keep = mask.to(torch.uint8).contiguous()
    vertex_map = torch.empty([V], dtype=torch.int32, device=dev)
    ws, need = _workspace('tdgp_mesh_compact_workspace_bytes', T, V, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.stream_of(vertices)
        _lib.call('tdgp_mesh_compact_count', triangles.data_ptr(), T, V, component.data_ptr(), keep.data_ptr(), K, ws.data_ptr(), need, stream)
        V2, T2 = (int(x) for x in ws[:16].view(torch.int64).cpu())
        out_v = torch.empty([V2, 3], dtype=torch.float32, device=dev)
        out_t = torch.empty([T2, 3], dtype=torch.int32, device=dev)
        out_a = [torch.empty([V2, a.shape[1]], dtype=torch.float32, device=dev) for a in attributes]
        n = len(attributes)
        a_in = (ctypes.c_void_p * max(n, 1))(*[a.data_ptr() for a in attributes])
        a_out = (ctypes.c_void_p * max(n, 1))(*[a.data_ptr() for a in out_a])
        a_ch = (ctypes.c_int32 * max(n, 1))(*[int(a.shape[1]) for a in attributes])
        _lib.call('tdgp_mesh_compact_emit', vertices.data_ptr(), triangles.data_ptr(), T, V, component.data_ptr(), keep.data_ptr(), K, ws.data_ptr(), need,
                  out_v.data_ptr(), V2, out_t.data_ptr(), T2, vertex_map.data_ptr(), a_in, a_out, a_ch, n, stream)
    return out_v, out_t, tuple(out_a), vertex_map


def clean_mesh(vertices, triangles, attributes=(), return_components=False, **select_kwargs):
    """`components` -> `select(**select_kwargs)` -> `keep_components`: (vertices', triangles', attributes', vertex_map).  An empty mesh passes
    through as empty [0,3] tensors.  return_components=True: also (Components, mask), e.g. to report what was dropped."""
    vertices, triangles = _check_mesh(vertices, triangles)                   # validated once; the three steps below trust it
    attributes = _check_attributes(attributes, vertices)
    comps = _components(vertices, triangles)
    mask = select(comps, **select_kwargs)
    out = _keep_components(vertices, triangles, comps, mask, attributes)
    return (*out, comps, mask) if return_components else out

"""Mesh decimation: round-based quadric edge collapse (Garland-Heckbert 1997) with a link-condition test, for the indexed mesh
`geometry.marching_cubes` leaves on the device (csrc/mesh_decimate.hip, contract in include/tdgp.h).

    d = decimate(vertices, triangles, target_triangles=100_000)       # Decimated(vertices [V',3], triangles [T',3], attributes, vertex_map [V],
    d = decimate(vertices, triangles, max_error=0.05)                 #           triangle_map [T'], rounds, stopped)

Where `mesh_simplify` merges whatever shares a grid cell, this keeps the surface a surface: an edge is collapsed only when the link condition
holds, no neighbouring triangle flips and (with max_error) the area-weighted RMS distance of the new vertex to the planes it stands for stays
within the bound -- a closed, consistently oriented input stays closed, oriented and of the same topology.  A round collapses an independent
set of edges at once: every candidate claims its two one-rings with a 64-bit atomic minimum of (cost, hashed corner id), and the edges that
still own their endpoints and opposite vertices are applied together.  No priority queue; every output is a pure function of the arrays as
given -- the same bytes on every run.  A round removes only a few percent of the vertices, so a 10x reduction takes tens of rounds, each with
one host read-back (the number selected) besides the corner table's and the triangle count's.  The quadric sums follow corner-table order, so
they are NOT invariant under a permutation of the triangles.  The rim is pinned as found in front of round 0.  GPU only: no CPU path.
"""
import collections
import math

import torch

from . import _lib
from . import mesh_simplify as _mesh_simplify
from . import mesh_surface as _mesh_surface

Decimated = collections.namedtuple('Decimated', ['vertices', 'triangles', 'attributes', 'vertex_map', 'triangle_map', 'rounds', 'stopped'])
STOPPED = ('target', 'exhausted', 'max_rounds')
OPTIONS = ('target_triangles', 'max_error', 'max_rounds', 'rank_tol', 'fix_boundary')
MIX_MULTIPLIERS = (0x7feb352d, 0x846ca68b)


def mix(h):
    """The tie-break of a key: a bijection on uint32 (xor-shifts and multiplications by odd constants), as the kernel computes it."""
    h &= 0xffffffff
    h ^= h >> 16
    h = (h * MIX_MULTIPLIERS[0]) & 0xffffffff
    h ^= h >> 15
    h = (h * MIX_MULTIPLIERS[1]) & 0xffffffff
    return h ^ (h >> 16)


def max_collapses(T, target_triangles):
    """kmax of a round: a collapse removes two triangles, so ceil((T - target) / 2) of them reach the target."""
    return max(0, -((target_triangles - T) // 2))


def _check_args(target_triangles, max_error, max_rounds, rank_tol, fix_boundary):
    """Checked without a device -> (target or None, max_error as a float or 0.0 for none, max_rounds, rank_tol, fix_boundary)."""
    if target_triangles is None and max_error is None:
        raise ValueError('decimate needs target_triangles, max_error or both')
    if target_triangles is not None and (isinstance(target_triangles, bool) or not isinstance(target_triangles, int) or target_triangles < 0):
        raise ValueError(f'target_triangles must be a non-negative int, got {target_triangles!r}')
    if max_error is not None:
        if isinstance(max_error, bool) or not isinstance(max_error, (int, float)):
            raise TypeError(f'max_error must be a float, got {type(max_error).__name__}')
        max_error = float(max_error)
        if not (math.isfinite(max_error) and max_error > 0):
            raise ValueError(f'max_error must be positive and finite, got {max_error!r}')
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or max_rounds < 0:
        raise ValueError(f'max_rounds must be a non-negative int, got {max_rounds!r}')
    if isinstance(rank_tol, bool) or not isinstance(rank_tol, (int, float)):
        raise TypeError(f'rank_tol must be a float, got {type(rank_tol).__name__}')
    rank_tol = float(rank_tol)
    if not (math.isfinite(rank_tol) and rank_tol >= 0):
        raise ValueError(f'rank_tol must be finite and not negative, got {rank_tol!r}')
    if not isinstance(fix_boundary, bool):
        raise TypeError(f'fix_boundary must be a bool, got {type(fix_boundary).__name__}')
    return target_triangles, 0.0 if max_error is None else max_error, max_rounds, rank_tol, fix_boundary


def _compact(tri, V, parent, tmap):
    """Relabel through `parent`, drop what repeats an index or leaves [0, V), keep the order -> (triangles, triangle_map)."""
    ct, rotated = _mesh_simplify._relabel(tri, V, parent)
    out_t, kept = _mesh_simplify._emit(ct, *_mesh_simplify._count(rotated, False))
    return out_t, (kept if tmap is None else tmap[kept.long()])


def decimate(vertices, triangles, target_triangles=None, max_error=None, max_rounds=256, rank_tol=1e-3, fix_boundary=True, attributes=(), *, history=None):
    """-> Decimated(vertices fp32 [V',3], triangles int32 [T',3], attributes (fp32 [V',c], ...), vertex_map int32 [V], triangle_map int32 [T'],
    rounds, stopped).  Edges are collapsed, cheapest first within every neighbourhood, until at most `target_triangles` are left ('target'), a
    round selects nothing ('exhausted') or `max_rounds` have run ('max_rounds'); rounds counts every round run, the empty last one included.
    max_error (in the units of `vertices`): a collapse is allowed only while the area-weighted RMS distance of the new vertex to the planes
    accumulated in it stays within the bound (not a Hausdorff bound; `mesh_distance.mesh_distance` measures that).  With both, a collapse satisfies the bound and the loop stops at the
    target.  A vertex leaves only by being merged into another; survivors keep their order (a vertex no triangle names stays), and
    vertex_map[v] is the output index of the vertex v ended up in.  Surviving triangles keep their order; triangle_map[j] is the input index
    of output triangle j.  A triangle with an index outside [0, V) or a repeated index is dropped in front of round 0.  fix_boundary: the rim
    (`mesh_surface.boundary_vertices` of the input) neither moves nor leaves.  attributes: fp32 [V,c] arrays; the survivor of a collapse gets
    the two ends' values interpolated at the projection of the new position onto the edge.  history: a list that receives, per round,
    (triangles in front of it, edges selected, edges collapsed).  include/tdgp.h has the operations, in order."""
    target, max_error, max_rounds, rank_tol, fix_boundary = _check_args(target_triangles, max_error, max_rounds, rank_tol, fix_boundary)
    vertices, triangles = _mesh_surface._check_mesh(vertices, triangles)
    attributes = _mesh_simplify._check_attributes(attributes, vertices)
    dev, V = vertices.device, int(vertices.shape[0])
    channels = [int(a.shape[1]) for a in attributes]
    C = sum(channels)
    parent = torch.arange(V, dtype=torch.int32, device=dev)
    tri, tmap = _compact(triangles, V, parent, None)
    T = int(tri.shape[0])
    pos = torch.empty([V, 3], dtype=torch.float64, device=dev)
    quadric = torch.empty([V, 10], dtype=torch.float64, device=dev)
    weight = torch.empty([V], dtype=torch.float64, device=dev)
    attr = torch.cat([a.double() for a in attributes], dim=1).contiguous() if C else None
    rim = None
    table = _mesh_surface._corner_table(tri, V) if V > 0 else None
    with torch.cuda.device(dev):
        stream = _lib.stream_of(vertices)
        if V > 0:
            if fix_boundary and T > 0:
                rim = _mesh_surface._boundary(tri, V, table)
            _lib.call('tdgp_mesh_decimate_quadrics', vertices.data_ptr(), tri.data_ptr(), T, V, table.start.data_ptr(), table.corner.data_ptr(), pos.data_ptr(),
                      quadric.data_ptr(), weight.data_ptr(), stream)
        best = torch.empty([V], dtype=torch.int64, device=dev)
        rounds = 0
        while True:
            if target is not None and T <= target:
                stopped = 'target'
                break
            if rounds >= max_rounds:
                stopped = 'max_rounds'
                break
            if T == 0 or V == 0:
                stopped = 'exhausted'
                break
            table = _mesh_surface._corner_table(tri, V) if table is None else table
            key = torch.empty([3 * T], dtype=torch.int64, device=dev)
            place = torch.empty([3 * T, 3], dtype=torch.float64, device=dev)
            opposite = torch.empty([3 * T, 2], dtype=torch.int32, device=dev)
            flag = torch.empty([3 * T], dtype=torch.uint8, device=dev)
            selected = torch.empty([3 * T], dtype=torch.int32, device=dev)
            ws, need = _lib.byte_workspace('tdgp_mesh_decimate_select_workspace_bytes', (T,), dev, ValueError(f'decimate: 3 T = {3 * T} is more than the 2^31 - 1 it indexes'))
            mesh = (tri.data_ptr(), T, V, table.start.data_ptr(), table.corner.data_ptr())
            _lib.call('tdgp_mesh_decimate_candidates', pos.data_ptr(), quadric.data_ptr(), weight.data_ptr(), _lib.ptr(rim), *mesh, max_error, rank_tol, key.data_ptr(),
                      place.data_ptr(), opposite.data_ptr(), stream)
            _lib.call('tdgp_mesh_decimate_claim', key.data_ptr(), *mesh, best.data_ptr(), stream)
            _lib.call('tdgp_mesh_decimate_select', key.data_ptr(), best.data_ptr(), opposite.data_ptr(), tri.data_ptr(), T, V, flag.data_ptr(), selected.data_ptr(),
                      ws.data_ptr(), need, stream)
            K = int(ws[:8].view(torch.int64).cpu())                                     # the one number read back per round
            rounds += 1
            table = None
            if history is not None:
                history.append((T, K, K if target is None else min(K, max_collapses(T, target))))
            if K == 0:
                stopped = 'exhausted'
                break
            selected = selected[:K]
            if target is not None and K > max_collapses(T, target):                    # the cheapest kmax: keys are distinct, a sort is plumbing
                K = max_collapses(T, target)
                selected = selected[torch.sort(key[selected.long()]).indices[:K]].contiguous()
            _lib.call('tdgp_mesh_decimate_apply', selected.data_ptr(), K, tri.data_ptr(), T, V, _lib.ptr(rim), place.data_ptr(), pos.data_ptr(), quadric.data_ptr(),
                      weight.data_ptr(), _lib.ptr(attr), C, parent.data_ptr(), stream)
            tri, tmap = _compact(tri, V, parent, tmap)
            T = int(tri.shape[0])
        ws, need = _lib.byte_workspace('tdgp_mesh_decimate_gather_workspace_bytes', (V,), dev, ValueError(f'decimate: V = {V} is more than the 2^31 - 2 it indexes'))
        _lib.call('tdgp_mesh_decimate_gather_count', parent.data_ptr(), V, ws.data_ptr(), need, stream)
        V_out = int(ws[:8].view(torch.int64).cpu())
        out_v = torch.empty([V_out, 3], dtype=torch.float32, device=dev)
        out_a = torch.empty([V_out, C], dtype=torch.float32, device=dev) if C else None
        vmap = torch.empty([V], dtype=torch.int32, device=dev)
        _lib.call('tdgp_mesh_decimate_gather', pos.data_ptr(), _lib.ptr(attr), C, parent.data_ptr(), V, rounds + 1, ws.data_ptr(), need, out_v.data_ptr(), V_out,
                  _lib.ptr(out_a), vmap.data_ptr(), stream)
    out_t = _mesh_simplify._relabel(tri, V, vmap)[0]
    outs, at = [], 0
    for c in channels:
        outs.append(out_a[:, at:at + c].contiguous())
        at += c
    return Decimated(out_v, out_t, tuple(outs), vmap, tmap, rounds, stopped)


def apply(vertices, triangles, options, attributes=()):
    """The `decimate=` argument of geometry.extract_geometry / mesh.render_mesh_frames: a dict of `decimate` keyword arguments -> Decimated."""
    return decimate(vertices, triangles, attributes=attributes, **check_options(options))


def check_options(options):
    """A `decimate=` dict, checked without a device -> a copy."""
    if not isinstance(options, dict):
        raise TypeError(f'decimate must be None or a dict of mesh_decimate.decimate arguments, got {type(options).__name__}')
    kw = dict(options)
    if set(kw) - set(OPTIONS):
        raise ValueError(f'decimate: unknown options {sorted(set(kw) - set(OPTIONS))}; known: {sorted(OPTIONS)}')
    _check_args(kw.get('target_triangles'), kw.get('max_error'), kw.get('max_rounds', 256), kw.get('rank_tol', 1e-3), kw.get('fix_boundary', True))
    return kw

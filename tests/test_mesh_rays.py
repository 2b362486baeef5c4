"""Mesh rays without a GPU: the properties of the restatement (tests/mesh_rays_reference.py) that make it worth being the yardstick -- the
walk through the grid returns the bits of the scan over all triangles on adversarial rays, no ray passes between the triangles of a closed
mesh, t agrees with the plane formula, `side` with the normal, the direction tables are what the contract says, closed and convex meshes
give the exact occlusions -- and the host side of 3dgp_amd/mesh_rays.py: refusals before any launch, the layout integers, the ABI."""
import functools
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import mc_reference as MC
import mesh_components_reference as CR
import mesh_distance_reference as MD
import mesh_raster_reference as MR
import mesh_rays_reference as R
import mesh_surface_reference as SR
import shapes_reference as SH

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
NEW = ['tdgp_mesh_rays_cast', 'tdgp_mesh_rays_ao']
PLANE_TOLERANCE = 4.5e-15                   # twice the 2.25e-15 measured below


def _mc_mesh():
    """Marching cubes of speck_volume(24) by the numpy marcher: the mesh of the GPU tests up to the order of its axes."""
    spec = importlib.util.spec_from_file_location('tool_gen_mc_table_rays', os.path.join(REPO, 'tools', 'gen_mc_table.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    vol = CR.speck_volume(24)
    ids = MC.crossing_edge_ids(vol, 0.0)
    return MC.edge_vertices(vol, 0.0, ids), np.searchsorted(ids, MC.marcher(vol, 0.0, gen.table(), gen.edge_info)).astype(np.int32)


MESHES = {
    'icosphere(2)': (lambda: MR.icosphere(2)[:2], (0.25, 0.7, 1e6)),
    'cube': (lambda: (CR.CUBE_V, CR.CUBE_T), (0.125, 0.5, 1e6)),
    'lattice(6)': (lambda: SR.lattice(6)[:2], (0.5, 1.5, 1e6)),
    'marching cubes': (_mc_mesh, (1.0, 3.0, 1e6)),
    'soup': (lambda: MD.soup(120, seed=7), (0.4, 1.25, 1e6)),
}


@functools.lru_cache(maxsize=None)
def grid_of(name, k):
    v, t = MESHES[name][0]()
    return MD.build_grid(np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32), MESHES[name][1][k])


def same(got, want):
    return [f for f in got._fields if getattr(got, f).tobytes() != getattr(want, f).tobytes()]


@pytest.mark.parametrize('name', list(MESHES))
def test_the_walk_returns_the_bits_of_the_scan(name):
    """254 rays per mesh (origins inside the box and up to 4x outside it, rays that miss the box, axis-parallel ones, rays in a cell face,
    through cell corners and along cell edges of the finest grid, at vertices and fp32-rounded edge midpoints, starting on the surface) at
    three cell sizes, and with three windows that cut hits off: (t, depth, triangle, bary, side) identical, any-hit equal to `a hit exists`."""
    fine = grid_of(name, 0)
    o, d = R.adversarial_rays(fine, seed=11)
    assert len(o) == 254
    want = R.scan_rays(o, d, fine)
    hit = want.triangle >= 0
    assert 40 <= hit.sum() <= 240 and np.isinf(want.t[~hit]).all() and (want.side[hit] != 0).all() and (want.side[~hit] == 0).all()
    b = want.bary[hit].astype(D)
    assert (b >= 0).all() and (b.sum(1) <= 1 + 1e-6).all()
    for k in range(3):
        grid = grid_of(name, k)
        ev, cells = [], []
        got = R.first_hits(o, d, grid, evaluated=ev, cells=cells)
        assert not same(got, want), (name, grid.dims, same(got, want))
        print(f'{name} grid {grid.dims}: {np.mean(ev):.1f} triangle tests and {np.mean(cells):.1f} cells per ray on the walk, {grid.valid_count} on the scan')
    assert grid.dims == (1, 1, 1)
    assert not same(R.first_hits(o, d, fine, brute_force=True), want)
    mid = float(np.median(want.t[hit & (want.t > 0)]))
    for window in ((0.0, mid), (mid, np.inf), (0.5 * mid, 1.5 * mid)):
        cut = R.scan_rays(o, d, fine, *window)
        assert not same(R.first_hits(o, d, fine, *window), cut), (name, window)
        assert (cut.t[cut.triangle >= 0] >= window[0]).all() and (cut.t[cut.triangle >= 0] <= window[1]).all()
        assert ((cut.triangle != want.triangle) & hit).sum() >= 10                                  # the window does cut first hits off
        assert np.array_equal(R.occluded(o, d, fine, *window, walk=True), (cut.triangle >= 0).astype(np.uint8))
        assert np.array_equal(R.occluded(o, d, fine, *window), (cut.triangle >= 0).astype(np.uint8))


def test_rays_that_are_no_rays_and_empty_grids():
    grid = grid_of('cube', 0)
    o = np.array([[np.nan, 0, 0], [0.5, 0.5, -1], [0.5, 0.5, -1], [0.5, 0.5, -1], [5, 5, 5]], F)
    d = np.array([[0, 0, 1], [0, np.inf, 1], [0, 0, 0], [0, 0, 1], [1, 0, 0]], F)
    for got in (R.scan_rays(o, d, grid), R.first_hits(o, d, grid)):
        assert np.isnan(got.t[:3]).all() and np.isnan(got.depth[:3]).all() and (got.triangle[:3] == -1).all() and np.isnan(got.bary[:3]).all() and (got.side[:3] == 0).all()
        assert got.t[3] == 1.0 and got.depth[3] == F(1.0) and got.triangle[3] == 8 and got.side[3] == 1           # on the diagonal of the face z = 0: triangles 8 and 9 share it
        assert got.t[4] == np.inf and got.triangle[4] == -1 and got.side[4] == 0 and np.isnan(got.bary[4]).all()
    empty = MD.build_grid(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    for got in (R.scan_rays(o, d, empty), R.first_hits(o, d, empty)):
        assert np.isnan(got.t[:3]).all() and np.isinf(got.t[3:]).all() and (got.triangle == -1).all()


def test_no_ray_passes_between_the_triangles_of_a_closed_mesh():
    """icosphere(2) from an interior point: every ray to a vertex, to an fp32-rounded edge midpoint, and 2000 seeded random ones hits, and
    always from the same side (the inner one: -1)."""
    v, t = MR.icosphere(2)[:2]
    grid = MD.build_grid(v, t, 0.25)
    p = np.array([0.11, -0.07, 0.05], F)
    edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1), axis=0)
    mids = ((v[edges[:, 0]].astype(D) + v[edges[:, 1]].astype(D)) / 2.0).astype(F)
    rs = np.random.RandomState(4)
    targets = np.concatenate([v, mids, p + rs.randn(2000, 3).astype(F)])
    d = (targets - p).astype(F)
    assert len(edges) == 480 and len(d) == 162 + 480 + 2000 and (d != 0).any(1).all()
    got = R.scan_rays(np.broadcast_to(p, d.shape), d, grid)
    assert (got.triangle >= 0).all() and (got.side == -1).all() and (got.t > 0).all() and np.isfinite(got.t).all()
    # at a vertex or on an edge the hit is shared: the smallest triangle index among those that hold it
    at_vertex = got.triangle[:162]
    assert all(i in t[at_vertex[i]] for i in range(162))
    walked = R.first_hits(np.broadcast_to(p, (642, 3)), d[:642], grid)
    assert not same(walked, R.Hits(*(x[:642] for x in got)))
    # from outside every ray that hits enters through the outer side
    o = (3.0 * targets[642:1142] / np.linalg.norm(targets[642:1142], axis=1, keepdims=True)).astype(F)
    out = R.scan_rays(o, (-o).astype(F), grid)
    assert (out.triangle >= 0).all() and (out.side == 1).all()


def test_t_against_the_plane_formula_and_side_against_the_normal():
    """t of the sheared form against n.(a - o) / n.d on the random hits of two meshes; side = +1 iff the stored winding's normal points
    against d.  Both formulas are a handful of double operations on the same inputs: measured 2.25e-15 relative at worst over 439 hits with t > 1e-3
    (rays from up to one box size outside, aimed into the box), asserted at twice that."""
    worst, count = 0.0, 0
    for name in ('icosphere(2)', 'soup'):
        grid = grid_of(name, 1)
        rs = np.random.RandomState(8)
        lo, hi = np.array(grid.lo), np.array(grid.hi)
        o = (lo - (hi - lo) + rs.rand(400, 3) * 3 * (hi - lo)).astype(F)
        d = ((lo + rs.rand(400, 3) * (hi - lo)) - o).astype(F)
        h = R.scan_rays(o, d, grid)
        k = np.flatnonzero((h.triangle >= 0) & (h.t > 1e-3))
        a, b, c = MD._corners(grid.vertices, grid.triangles, h.triangle[k])
        n = np.cross(b - a, c - a)
        od, dd = o[k].astype(D), d[k].astype(D)
        plane = (n * (a - od)).sum(1) / (n * dd).sum(1)
        rel = np.abs(plane - h.t[k]) / h.t[k]
        worst, count = max(worst, float(rel.max())), count + len(k)
        assert np.array_equal(h.side[k], np.where((n * dd).sum(1) < 0, 1, -1))
        x = od + h.t[k, None] * dd                                                                  # the hit point from t and from the weights
        w = h.bary[k].astype(D)
        y = a * (1 - w.sum(1))[:, None] + b * w[:, :1] + c * w[:, 1:]
        assert np.abs(x - y).max() < 1e-5
    print(f't against the plane formula on {count} hits: {worst:.3e} relative at worst, {PLANE_TOLERANCE:.1e} allowed')
    assert count >= 200 and worst <= PLANE_TOLERANCE


def test_the_direction_tables():
    for rays in (16, 32, 64):
        for rotations in (1, 16):
            tab = R.ao_tables(rays, rotations)
            assert tab.shape == (rotations, rays, 3) and tab.dtype == F
            ln = np.sqrt((tab.astype(D) ** 2).sum(-1))
            assert np.abs(ln - 1).max() <= 2 * np.finfo(F).eps and (tab[..., 2] > 0).all()
            assert np.allclose(np.sort(tab[0, :, 2].astype(D) ** 2), 1 - (np.arange(rays)[::-1] + 0.5) / rays, atol=1e-6)      # cosine-weighted: z^2 uniform
            assert abs(float(tab[..., :2].astype(D).mean())) < 0.05                                # no preferred azimuth
            if rotations > 1:
                assert not np.array_equal(tab[0], tab[1]) and np.array_equal(tab[0, :, 2], tab[1, :, 2])
    tdgp_tables = importlib.import_module('3dgp_amd').mesh_rays._tables
    assert tdgp_tables(32, 16).tobytes() == R.ao_tables(32, 16).tobytes()                           # the product builds the same bytes


def test_ambient_occlusion_of_a_closed_convex_mesh_and_of_a_wall():
    v, t = MR.icosphere(2)[:2]
    grid = MD.build_grid(v, t, 0.25)
    outward = v.copy()
    tab = R.ao_tables(32, 16)
    bias = float(F(1e-3) * F(grid.cell))
    assert (R.ambient_occlusion(v, outward, grid, tab, bias) == 1.0).all()                          # convex: nothing above the tangent plane
    assert (R.ambient_occlusion(v, -outward, grid, tab, bias) == 0.0).all()                         # closed: no way out
    few = slice(0, 12)
    assert np.array_equal(R.ambient_occlusion(v[few], -outward[few], grid, tab, bias, walk=True), np.zeros(12, F))
    assert np.array_equal(R.ambient_occlusion(v[few], outward[few], grid, tab, bias, walk=True), np.ones(12, F))
    bad_p, bad_n = v[:3].copy(), outward[:3].copy()
    bad_p[0, 1], bad_n[1] = np.nan, 0.0
    got = R.ambient_occlusion(bad_p, bad_n, grid, tab, bias)
    assert np.isnan(got[:2]).all() and got[2] == 1.0
    assert (R.ambient_occlusion(v[:5], outward[:5], MD.build_grid(v, t[:0]), tab, bias) == 1.0).all()
    # the centre of a large square facing up, a vertical wall through the centre: half the hemisphere, by the cosine measure too
    s, hgt = 50.0, 200.0
    wv = np.array([[-s, -s, 0], [s, -s, 0], [s, s, 0], [-s, s, 0], [0.25, -s, 0], [0.25, s, 0], [0.25, s, hgt], [0.25, -s, hgt]], F)
    wt = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    wall = MD.build_grid(wv, wt, 25.0)
    pts, nrm = np.zeros((64, 3), F), np.tile(np.array([[0, 0, 1]], F), (64, 1))
    for rays in (16, 32, 64):
        tabs = R.ao_tables(rays, 16)
        scan = R.ambient_occlusion(pts, nrm, wall, tabs, 1e-3)
        walk = R.ambient_occlusion(pts[:16], nrm[:16], wall, tabs, 1e-3, walk=True)
        assert np.array_equal(walk, scan[:16])
        print(f'wall over half the hemisphere, {rays} rays: mean {scan.mean():.4f} (analytic 0.5, wall at x = 0.25 of height 200), per point {scan.min():.4f} .. {scan.max():.4f}')
        assert (R.ambient_occlusion(pts, nrm, wall, tabs, 1e-3, radius=0.2) == 1.0).all()          # the wall is farther than the radius


def test_the_rasteriser_against_the_rays_on_the_cpu():
    """The precondition of the GPU cross-check: the two numpy restatements alone, icosphere(1) under two pinhole cameras at 128 x 128, must
    disagree on fewer than 1 % of the pixels (measured: 0 and 0 of 16384; the largest depth difference where they agree: 6.3e-04, the
    rasteriser's depth being that of its snapped triangle)."""
    v, t = MR.icosphere(1, 0.3)
    grid = MD.build_grid(v, t)
    for fov, radius in ((40.0, 1.0), (50.0, 1.1)):
        o, d = SH.pinhole_rays(128, fov, radius)
        c2w, focal = MR.pinhole_camera(fov, radius)
        fr = MR.frames(v, t, c2w, focal, o, d, 128, 128, 1e-3, 'none', 0.0, 0.0)
        h = R.scan_rays(o, d, grid)
        status = (h.triangle >= 0).astype(np.int32)
        agree = (status == fr['status']) & (h.triangle == fr['tri'])
        both = agree & (status == 1)
        diff = np.abs(h.depth[both].astype(D) - fr['t_hit'][both].astype(D)).max()
        print(f'fov {fov} radius {radius}: {(~agree).sum()} of {agree.size} pixels differ, {status.mean():.3f} hit, depth differs by {diff:.3e} at most')
        assert (~agree).mean() < 0.01 and status.mean() > 0.2


# ------------------------------------------------------------------------------------------------ the host side
def _cpu_grid(tdgp):
    v, t = torch.tensor(CR.CUBE_V), torch.tensor(CR.CUBE_T)
    return tdgp.mesh_distance.TriangleGrid(v, t, torch.ones(12, dtype=torch.uint8), (0.0,) * 3, (1.0,) * 3, 1.0, (1, 1, 1), torch.tensor([0, 12], dtype=torch.int32),
                                           torch.arange(12, dtype=torch.int32), 12)


def test_refusals_before_any_launch(tdgp):
    M = tdgp.mesh_rays
    grid = _cpu_grid(tdgp)
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    for call in (lambda: M.first_hits(o, d, grid), lambda: M.occluded(o, d, grid), lambda: M.segment_visible(o, d, grid), lambda: M.ambient_occlusion(o, d, grid),
                 lambda: M.vertex_occlusion(grid.vertices, grid.triangles)):
        with pytest.raises(ValueError, match='GPU'):
            call()
    with pytest.raises(TypeError, match='TriangleGrid'):
        M.first_hits(o, d, (grid.vertices, grid.triangles))
    for bad in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 2), torch.zeros(12)):
        with pytest.raises(ValueError, match=r'fp32 \[N,3\]'):
            M.first_hits(bad, d, grid)
    for rays in (0, 8, 20, 128, 32.0, True):
        with pytest.raises(ValueError, match='rays'):
            M.ao_tables(rays)
        with pytest.raises(ValueError, match='rays'):
            M._check_count(rays)
    for rotations in (0, 3, 128, 2.0):
        with pytest.raises(ValueError, match='rotations'):
            M.ao_tables(32, rotations)
    for window in ((float('nan'), 1.0), (0.0, float('nan')), (2.0, 1.0), (float('-inf'), 1.0), (float('inf'), float('inf'))):
        with pytest.raises(ValueError, match='t_min'):
            M._check_window(*window)
    assert M._check_window(0, float('inf')) == (0.0, float('inf')) and M._check_window(-1.0, -1.0) == (-1.0, -1.0)
    with pytest.raises(TypeError):
        M._check_window('0', 1.0)
    for bias in (-1e-3, float('nan'), float('inf'), 1e39):
        with pytest.raises(ValueError, match='bias'):
            M._fp32(bias, 'bias', False)
    for radius in (0.0, -1.0, float('nan'), 1e-50):
        with pytest.raises(ValueError, match='radius'):
            M._fp32(radius, 'radius', True)
    assert M._fp32(0.0, 'bias', False) == 0.0 and M._fp32(float('inf'), 'radius', True) == float('inf') and M._fp32(0.1, 'radius', True) == float(F(0.1))
    assert M.RAYS == (16, 32, 64) and M.ROTATIONS_MAX == 64 and M.Hits._fields == ('t', 'depth', 'triangle', 'bary', 'side')
    assert M.GOLDEN_ANGLE == R.GOLDEN_ANGLE


def test_the_entry_points_in_header_binding_and_source(tdgp):
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    source = open(os.path.join(REPO, '3dgp_amd', 'csrc', 'mesh_rays.hip')).read()
    plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NEW:
        proto = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', plain)
        assert proto, name
        assert len(proto.group(1).split(',')) == len(tdgp._lib._PROTOTYPES[name][1]), name               # one ctypes type per parameter
        assert re.search(r'TDGP_API int ' + name + r'\(', source), name
    assert 'mesh_rays.hip' in tdgp.build.SOURCES and 'mesh_rays' in tdgp.__doc__
    for doc in ('README.md', 'DESIGN.md'):                                                          # the count the documents state is the table's
        assert f'{len(tdgp._lib.EXPORTS)} entry points' in open(os.path.join(REPO, doc)).read()
    assert 'asm' not in source and 'atomic' not in re.sub(r'//.*', '', source) and '__shared__' not in source

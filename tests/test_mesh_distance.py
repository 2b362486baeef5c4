"""Mesh distance without a GPU: the properties of the restatement (tests/mesh_distance_reference.py) that make it worth being the yardstick
-- the shell walk returns the bits of the scan over all triangles, the per-triangle function is a lower envelope of the triangle's points,
analytic pairs give their analytic distances, the two directions are not mixed up -- and the host side of 3dgp_amd/mesh_distance.py:
refusals before any launch, the layout integers, the colour ramp, the tool's readers and the ABI."""
import functools
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_components_reference as CR
import mesh_distance_reference as R
import mesh_raster_reference as MR
import mesh_surface_reference as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
NEW = ['tdgp_mesh_distance_prepare', 'tdgp_mesh_distance_grid_count', 'tdgp_mesh_distance_scan_workspace_bytes', 'tdgp_mesh_distance_grid_emit',
       'tdgp_mesh_distance_cell_start', 'tdgp_mesh_distance_closest', 'tdgp_mesh_distance_sample_count', 'tdgp_mesh_distance_sample_emit',
       'tdgp_mesh_distance_reduce_workspace_bytes', 'tdgp_mesh_distance_reduce']


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_distance_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('T,cells', [(60, 1), (90, 2), (120, 4), (160, 6), (200, 9)])
def test_the_walk_returns_the_bits_of_the_scan(T, cells):
    """Random soups with a collinear triangle, a two-vertices-coincide triangle and invalid ones, grids from 1^3 to 9^3 cells, 210 queries
    each: inside the box, up to 4x outside it, on vertices, on cell faces."""
    v, t = R.soup(T, seed=T)
    probe = R.build_grid(v, t, cell=1e6)
    assert probe.dims == (1, 1, 1)
    extent = max(h - l for l, h in zip(probe.lo, probe.hi))
    grid = R.build_grid(v, t, cell=extent / (cells - 0.5)) if cells > 1 else probe
    assert max(grid.dims) == cells and grid.valid_count == T - 4
    pts = R.query_points(grid, seed=T + 1, n=70)
    assert len(pts) == 210
    walked, scanned = [], []
    walk, scan = R.closest_points(pts, grid, evaluated=walked), R.closest_points(pts, grid, brute_force=True, evaluated=scanned)
    assert walk.sqdist.tobytes() == scan.sqdist.tobytes() and walk.triangle.tobytes() == scan.triangle.tobytes()
    assert walk.point.tobytes() == scan.point.tobytes() and walk.distance.tobytes() == scan.distance.tobytes()
    many = R.scan_points(pts, grid)                                                             # the scan as arrays: what the GPU tests compare with
    assert all(x.tobytes() == y.tobytes() for x, y in zip(many, scan))
    assert (scan.triangle >= 0).all() and not set(scan.triangle.tolist()) & {12, 13, 14, 15}
    print(f'T = {T}, grid {grid.dims}: {np.mean(walked):.1f} evaluations per point on the walk, {np.mean(scanned):.1f} on the scan')
    if cells >= 6:
        assert np.mean(walked[:70]) < np.mean(scanned[:70])                                     # inside the box the walk prunes


def test_the_per_triangle_function_is_never_above_the_triangle_s_points():
    """d2 against the minimum over a 61-step barycentric lattice of the triangle, 200 random cases.  Coordinates are O(1), so the rounding of
    either side is a few 1e-16 of the squared scale: 1e-12 absolute and 1e-9 relative are orders above it and orders below any real error."""
    rs = np.random.RandomState(0)
    k = 60
    i, j = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing='ij')
    keep = i + j <= k
    u, w = (i[keep] / k)[:, None], (j[keep] / k)[:, None]
    worst = 0.0
    for case in range(200):
        a, b, c, p = rs.randn(4, 3).astype(F).astype(D) * (0.05 if case % 4 == 0 else 1.0)
        if case % 10 == 0:
            c = a + (b - a) * 2.0                                                               # collinear
        if case % 25 == 0:
            b = a.copy()                                                                        # two vertices coincide
        d2, q = R.point_triangle(p, a, b, c)
        lattice = a + u * (b - a) + w * (c - a)
        m = ((lattice - p) ** 2).sum(1).min()
        assert d2 <= m * (1 + 1e-9) + 1e-12, (case, float(d2), m)
        assert abs(((q - p) ** 2).sum() - d2) <= 1e-12 + 1e-9 * d2                               # q is at that distance
        worst = max(worst, m - float(d2))
    assert worst > 0


@functools.lru_cache(maxsize=None)
def cube_pair():
    va, t = CR.CUBE_V.copy(), CR.CUBE_T.copy()
    vb = va + np.array([0.25, 0, 0], F)
    return va, t, vb, R.mesh_distance(va, t, vb, t, spacing=0.25)


def test_unit_cube_against_its_shifted_copy():
    va, t, vb, d = cube_pair()
    sa = R.sample_surface(va, t, 0.25)
    assert len(sa.points) == 468 and d.a_to_b.samples == d.b_to_a.samples == 468
    assert np.bincount(sa.triangle).tolist() == [39] * 12                                       # k = ceil(sqrt(2) / 0.25) = 6: 36 + 3
    assert d.a_to_b.max == d.b_to_a.max == d.hausdorff == 0.25
    for s, (v0, v1) in ((d.a_to_b, (va, vb)), (d.b_to_a, (vb, va))):
        c = R.closest_points(R.sample_surface(v0, t, 0.25).points[s.argmax_sample][None], R.build_grid(v1, t))
        assert c.sqdist[0] == 0.0625 and c.distance[0] == F(0.25)
        assert abs(s.area - 6.0) <= 6e-12
        assert abs(s.mean - 0.0868) < 5e-4 and abs(s.rms - 0.1360) < 5e-4, (s.mean, s.rms)
    print(f'cube vs cube + 0.25 x: mean {d.mean:.6f}, rms {d.rms:.6f}')
    assert abs(d.mean - 0.0868) < 5e-4 and abs(d.rms - 0.1360) < 5e-4


def test_icosphere_against_a_larger_one():
    v, t = MR.icosphere(2)[:2]
    w = MR.icosphere(2, radius=1.1)[0]
    d = R.mesh_distance(v, t, w, t, spacing=0.2, brute_force=True)                               # (the walk of the restatement takes 13 s here)
    print(f'icosphere(2) r 1 vs r 1.1: inner -> outer max {d.a_to_b.max!r}, outer -> inner max {d.b_to_a.max!r}, {d.a_to_b.samples} samples')
    assert d.a_to_b.samples == d.b_to_a.samples == 2240
    assert abs(d.a_to_b.max - 0.09856) < 1e-5
    assert abs(d.b_to_a.max - 0.1) <= 2 * float(np.spacing(F(1.1)))                           # the vertices of both spheres are rounded to fp32
    assert d.hausdorff == d.b_to_a.max and d.a_to_b.max < d.b_to_a.max


def test_the_directions_are_not_mixed_up():
    va, t = CR.CUBE_V, CR.CUBE_T
    vb = np.concatenate([va, np.array([[3, 0, 0], [3, 0.125, 0], [3, 0, 0.125]], F)])
    tb = np.concatenate([t, np.array([[8, 9, 10]], np.int32)])
    d = R.mesh_distance(va, t, vb, tb, spacing=0.25)
    assert d.a_to_b.max == 0.0 and d.a_to_b.mean == 0.0 and d.a_to_b.rms == 0.0
    assert d.b_to_a.max == 2.0 and d.hausdorff == 2.0 and d.b_to_a.argmax_sample >= 468
    one = R.mesh_distance(va, t, vb, tb, spacing=0.25, symmetric=False)
    assert one.b_to_a is None and one.hausdorff == 0.0


def test_layout_integers():
    v, t = SR.lattice(6)[:2]
    g = R.build_grid(v, t, cell=1.0)
    assert g.dims == (6, 6, 1) and g.lo == (0.0, 0.0, 0.0) and g.hi == (5.0, 5.0, 0.0) and len(g.cell_start) == 37
    assert g.cell_start[0] == 0 and g.cell_start[-1] == len(g.pair_triangle) and (np.diff(g.cell_start) >= 0).all()
    for c in range(36):
        l = g.pair_triangle[g.cell_start[c]:g.cell_start[c + 1]]
        assert (np.diff(l) > 0).all()
    assert R.default_cell(v, t) == float(F(2.0 * math.sqrt(0.5)))                              # 50 triangles of area 1/2
    for spacing, k in ((2.0, 1), (1.0, 2), (0.75, 2), (0.01, 64)):
        s = R.sample_surface(v, t, spacing)
        assert np.bincount(s.triangle).tolist() == [k * k + 3] * len(t) and abs(R.fixed_sum(s.weight) - 25.0) < 1e-10
    sv, st = R.soup(60, seed=3)
    s = R.sample_surface(sv, st, 0.5)
    assert not set(s.triangle.tolist()) & {12, 13, 14, 15} and set(s.triangle.tolist()) == set(range(60)) - {12, 13, 14, 15}
    empty = R.build_grid(sv, st[12:16])
    assert empty.dims == (1, 1, 1) and empty.valid_count == 0 and R.closest_points(sv[:2], empty).triangle.tolist() == [-1, -1]
    c = R.closest_points(np.array([[np.nan, 0, 0], [0, np.inf, 0]], F), g)
    assert np.isnan(c.sqdist).all() and c.triangle.tolist() == [-1, -1] and np.isnan(c.point).all()
    x = np.random.RandomState(1).rand(70000)
    assert abs(R.fixed_sum(x) - math.fsum(x)) < 1e-9 and R.fixed_sum([]) == 0.0
    assert R.reduce([1.0, 1.0, 1.0], [F(2), F('nan'), F(2)])[3:] == (2.0, 0)


def test_refusals_come_before_any_launch(tdgp):
    M = tdgp.mesh_distance
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    grid = M.TriangleGrid(v, t, None, (0.0,) * 3, (0.0,) * 3, 1.0, (1, 1, 1), None, None, 0)
    bad = [lambda: M.build_grid(v, t), lambda: M.sample_surface(v, t, 0.5), lambda: M.mesh_distance(v, t, v, t), lambda: M.default_cell(v, t),
           lambda: M.closest_points(v, grid), lambda: M.vertex_distances(v, grid), lambda: M.build_grid(v.double(), t), lambda: M.build_grid(v[:, :2], t),
           lambda: M.build_grid(v, t.long()), lambda: M.build_grid(v, t.reshape(6)), lambda: M._check_length(0.0, 'cell'), lambda: M._check_length(-1.0, 'cell'),
           lambda: M._check_length(float('nan'), 'spacing'), lambda: M._check_length(float('inf'), 'spacing'), lambda: M._check_length(1e-50, 'cell'),
           lambda: M._check_length(1e39, 'cell'), lambda: M.error_colours(torch.zeros(3), -1.0), lambda: M.error_colours(torch.zeros(3, 2), 1.0)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'call {k} did not raise')
    with pytest.raises(ValueError, match='no CPU path'):
        M.build_grid(v, t)
    for call in (lambda: M.build_grid([0], t), lambda: M._check_length('wide', 'cell'), lambda: M._check_length(True, 'cell'), lambda: M.closest_points(v, (1, 2)),
                 lambda: M.one_sided((v, v, v), grid)):
        with pytest.raises(TypeError):
            call()
    assert M._check_length(0.1, 'cell') == float(F(0.1)) and M.grid_dims((0.0, 0.0, 0.0), (5.0, 5.0, 0.0), 1.0) == (6, 6, 1)
    assert M._default_cell(50, 25.0) == float(F(2.0 * math.sqrt(0.5))) and M._default_cell(0, 0.0) == 1.0 and M._default_cell(3, 0.0) == 1.0
    assert M.stats_from_sums(2.0, 1.0, 1.0, 3.0, 7, 9) == R.stats_from_sums(2.0, 1.0, 1.0, 3.0, 7, 9) == (3.0, 0.5, math.sqrt(0.5), 2.0, 7, 9)
    a, b = R.Stats(1.0, 0.5, 0.75, 2.0, 0, 4), R.Stats(2.0, 0.25, 0.5, 6.0, 1, 4)
    assert M.pool(a, b) == R.pool(a, b) and M.pool(a, b)[0] == (0.5 * 2.0 + 0.25 * 6.0) / 8.0
    assert (M.CELLS_MAX, M.PAIRS_MAX, M.SAMPLES_MAX, M.K_MAX) == (2 ** 24, 2 ** 31 - 1, 2 ** 27, 64)


def test_error_colours_are_a_fixed_ramp(tdgp):
    M = tdgp.mesh_distance
    d = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 5.0, float('nan'), float('inf')])
    c = M.error_colours(d, 2.0)
    assert c.shape == (8, 3) and c.dtype == torch.float32 and float(c.min()) >= 0 and float(c.max()) <= 1
    assert c[0].tolist() == [0.0, 0.0, 0.5] and c[2].tolist() == [0.0, 1.0, 0.0] and c[4].tolist() == c[5].tolist() == c[6].tolist() == c[7].tolist() == [1.0, 0.0, 0.0]
    assert c[1].tolist() == [0.0, 0.5, 1.0] and c[3].tolist() == [1.0, 1.0, 0.0]
    assert M.error_colours(d[:3], 0.0).tolist() == [[0.0, 0.0, 0.5]] * 3


def test_the_tool_reads_what_geometry_writes(tdgp, tmp_path):
    tool = _tool('mesh_distance')
    v, t = MR.icosphere(1)[:2]
    g = tdgp.geometry
    g.save_obj(str(tmp_path / 'a.obj'), torch.from_numpy(v), torch.from_numpy(t))
    g.save_ply(str(tmp_path / 'a.ply'), torch.from_numpy(v), torch.from_numpy(t))
    g.save_ply(str(tmp_path / 'c.ply'), torch.from_numpy(v), torch.from_numpy(t), colours=torch.rand(len(v), 3))
    for name in ('a.ply', 'c.ply'):
        rv, rt = tool.read_mesh(str(tmp_path / name))
        assert rv.dtype == F and rt.dtype == np.int32 and rv.tobytes() == v.tobytes() and rt.tobytes() == t.tobytes()
    rv, rt = tool.read_mesh(str(tmp_path / 'a.obj'))
    assert rt.tobytes() == t.tobytes() and rv.shape == v.shape and np.abs(rv - v).max() <= 1e-6   # .obj is text
    with pytest.raises(SystemExit):
        tool.parse_args(['a.obj'])
    with pytest.raises(SystemExit):
        tool.parse_args(['a.obj', 'b.obj', '--spacing', '0'])
    a = tool.parse_args(['a.obj', 'b.ply', '--spacing', '0.5', '--one-sided', '--json', 'x.json'])
    assert a.spacing == 0.5 and a.one_sided and a.json == 'x.json' and a.ply is None
    (tmp_path / 'bad.stl').write_text('solid')
    with pytest.raises(ValueError):
        tool.read_mesh(str(tmp_path / 'bad.stl'))
    ex = _tool('extract_geometry')
    assert not hasattr(ex.parse_args(['--seeds', '0']), 'distance_report') and ex.parse_args(['--seeds', '0', '--distance-report']).distance_report is True
    assert json.dumps(tool.report(R.mesh_distance(CR.CUBE_V, CR.CUBE_T, CR.CUBE_V, CR.CUBE_T, spacing=0.5)))


def test_entry_points_are_declared_bound_and_refuse_what_they_cannot_index(tdgp):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'tdgp.h')).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf'\b{name}\s*\(', header) and name in tdgp._lib.EXPORTS
    assert sorted(n for n in tdgp._lib.EXPORTS if n.startswith('tdgp_mesh_distance')) == sorted(NEW)
    assert 'mesh_distance.hip' in tdgp.build.SOURCES
    lib = tdgp._lib.load()
    F3, I3 = (tdgp._lib.c_float * 3), (tdgp._lib.c_int * 3)
    lo, one = F3(0, 0, 0), I3(1, 1, 1)
    assert lib.tdgp_mesh_distance_scan_workspace_bytes(-1) == -1 and lib.tdgp_mesh_distance_scan_workspace_bytes(2 ** 31) == -1
    assert lib.tdgp_mesh_distance_scan_workspace_bytes(0) == 64 and lib.tdgp_mesh_distance_scan_workspace_bytes(257) == 128
    assert lib.tdgp_mesh_distance_reduce_workspace_bytes(-1) == -1 and lib.tdgp_mesh_distance_reduce_workspace_bytes(2 ** 31) == -1
    assert lib.tdgp_mesh_distance_reduce_workspace_bytes(0) == 64 and lib.tdgp_mesh_distance_reduce_workspace_bytes(257) == 64 + 128
    # the argument checks of the C side come before any launch: they answer without a device
    assert lib.tdgp_mesh_distance_prepare(None, None, 2 ** 31, 4, None, None, None, None) == -1 and b'2^31 - 1' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_prepare(None, None, 4, 4, None, None, None, None) == -1 and b'null pointer' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_grid_count(None, None, 4, lo, 0.0, one, None, None) == -1 and b'cell' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_grid_count(None, None, 4, lo, 1.0, I3(0, 1, 1), None, None) == -1 and b'dimension' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_grid_count(None, None, 4, lo, 1.0, I3(512, 512, 65), None, None) == -1 and b'2^24 cells' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_grid_count(None, None, 4, F3(float('inf'), 0, 0), 1.0, one, None, None) == -1 and b'finite' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_grid_count(None, None, 4, lo, 1.0, one, None, None) == -1 and b'null pointer' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_grid_emit(None, None, 4, lo, 1.0, one, None, 0, None, None, 4, None) == -1 and b'null workspace' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_cell_start(None, 0, 0, None, None) == -1 and b'cells' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_cell_start(None, 4, 1, None, None) == -1 and b'null pointer' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_closest(None, 4, None, None, 0, 0, None, lo, 1.0, one, None, None, 0, 2, None, None, None, None, None, None) == -1 and b'brute_force' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_closest(None, 4, None, None, 0, 0, None, lo, 1.0, one, None, None, 0, 0, None, None, None, None, None, None) == -1 and b'null pointer' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_sample_count(None, None, 4, 4, None, 0.0, None, None) == -1 and b'spacing' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_sample_count(None, None, 4, 4, None, float('inf'), None, None) == -1 and b'spacing' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_sample_emit(None, None, 4, 4, None, 1.0, None, 0, None, None, None, 4, None) == -1 and b'null workspace' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_distance_reduce(None, None, 4, None, 0, None) == -1 and b'null workspace' in lib.tdgp_last_error()
    # empty inputs are no-ops that need no device
    assert lib.tdgp_mesh_distance_prepare(None, None, 0, 0, None, None, None, None) == 0
    assert lib.tdgp_mesh_distance_grid_count(None, None, 0, lo, 1.0, one, None, None) == 0
    assert lib.tdgp_mesh_distance_grid_emit(None, None, 0, lo, 1.0, one, None, 0, None, None, 0, None) == 0
    assert lib.tdgp_mesh_distance_closest(None, 0, None, None, 0, 0, None, lo, 1.0, one, None, None, 0, 0, None, None, None, None, None, None) == 0
    assert lib.tdgp_mesh_distance_sample_count(None, None, 0, 0, None, 1.0, None, None) == 0
    assert lib.tdgp_mesh_distance_sample_emit(None, None, 0, 0, None, 1.0, None, 0, None, None, None, 0, None) == 0

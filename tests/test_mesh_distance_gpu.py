"""Mesh distance on the GPU: tdgp_mesh_distance_* and the drivers of 3dgp_amd/mesh_distance.py bit for bit against the restatement of their
contract (tests/mesh_distance_reference.py, whose walk and scan tests/test_mesh_distance.py holds against each other): the grid's arrays,
closest points by the walk and by the scan at three cell sizes per mesh (identical across them: what an unsound bound would break), the
block edges of the one-wave launch, points that are not finite, the samples at k = 1, 2 and 64, the statistics of three analytic pairs, a
decimated marching-cubes mesh against its source, and the two command lines."""
import functools
import importlib
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_components_reference as CR
import mesh_distance_reference as R
import mesh_raster_reference as MR
import mesh_surface_reference as SR
from conftest import report_parity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    if isinstance(a, np.ndarray) and not a.flags.writeable:
        a = a.copy()
    return torch.as_tensor(a).to(DEV)


def H(t):
    return t.detach().cpu().numpy()


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        g, w = (a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a) for a in (got, want))
        bad = np.argwhere(g != w)
        first = tuple(bad[0]) if len(bad) else ()
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}')


def _mc_mesh():
    tdgp = importlib.import_module('3dgp_amd')
    v, t = tdgp.geometry.marching_cubes(T(CR.speck_volume(24)), 0.0)
    return H(v), H(t)


# name -> (mesh, the three cell sizes: the last one gives a 1 x 1 x 1 grid)
MESHES = {
    'icosphere(2)': (lambda: MR.icosphere(2)[:2], (0.25, 0.7, 1e6)),
    'cube': (lambda: (CR.CUBE_V, CR.CUBE_T), (0.125, 0.5, 1e6)),
    'lattice(6)': (lambda: SR.lattice(6)[:2], (0.5, 1.5, 1e6)),                                  # planar: one grid axis has 1 cell
    'marching cubes': (_mc_mesh, (1.0, 3.0, 1e6)),
    'soup': (lambda: R.soup(120, seed=7), (0.4, 1.25, 1e6)),
}
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def named_mesh(name):
    v, t = MESHES[name][0]()
    v, t = np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32)
    for a in (v, t):
        a.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def reference_grid(name, k):
    v, t = named_mesh(name)
    return R.build_grid(v, t, MESHES[name][1][k])


@functools.lru_cache(maxsize=None)
def reference_queries(name):
    """257 points (an ordinary one, one NaN, one infinite, then inside the box, up to 4x outside it, on vertices, on faces of the finest
    grid's cells) and the restatement's scan over all triangles for them: computed once, shared, never written."""
    grid = reference_grid(name, 0)
    pool = R.query_points(grid, seed=11, n=86)
    pts = np.concatenate([pool[:1], np.array([[np.nan, 0, 0], [0, -np.inf, 1]], F), pool[1:]])[:257].astype(F)
    want = R.scan_points(pts, grid)
    for a in (pts,) + tuple(want):
        a.setflags(write=False)
    return pts, want


def check_closest(got, want, what, n=None):
    assert got._fields == ('sqdist', 'distance', 'triangle', 'point')
    for f in got._fields:
        same_bytes(H(getattr(got, f)), getattr(want, f)[:n], f'{f} {what}')


def check_grid(got, want, what):
    assert got.dims == want.dims and got.lo == want.lo and got.hi == want.hi and got.cell == want.cell and got.valid_count == want.valid_count, \
        (what, got.dims, want.dims, got.lo, want.lo, got.hi, want.hi, got.cell, want.cell)
    same_bytes(H(got.valid), want.valid, 'valid ' + what)
    same_bytes(H(got.cell_start), want.cell_start, 'cell_start ' + what)
    same_bytes(H(got.pair_triangle), want.pair_triangle, 'pair_triangle ' + what)


@pytest.mark.parametrize('name', list(MESHES))
def test_closest_points_bit_for_bit(tdgp, name):
    M = tdgp.mesh_distance
    v, t = named_mesh(name)
    pts, want = reference_queries(name)
    tv, tt, tp = T(v), T(t), T(pts)
    assert np.isnan(want.sqdist[1:3]).all() and (want.triangle[1:3] == -1).all() and np.isfinite(want.sqdist[3:]).all() and (want.triangle[3:] >= 0).all()
    for k, cell in enumerate(MESHES[name][1]):
        grid = M.build_grid(tv, tt, cell)
        check_grid(grid, reference_grid(name, k), f'{name} cell {cell}')
        got, evaluated = M.closest_points(tp, grid, return_evaluated=True)
        check_closest(got, want, f'{name} cell {cell} walk')
        print(f'{name}: grid {grid.dims}, {grid.pair_triangle.shape[0]} pairs, {float(evaluated.float().mean()):.1f} triangles evaluated per point of {grid.valid_count}')
    assert grid.dims == (1, 1, 1)
    if name == 'lattice(6)':
        assert reference_grid(name, 0).dims[2] == 1 and min(reference_grid(name, 0).dims[:2]) > 1
    check_closest(M.closest_points(tp, M.build_grid(tv, tt, MESHES[name][1][0]), brute_force=True), want, f'{name} scan')
    default = M.build_grid(tv, tt)
    check_grid(default, R.build_grid(v, t), f'{name} default cell')
    assert default.cell == R.default_cell(v, t) == M.default_cell(tv, tt)
    check_closest(M.closest_points(tp, default), want, f'{name} default cell walk')


@pytest.mark.parametrize('n', COUNTS)
def test_point_counts_at_the_block_edges(tdgp, n):
    M = tdgp.mesh_distance
    v, t = named_mesh('icosphere(2)')
    pts, want = reference_queries('icosphere(2)')
    grid = M.build_grid(T(v), T(t), 0.25)
    for brute in (False, True):
        got = M.closest_points(T(pts[:n].copy()).reshape(n, 3), grid, brute_force=brute)
        assert got.sqdist.shape == (n,) and got.point.shape == (n, 3)
        check_closest(got, want, f'N = {n} brute_force = {brute}', n)


def test_grids_are_the_same_bytes_on_every_run_and_take_degenerate_meshes(tdgp):
    M = tdgp.mesh_distance
    v, t = named_mesh('marching cubes')
    tv, tt = T(v), T(t)
    a, b = M.build_grid(tv, tt, 1.0), M.build_grid(tv, tt, 1.0)
    assert torch.equal(a.cell_start, b.cell_start) and torch.equal(a.pair_triangle, b.pair_triangle) and a.dims == b.dims
    none_t = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    sv, st = named_mesh('soup')
    pts = T(sv[:5].copy())
    for what, (gv, gt) in (('T = 0', (tv, none_t)), ('all invalid', (T(sv), T(st[12:16].copy()))), ('V = 0', (torch.zeros(0, 3, device=DEV), none_t))):
        g = M.build_grid(gv, gt)
        check_grid(g, R.build_grid(H(gv), H(gt)), what)
        assert g.dims == (1, 1, 1) and g.valid_count == 0 and g.cell_start.tolist() == [0, 0] and g.pair_triangle.shape == (0,) and g.cell == 1.0
        for brute in (False, True):
            c = M.closest_points(pts, g, brute_force=brute)
            assert torch.isinf(c.sqdist).all() and torch.isinf(c.distance).all() and (c.triangle == -1).all() and torch.isnan(c.point).all(), what
        s = M.sample_surface(gv, gt, 0.5)
        assert s.points.shape == (0, 3) and s.weight.shape == (0,) and s.triangle.shape == (0,)
    # a cell far below what 2^24 cells allow is doubled, and the cell used is returned
    fine = M.build_grid(tv, tt, 1e-3)
    want = R.build_grid(v, t, 1e-3)
    assert fine.cell == want.cell > 1e-3 and fine.dims == want.dims and fine.dims[0] * fine.dims[1] * fine.dims[2] <= 2 ** 24
    same_bytes(H(fine.cell_start), want.cell_start, 'cell_start after doubling')
    same_bytes(H(fine.pair_triangle), want.pair_triangle, 'pair_triangle after doubling')


@pytest.mark.parametrize('name,spacing,k', [('lattice(6)', 2.0, 1), ('lattice(6)', 1.0, 2), ('cube', 0.01, 64), ('soup', 0.3, None), ('icosphere(2)', None, None)])
def test_sample_surface_bit_for_bit(tdgp, name, spacing, k):
    v, t = named_mesh(name)
    want = R.sample_surface(v, t, spacing)
    got = tdgp.mesh_distance.sample_surface(T(v), T(t), spacing)
    if k is not None:
        assert np.bincount(want.triangle).tolist() == [k * k + 3] * len(t)
    same_bytes(H(got.triangle), want.triangle, f'triangle {name} {spacing}')
    same_bytes(H(got.points), want.points, f'points {name} {spacing}')
    same_bytes(H(got.weight), want.weight, f'weight {name} {spacing}')


def test_too_many_samples_are_refused_with_the_spacing_named(tdgp):
    v, t = SR.lattice(130)[:2]                                                                  # 33282 triangles at k = 64: 4099 samples each, more than 2^27
    assert len(t) * 4099 > 2 ** 27
    with pytest.raises(ValueError, match='spacing'):
        tdgp.mesh_distance.sample_surface(T(v), T(t), 1e-6)


def check_stats(got, want, what):
    assert got._fields == ('max', 'mean', 'rms', 'area', 'argmax_sample', 'samples')
    for f in got._fields:
        a, b = getattr(got, f), getattr(want, f)
        assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), f'{what}.{f}: {a!r} vs {b!r}'


def _pairs():
    cube_v, cube_t = CR.CUBE_V, CR.CUBE_T
    ico_v, ico_t = MR.icosphere(2)[:2]
    extra_v = np.concatenate([cube_v, np.array([[3, 0, 0], [3, 0.125, 0], [3, 0, 0.125]], F)])
    extra_t = np.concatenate([cube_t, np.array([[8, 9, 10]], np.int32)])
    return {'cube vs cube + 0.25 x': (cube_v, cube_t, cube_v + np.array([0.25, 0, 0], F), cube_t, 0.25),
            'icosphere(2) vs radius 1.1': (ico_v, ico_t, MR.icosphere(2, radius=1.1)[0], ico_t, 0.2),
            'cube vs cube and a far triangle': (cube_v, cube_t, extra_v, extra_t, 0.25)}


@functools.lru_cache(maxsize=None)
def reference_distance(name):
    va, ta, vb, tb, spacing = _pairs()[name]
    return R.mesh_distance(va, ta, vb, tb, spacing, brute_force=True)


@pytest.mark.parametrize('name', ['cube vs cube + 0.25 x', 'icosphere(2) vs radius 1.1', 'cube vs cube and a far triangle'])
def test_mesh_distance_bit_for_bit(tdgp, name):
    M = tdgp.mesh_distance
    va, ta, vb, tb, spacing = _pairs()[name]
    want = reference_distance(name)
    got = M.mesh_distance(T(va), T(ta), T(vb), T(tb), spacing, return_samples=True)
    print(f'{name}: hausdorff {got.hausdorff!r}, mean {got.mean!r}, rms {got.rms!r}; a -> b max {got.a_to_b.max!r}, b -> a max {got.b_to_a.max!r}')
    check_stats(got.a_to_b, want.a_to_b, name + ' a_to_b')
    check_stats(got.b_to_a, want.b_to_a, name + ' b_to_a')
    assert (got.hausdorff, got.mean, got.rms) == (want.hausdorff, want.mean, want.rms)
    (da, wa), (db, wb) = got.samples
    assert da.shape == wa.shape == (want.a_to_b.samples,) and db.shape == wb.shape == (want.b_to_a.samples,) and da.dtype == torch.float32 and wa.dtype == torch.float64
    assert float(da.max()) == got.a_to_b.max and float(db[got.b_to_a.argmax_sample]) == got.b_to_a.max
    one = M.mesh_distance(T(va), T(ta), T(vb), T(tb), spacing, symmetric=False)
    check_stats(one.a_to_b, want.a_to_b, name + ' one-sided')
    assert one.b_to_a is None and one.samples is None and (one.hausdorff, one.mean, one.rms) == (want.a_to_b.max, want.a_to_b.mean, want.a_to_b.rms)
    stats = M.one_sided(M.sample_surface(T(va), T(ta), spacing), M.build_grid(T(vb), T(tb), 10.0))                         # another grid, the same bits
    check_stats(stats, want.a_to_b, name + ' one_sided')
    if name == 'cube vs cube + 0.25 x':
        assert got.hausdorff == 0.25 and got.a_to_b.samples == 468 and abs(got.a_to_b.area - 6.0) <= 6e-12
    if name == 'cube vs cube and a far triangle':
        assert got.a_to_b.max == 0.0 and got.b_to_a.max == 2.0 and got.hausdorff == 2.0


def test_a_mesh_against_itself_and_a_decimated_one_against_its_source(tdgp):
    M = tdgp.mesh_distance
    v, t = named_mesh('marching cubes')
    tv, tt = T(v), T(t)
    # against itself: exactly 0 where every face is axis-aligned (the flat coordinate of a sample is a + u*0 + v*0: exact)
    for name in ('cube', 'lattice(6)'):
        fv, ft = (T(a) for a in named_mesh(name))
        zero = M.mesh_distance(fv, ft, fv, ft)
        assert zero.hausdorff == 0.0 and zero.mean == 0.0 and zero.rms == 0.0 and zero.a_to_b.max == zero.b_to_a.max == 0.0 and zero.a_to_b.area > 0, name
    # on a general mesh the centroid samples are ROUNDED to fp32 (the contract: the point rounded once), so they leave their own triangle by up
    # to half an ulp per coordinate: sqrt(3)/2 ulp of the largest coordinate bounds the distance (measured: 1.38e-06 of the 1.65e-06 allowed);
    # the vertex samples are exact, and so is the weightless maximum over them
    zero = M.mesh_distance(tv, tt, tv, tt, return_samples=True)
    bound = math.sqrt(3.0) / 2.0 * float(np.spacing(F(np.abs(v).max()))) * (1 + 1e-6)
    print(f'marching cubes against itself: max {zero.hausdorff:.3e}, rms {zero.rms:.3e}, bound {bound:.3e}')
    assert 0.0 <= zero.hausdorff <= bound and zero.a_to_b == zero.b_to_a and zero.a_to_b.area > 0
    assert float(zero.samples[0][0][zero.samples[0][1] == 0].max()) == 0.0
    d = tdgp.mesh_decimate.decimate(tv, tt, target_triangles=len(t) // 4)
    got = M.mesh_distance(d.vertices, d.triangles, tv, tt)
    report_parity(f'speck_volume(24) decimated {len(t)} -> {d.triangles.shape[0]} triangles: sampled two-sided distance to the source (voxels)',
                  hausdorff=got.hausdorff, mean=got.mean, rms=got.rms, decimated_to_source_max=got.a_to_b.max, source_to_decimated_max=got.b_to_a.max,
                  samples=got.a_to_b.samples + got.b_to_a.samples)
    assert all(math.isfinite(x) for x in (got.hausdorff, got.mean, got.rms, got.a_to_b.max, got.b_to_a.max))
    assert got.hausdorff >= max(got.a_to_b.max, got.b_to_a.max)
    per_vertex = M.vertex_distances(d.vertices, M.build_grid(tv, tt))
    colours = M.error_colours(per_vertex.distance, got.hausdorff)
    assert colours.shape == (d.vertices.shape[0], 3) and colours.dtype == torch.float32 and float(colours.min()) >= 0.0 and float(colours.max()) <= 1.0
    named = torch.unique(d.triangles.long())
    assert float(per_vertex.distance[named].max()) <= got.a_to_b.max                              # the vertices triangles name are samples of the decimated mesh


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_distance_gpu_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_two_tools(tdgp, tmp_path, capsys):
    cfg = tdgp.config.config_tiny()
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    ex = _tool('extract_geometry')
    common = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--volume-res', '24', '--cube-size', str(2.0 * cfg.cube_scale), '--thresh-value', '0.0', '--save-ply', '--save-obj',
              '--no-save-mrc']
    ex.main(common + ['--output-dir', str(tmp_path / 'raw')])
    raw_out = capsys.readouterr().out
    ex.main(common + ['--output-dir', str(tmp_path / 'dec'), '--decimate-triangles', '100'])
    dec_out = capsys.readouterr().out
    ex.main(common + ['--output-dir', str(tmp_path / 'rep'), '--decimate-triangles', '100', '--distance-report'])
    rep_out = capsys.readouterr().out
    ex.main(common + ['--output-dir', str(tmp_path / 'raw2'), '--distance-report'])                                        # nothing simplified: nothing to report
    assert capsys.readouterr().out == raw_out
    for a, b in (('dec', 'rep'), ('raw', 'raw2')):                                                                         # the flag changes no output file
        for ext in ('ply', 'obj'):
            for name in ('0000', '0001'):
                assert open(tmp_path / a / f'{name}.{ext}', 'rb').read() == open(tmp_path / b / f'{name}.{ext}', 'rb').read()
    extra = [ln for ln in rep_out.splitlines() if ln not in dec_out.splitlines()]
    assert len(extra) == 2 and [ln for ln in rep_out.splitlines() if ln not in extra] == dec_out.splitlines()
    lines = [json.loads(ln) for ln in extra]
    assert [ln['name'] for ln in lines] == ['0000', '0001']
    for ln in lines:
        assert set(ln['distance']) == {'hausdorff', 'mean', 'rms', 'result_to_full_max', 'full_to_result_max', 'samples'} and ln['triangles'] <= ln['triangles_full']
    shrunk = [ln for ln in lines if ln['triangles'] < ln['triangles_full']]
    assert shrunk and all(0 < ln['distance']['hausdorff'] < float('inf') and ln['triangles'] <= 100 for ln in shrunk)
    line = shrunk[0]
    name = line['name']
    md = _tool('mesh_distance')
    out = md.main([str(tmp_path / 'dec' / f'{name}.obj'), str(tmp_path / 'raw' / f'{name}.ply'), '--json', str(tmp_path / 'd.json'), '--ply', str(tmp_path / 'err.ply')])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    saved = json.load(open(tmp_path / 'd.json'))
    assert printed == saved == json.loads(json.dumps(out))
    assert set(saved) == {'hausdorff', 'mean', 'rms', 'a_to_b', 'b_to_a', 'a', 'b', 'spacing', 'vertex_max'}
    assert set(saved['a_to_b']) == {'max', 'mean', 'rms', 'area', 'argmax_sample', 'samples'} and saved['a']['triangles'] == line['triangles']
    assert saved['hausdorff'] == line['distance']['hausdorff'] and saved['mean'] == line['distance']['mean']             # the files hold the same fp32 meshes
    rv, rt = md.read_mesh(str(tmp_path / 'err.ply'))
    av, at = md.read_mesh(str(tmp_path / 'dec' / f'{name}.ply'))
    assert rv.tobytes() == av.tobytes() and rt.tobytes() == at.tobytes() and b'property uchar red' in open(tmp_path / 'err.ply', 'rb').read(400)
    one = md.main([str(tmp_path / 'dec' / f'{name}.ply'), str(tmp_path / 'raw' / f'{name}.obj'), '--one-sided', '--spacing', '0.05'])
    capsys.readouterr()
    assert one['b_to_a'] is None and one['spacing'] == 0.05 and one['hausdorff'] == one['a_to_b']['max']

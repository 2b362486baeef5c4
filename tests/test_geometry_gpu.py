"""Shape extraction on the GPU: the voxel grid against the reference's (bit for bit), the HIP marching cubes against a numpy marcher driven by
the same table and against the properties of a closed surface, the density grid against the reference's densities, and the whole path."""
import importlib.util
import os

import numpy as np
import pytest

import mc_reference as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gen():
    spec = importlib.util.spec_from_file_location('tool_gen_mc_table', os.path.join(REPO, 'tools', 'gen_mc_table.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def _mc(tdgp, torch, vol, thresh):
    v, t = tdgp.geometry.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), thresh)
    assert v.is_cuda and t.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32 and v.ndim == 2 and t.ndim == 2 and v.shape[1] == 3 and t.shape[1] == 3
    return v.cpu().numpy(), t.cpu().numpy()


def test_voxel_coords_bit_equal_to_the_reference(tdgp, torch_, golden):
    g = golden('geometry')
    origin = g['voxel_origin'].tolist()
    for res in (8, 21):
        got = tdgp.geometry.create_voxel_coords(res, origin, float(g[f'coords_r{res}_cube']), 1)
        assert got.shape == (1, res ** 3, 3)
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), g[f'coords_r{res}'].view(np.uint32)), res
    got = tdgp.geometry.create_voxel_coords(8, origin, float(g['coords_r8_cube']), 3)
    assert got.shape == (3, 512, 3) and all(np.array_equal(got[b].cpu().numpy().view(np.uint32), g['coords_r8'].view(np.uint32)) for b in range(3))
    res, i0, n = (int(x) for x in g['strip_spec'])
    assert i0 > 2 ** 24                                   # the strip lies where the index is no longer exact in fp32
    full = tdgp.geometry.create_voxel_coords(res, origin, float(g['strip_cube']), 1)
    assert np.array_equal(full[0, i0:i0 + n].cpu().numpy().view(np.uint32), g['strip_coords'].view(np.uint32))
    # the slab form (tdgp_voxel_coords from an offset) writes the same values as the whole grid
    part = torch_.empty([n, 3], dtype=torch_.float32, device='cuda')
    tdgp.geometry._voxel_coords_into(part, i0, res, tdgp.geometry._grid_constants(res, origin, float(g['strip_cube'])))
    assert np.array_equal(part.cpu().numpy().view(np.uint32), g['strip_coords'].view(np.uint32))


SMALL_VOLUMES = {
    'sphere': lambda: (R.sphere(12, 4.2), 0.0),
    'torus': lambda: (R.torus((9, 12, 12), 3.4, 1.6), 0.0),
    'noise': lambda: (np.random.RandomState(11).rand(11, 12, 10).astype(np.float32), 0.5),
    'noise_5_9_17': lambda: (np.random.RandomState(12).rand(5, 9, 17).astype(np.float32), 0.45),
}


@pytest.mark.parametrize('name', sorted(SMALL_VOLUMES))
def test_marching_cubes_equals_the_numpy_marcher(tdgp, torch_, gen, name):
    vol, thresh = SMALL_VOLUMES[name]()
    verts, tris = _mc(tdgp, torch_, vol, thresh)
    ids = R.crossing_edge_ids(vol, thresh)
    assert len(verts) == len(ids) and len(ids) > 0
    want = R.marcher(vol, thresh, gen.table(), gen.edge_info)
    assert tris.min() >= 0 and tris.max() < len(ids)
    got = ids[tris]                                       # vertex order is documented: ascending (owning grid point, axis)
    assert np.array_equal(R.canonical(got), R.canonical(want))
    assert np.array_equal(got, want)                      # and the triangle order: by cell, then table order
    ref = R.edge_vertices(vol, thresh, ids)
    ulp = np.spacing(np.maximum(np.abs(ref), 1.0).astype(np.float32))
    worst = float((np.abs(verts.astype(np.float64) - ref.astype(np.float64)) / ulp).max())
    print(f'{name}: V={len(verts)} T={len(tris)} worst vertex distance {worst:.2f} ulp')
    assert worst <= 4.0, worst
    # on its edge: the two other coordinates are the grid point's, exactly
    pt, axis = ids // 3, ids % 3
    p = np.stack(np.unravel_index(pt, vol.shape), 1).astype(np.float32)
    for a in range(3):
        assert np.array_equal(verts[axis != a, a], p[axis != a, a])
    t = verts[np.arange(len(ids)), axis] - p[np.arange(len(ids)), axis]
    assert (t >= 0).all() and (t <= 1).all()


@pytest.mark.parametrize('shape,seed', [((64, 64, 64), 1), ((96, 80, 72), 2)])
def test_marching_cubes_properties_at_size(tdgp, torch_, shape, seed):
    vol = R.smooth_noise(shape, seed)
    thresh = float(np.median(vol))
    vol[[0, -1]] = vol[:, [0, -1]] = vol[:, :, [0, -1]] = vol.min() - 1.0
    verts, tris = _mc(tdgp, torch_, vol, thresh)
    assert len(verts) == R.count_crossing_edges(vol, thresh)
    assert np.array_equal(np.unique(tris), np.arange(len(verts)))
    R.assert_closed_oriented(tris)                        # every case that occurs takes part: nothing is excluded
    assert R.signed_volume(verts, tris) > 0
    ids = R.crossing_edge_ids(vol, thresh)
    assert float(np.abs(verts - R.edge_vertices(vol, thresh, ids)).max()) <= 1e-5
    print(f'{shape}: V={len(verts)} T={len(tris)}')


def test_marching_cubes_euler_characteristic_and_orientation(tdgp, torch_):
    for name, vol, chi in (('sphere', R.sphere(48, 17.3), 2), ('torus', R.torus((40, 64, 64), 18.2, 7.1), 0)):
        verts, tris = _mc(tdgp, torch_, vol, 0.0)
        E = R.assert_closed_oriented(tris)
        assert len(verts) - E + len(tris) == chi, name
        vol_mesh, vol_cells = R.signed_volume(verts, tris), float((vol >= 0).sum())
        assert vol_mesh > 0 and abs(vol_mesh - vol_cells) < 0.05 * vol_cells, (name, vol_mesh, vol_cells)


def test_marching_cubes_is_deterministic(tdgp, torch_):
    vol = torch_.from_numpy(R.smooth_noise((64, 48, 56), 4)).cuda()
    thresh = float(vol.median())
    a, b = tdgp.geometry.marching_cubes(vol, thresh), tdgp.geometry.marching_cubes(vol, thresh)
    assert a[0].shape[0] > 1000
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def test_marching_cubes_edge_shapes(tdgp, torch_, gen):
    torch = torch_
    mc = tdgp.geometry.marching_cubes
    for fill in (0.0, 1.0):                               # all below / all above
        v, t = mc(torch.full([6, 7, 8], fill, device='cuda'), 0.5)
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda
    for shape in ([1, 5, 5], [5, 1, 5], [5, 5, 1]):       # a side below 2: no cell
        v, t = mc(torch.rand(shape, device='cuda'), 0.5)
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3)
    one = np.zeros([2, 2, 2], np.float32)
    one[1, 0, 1] = 1.0
    v, t = _mc(tdgp, torch, one, 0.25)
    assert v.shape == (3, 3) and t.shape == (1, 3)
    ids = R.crossing_edge_ids(one, 0.25)
    assert np.array_equal(ids[t], R.marcher(one, 0.25, gen.table(), gen.edge_info))
    assert np.allclose(v, R.edge_vertices(one, 0.25, ids), atol=1e-6) and R.signed_volume(v - np.array([1, 0, 1], np.float32), t) > 0
    # a non-contiguous cropped view is marched as its contiguous copy
    big = torch.from_numpy(R.smooth_noise((20, 24, 28), 7)).cuda()
    view = big[3:-2, 12:, :-9]
    assert not view.is_contiguous()
    thresh = float(view.median())
    a, b = mc(view, thresh), mc(view.contiguous(), thresh)
    assert a[0].shape[0] > 0 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    vn, tn = a[0].cpu().numpy(), a[1].cpu().numpy()
    volc = view.contiguous().cpu().numpy()
    assert np.array_equal(R.crossing_edge_ids(volc, thresh)[tn], R.marcher(volc, thresh, gen.table(), gen.edge_info)) and len(vn) == R.count_crossing_edges(volc, thresh)


@pytest.fixture(scope='module')
def golden_generator(tdgp, torch_, golden):
    g = golden('geometry')
    cfg = tdgp.config.config_tiny()
    sd = tdgp.weights.random_state_dict(cfg, seed=int(g['seed'][0]), exercise_all=True)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(sd)
    return g, G.to('cuda').eval(), torch_.from_numpy(g['ws']).cuda()


def test_density_grid_against_the_reference(tdgp, torch_, golden_generator):
    """Held to the reference's own figures: the reference's fp32 densities are `r` of the range from its own float64 run; ours may be at most
    2 r (maximum) and 1.5 x its 99.9th percentile from the reference's fp32 grid."""
    g, G, ws = golden_generator
    res, cube, origin = int(g['density_spec'][0]), float(g['density_cube']), g['voxel_origin'].tolist()
    got = tdgp.geometry.density_grid(G, ws, res, origin, cube)
    assert tuple(got.shape) == (1, res, res, res) and got.dtype == torch_.float32
    ours, ref, f64 = got[0].cpu().numpy().astype(np.float64), g['sigma'].astype(np.float64), g['sigma_f64']
    rng = np.abs(ref).max()
    e_ours, e_ref = np.abs(ours - ref) / rng, np.abs(ref - f64) / rng
    figs = dict(range_err_max=e_ours.max(), reference_fp32_vs_f64_max=e_ref.max(), ratio_max=e_ours.max() / e_ref.max(),
                p999=np.quantile(e_ours, 0.999), reference_p999=np.quantile(e_ref, 0.999), ratio_p999=np.quantile(e_ours, 0.999) / np.quantile(e_ref, 0.999),
                ours_vs_f64_max=(np.abs(ours - f64) / rng).max())
    __import__('conftest').report_parity('density_grid (geometry golden, res 32) vs the reference fp32 densities', **figs)
    print(figs)
    assert e_ours.max() <= 2.0 * e_ref.max(), figs
    assert np.quantile(e_ours, 0.999) <= 1.5 * np.quantile(e_ref, 0.999), figs
    # slab size does not change a bit, and the slabs reproduce the one-call path
    small = tdgp.geometry.density_grid(G, ws, res, origin, cube, slab_points=4096)
    assert torch_.equal(small, got)
    coords = tdgp.geometry.create_voxel_coords(res, origin, cube, 1)
    whole = G.synthesis.compute_densities(ws, coords, noise_mode='const')
    assert tuple(whole.shape) == (1, res ** 3, 1) and torch_.equal(whole.reshape(1, res, res, res), got)


def test_extract_geometry_end_to_end(tdgp, torch_, golden_generator, tmp_path):
    g, G, ws = golden_generator
    res, cube, origin = int(g['density_spec'][0]), float(g['density_cube']), g['voxel_origin'].tolist()
    thresh = float(np.median(tdgp.geometry.density_grid(G, ws, res, origin, cube).cpu().numpy()))
    shapes = tdgp.geometry.extract_geometry(G, ws, volume_res=res, voxel_origin=origin, cube_size=cube, thresh_value=thresh, crop='reference', normalize=True)
    assert len(shapes) == 1
    s = shapes[0]
    sigma = s.sigma.cpu().numpy()
    assert sigma.shape == np.zeros([res] * 3)[tdgp.geometry.crop_reference(res)].shape
    V, T = s.vertices.shape[0], s.triangles.shape[0]
    assert V > 0 and T > 0 and V == R.count_crossing_edges(sigma, thresh)
    v = s.vertices.cpu().numpy().astype(np.float64)
    diag = float(np.sqrt(((v.max(0) - v.min(0)) ** 2).sum()))
    assert abs(diag - 1.0) <= 4 * np.finfo(np.float32).eps, diag
    raw = tdgp.geometry.extract_geometry(G, ws, volume_res=res, voxel_origin=origin, cube_size=cube, thresh_value=thresh, crop=None, normalize=False)[0]
    assert tuple(raw.sigma.shape) == (res, res, res) and raw.vertices.shape[0] == R.count_crossing_edges(raw.sigma.cpu().numpy(), thresh)
    assert float(raw.vertices.max()) <= res - 1 and float(raw.vertices.min()) >= 0
    tdgp.geometry.save_ply(tmp_path / 's.ply', s.vertices, s.triangles)
    pv, pf = __import__('test_geometry').parse_ply(tmp_path / 's.ply')
    assert np.array_equal(pv.view(np.uint32), s.vertices.cpu().numpy().view(np.uint32)) and np.array_equal(pf, s.triangles.cpu().numpy())

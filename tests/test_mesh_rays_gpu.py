"""Mesh rays on the GPU: tdgp_mesh_rays_cast / tdgp_mesh_rays_ao and the drivers of 3dgp_amd/mesh_rays.py bit for bit against the restatement
of their contract (tests/mesh_rays_reference.py, whose walk and scan tests/test_mesh_rays.py holds against each other): first hits by the
walk and by the scan at three cell sizes per mesh (identical across them: what an unsound traversal would break), the block edges of the
one-wave launch, rays that are no rays, empty grids, any-hit and segments, ambient occlusion at every lane-group width, the rasteriser of
mesh frames against the same camera rays, and occlusion in the frames, the extraction and the two command lines."""
import functools
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_components_reference as CR
import mesh_distance_reference as MD
import mesh_raster_reference as MR
import mesh_rays_reference as R
import mesh_surface_reference as SR
from conftest import report_parity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F, D = np.float32, np.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


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


# name -> (mesh, the three cell sizes: the last one gives a 1 x 1 x 1 grid): those of tests/test_mesh_distance_gpu.py
MESHES = {
    'icosphere(2)': (lambda: MR.icosphere(2)[:2], (0.25, 0.7, 1e6)),
    'cube': (lambda: (CR.CUBE_V, CR.CUBE_T), (0.125, 0.5, 1e6)),
    'lattice(6)': (lambda: SR.lattice(6)[:2], (0.5, 1.5, 1e6)),
    'marching cubes': (_mc_mesh, (1.0, 3.0, 1e6)),
    'soup': (lambda: MD.soup(120, seed=7), (0.4, 1.25, 1e6)),
}


@functools.lru_cache(maxsize=None)
def named_mesh(name):
    v, t = MESHES[name][0]()
    v, t = np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32)
    for a in (v, t):
        a.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def reference_grid(name, k=0):
    v, t = named_mesh(name)
    return MD.build_grid(v, t, MESHES[name][1][k])


@functools.lru_cache(maxsize=None)
def reference_rays(name):
    """257 rays (an ordinary one, a NaN origin, an infinite direction, a zero direction, then the adversarial set of the CPU tests) and the
    restatement's scan over all triangles for them: computed once, shared, never written."""
    grid = reference_grid(name)
    o, d = R.adversarial_rays(grid, seed=11)
    bad_o = np.array([[np.nan, 0, 0], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3]], F)
    bad_d = np.array([[0, 0, 1], [0, -np.inf, 1], [0, 0, 0]], F)
    o, d = np.concatenate([o[:1], bad_o, o[1:]])[:257], np.concatenate([d[:1], bad_d, d[1:]])[:257]
    want = R.scan_rays(o, d, grid)
    for a in (o, d) + tuple(want):
        a.setflags(write=False)
    return o, d, want


def check_hits(got, want, what, n=None):
    assert got._fields == ('t', 'depth', 'triangle', 'bary', 'side')
    for f in got._fields:
        same_bytes(H(getattr(got, f)), getattr(want, f)[:n], f'{f} {what}')


@pytest.mark.parametrize('name', list(MESHES))
def test_first_hits_bit_for_bit(tdgp, name):
    M, G = tdgp.mesh_rays, tdgp.mesh_distance
    v, t = named_mesh(name)
    o, d, want = reference_rays(name)
    tv, tt, to, td = T(v), T(t), T(o), T(d)
    assert np.isnan(want.t[1:4]).all() and (want.triangle[1:4] == -1).all() and (want.side[1:4] == 0).all() and not np.isnan(want.t[4:]).any()
    hit = want.triangle >= 0
    assert 40 <= hit.sum() <= 245 and np.isinf(want.t[4:][~hit[4:]]).all()
    for cell in MESHES[name][1]:
        grid = G.build_grid(tv, tt, cell)
        got, evaluated = M.first_hits(to, td, grid, return_evaluated=True)
        check_hits(got, want, f'{name} cell {cell} walk')                                            # identical across the cell sizes
        assert evaluated.dtype == torch.int32 and evaluated.shape == (257,) and int(evaluated[1:4].sum()) == 0
        print(f'{name}: grid {grid.dims}, {grid.pair_triangle.shape[0]} pairs, {float(evaluated.float().mean()):.1f} triangles evaluated per ray of {grid.valid_count}')
        same_bytes(H(M.occluded(to, td, grid)), hit.astype(np.uint8), f'occluded {name} cell {cell}')
    assert grid.dims == (1, 1, 1)
    fine = G.build_grid(tv, tt, MESHES[name][1][0])
    got, evaluated = M.first_hits(to, td, fine, brute_force=True, return_evaluated=True)
    check_hits(got, want, f'{name} scan')
    assert evaluated[4:].unique().tolist() == [fine.valid_count]
    check_hits(M.first_hits(to, td, G.build_grid(tv, tt)), want, f'{name} default cell walk')
    mid = float(np.median(want.t[hit & (want.t > 0)]))
    for window in ((0.0, mid), (mid, np.inf), (0.5 * mid, 1.5 * mid)):
        cut = R.scan_rays(o, d, reference_grid(name), *window)
        check_hits(M.first_hits(to, td, fine, *window), cut, f'{name} window {window} walk')
        check_hits(M.first_hits(to, td, fine, *window, brute_force=True), cut, f'{name} window {window} scan')
        same_bytes(H(M.occluded(to, td, fine, *window)), (cut.triangle >= 0).astype(np.uint8), f'occluded {name} window {window}')


@pytest.mark.parametrize('n', COUNTS)
def test_ray_counts_at_the_block_edges(tdgp, n):
    M = tdgp.mesh_rays
    v, t = named_mesh('icosphere(2)')
    o, d, want = reference_rays('icosphere(2)')
    grid = tdgp.mesh_distance.build_grid(T(v), T(t), 0.25)
    to, td = T(o[:n].copy()).reshape(n, 3), T(d[:n].copy()).reshape(n, 3)
    for brute in (False, True):
        got = M.first_hits(to, td, grid, brute_force=brute)
        assert got.t.shape == (n,) and got.bary.shape == (n, 2) and got.side.dtype == torch.int8
        check_hits(got, want, f'N = {n} brute_force = {brute}', n)
    same_bytes(H(M.occluded(to, td, grid)), (want.triangle[:n] >= 0).astype(np.uint8), f'occluded N = {n}')


def test_grids_without_triangles_and_two_runs(tdgp):
    M, G = tdgp.mesh_rays, tdgp.mesh_distance
    v, t = named_mesh('marching cubes')
    o, d, want = reference_rays('marching cubes')
    tv, tt, to, td = T(v), T(t), T(o), T(d)
    none_t = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    sv, st = named_mesh('soup')
    bad = np.isnan(want.t)
    for what, (gv, gt) in (('T = 0', (tv, none_t)), ('all invalid', (T(sv), T(st[12:16].copy()))), ('V = 0', (torch.zeros(0, 3, device=DEV), none_t))):
        g = G.build_grid(gv, gt)
        assert g.valid_count == 0
        for brute in (False, True):
            h = M.first_hits(to, td, g, brute_force=brute)
            check_hits(h, R.scan_rays(o, d, MD.build_grid(H(gv), H(gt))), what)
            assert torch.isinf(h.t[~T(bad)]).all() and (h.triangle == -1).all() and (h.side == 0).all() and torch.isnan(h.bary).all()
        assert int(M.occluded(to, td, g).sum()) == 0
        assert torch.equal(M.ambient_occlusion(to[4:9], td[4:9], g), torch.ones(5, device=DEV))
    grid = G.build_grid(tv, tt, 1.0)
    a, b = M.first_hits(to, td, grid), M.first_hits(to, td, grid)
    assert all(H(x).tobytes() == H(y).tobytes() for x, y in zip(a, b))


def test_occluded_and_segment_visible(tdgp):
    M = tdgp.mesh_rays
    v, t = named_mesh('cube')
    grid = tdgp.mesh_distance.build_grid(T(v), T(t), 0.125)
    rs = np.random.RandomState(2)
    uv = rs.rand(40, 2).astype(F)
    low = np.concatenate([uv, np.zeros((40, 1), F)], 1)                                           # on the face z = 0
    high = np.concatenate([uv[::-1], np.ones((40, 1), F)], 1)                                     # on the face z = 1
    inside = M.segment_visible(T(low), T(high), grid)                                             # through the inside: nothing between the faces
    assert inside.dtype == torch.uint8 and bool(inside.all())
    assert not bool(M.segment_visible(T(low), T(high), grid, bias=0.0).any())                      # without the bias both ends touch
    below, above = low - np.array([0, 0, 0.5], F), high + np.array([0, 0, 0.5], F)
    assert not bool(M.segment_visible(T(below), T(above), grid).any())                             # through the whole cube
    side = np.concatenate([np.full((40, 1), 1.5, F), uv[:, :1], -0.01 - uv[:, 1:]], 1).astype(F)    # beside the cube and below its floor: the segment stays under it
    assert bool(M.segment_visible(T(below), T(side), grid).all())                                  # round it
    same_bytes(H(M.segment_visible(T(below), T(above), grid)), 1 - R.occluded(below, (above - below).astype(F), reference_grid('cube'), 1e-4, 1.0 - 1e-4), 'segments')
    assert bool(M.segment_visible(T(low), T(low), grid).all())                                     # p == q: no ray, visible


@functools.lru_cache(maxsize=None)
def occlusion_points():
    """65 points on and round icosphere(2): its vertices pushed in and out, two of them spoilt."""
    v, _ = named_mesh('icosphere(2)')
    rs = np.random.RandomState(6)
    p = (v[:65] * (0.55 + 0.6 * rs.rand(65, 1))).astype(F)
    n = (v[:65] * np.where(rs.rand(65, 1) < 0.5, -1.0, 1.0) + 0.4 * rs.randn(65, 3)).astype(F)
    p[7, 2], n[11] = np.nan, 0.0
    for a in (p, n):
        a.setflags(write=False)
    return p, n


@pytest.mark.parametrize('rays', (16, 32, 64))
@pytest.mark.parametrize('rotations', (1, 16))
def test_ambient_occlusion_bit_for_bit(tdgp, rays, rotations):
    M = tdgp.mesh_rays
    v, t = named_mesh('icosphere(2)')
    p, n = occlusion_points()
    grid = tdgp.mesh_distance.build_grid(T(v), T(t), 0.25)
    tables = M.ao_tables(rays, rotations)
    same_bytes(H(tables), R.ao_tables(rays, rotations), 'tables')
    bias = float(F(1e-3) * F(grid.cell))
    for radius in (None, 0.6):
        want = R.ambient_occlusion(p, n, reference_grid('icosphere(2)'), R.ao_tables(rays, rotations), bias, np.inf if radius is None else radius)
        assert np.isnan(want[[7, 11]]).all() and not np.isnan(np.delete(want, [7, 11])).any() and 0 < np.nanmean(want) < 1 and len(np.unique(want[~np.isnan(want)])) > 4
        for count in (0, 1, 3, 4, 5, 63, 64, 65):                                                   # the lane-group edges of a wave
            got = M.ambient_occlusion(T(p[:count].copy()).reshape(count, 3), T(n[:count].copy()).reshape(count, 3), grid, rays, radius, None, rotations, tables=tables)
            same_bytes(H(got), want[:count], f'{rays} rays, {rotations} tables, radius {radius}, N = {count}')
        again = M.ambient_occlusion(T(p), T(n), grid, rays, radius, bias, rotations)
        assert H(again).tobytes() == H(got).tobytes()                                             # the same bytes on every run, bias given or derived
    print(f'{rays} rays, {rotations} tables: mean occlusion {np.nanmean(want):.4f} within 0.6')


def test_ambient_occlusion_of_the_sphere_is_exact(tdgp):
    M = tdgp.mesh_rays
    v, t = named_mesh('icosphere(2)')
    tv, tt = T(v), T(t)
    grid = tdgp.mesh_distance.build_grid(tv, tt, 0.25)
    for rays in (16, 32, 64):
        assert torch.equal(M.ambient_occlusion(tv, tv, grid, rays), torch.ones(len(v), device=DEV))              # convex, outward normals
        assert torch.equal(M.ambient_occlusion(tv, -tv, grid, rays), torch.zeros(len(v), device=DEV))            # closed, inward normals
    ao = M.vertex_occlusion(tv, tt, rays=32)
    assert ao.shape == (len(v),) and torch.equal(ao, torch.ones(len(v), device=DEV))
    lone = torch.cat([tv, torch.tensor([[5.0, 5.0, 5.0]], device=DEV)])                                          # a vertex no triangle names: NaN -> 1
    assert torch.equal(M.vertex_occlusion(lone, tt, rays=16), torch.ones(len(v) + 1, device=DEV))
    # the winding reversed: the vertex normals point inward, and the mesh is closed
    inward = M.vertex_occlusion(tv, tt.flip(1).contiguous(), rays=64)
    assert torch.equal(inward, torch.zeros(len(v), device=DEV))


def cameras(tdgp, n=2):
    angles = np.array([[0.3, 1.3, 0.0], [-0.5, 1.8, 0.0], [1.1, 1.5, 0.0]], F)[:n]
    return tdgp.generator.TensorGroup(angles=T(angles), fov=T(np.array([40.0, 50.0, 60.0], F)[:n]), radius=T(np.array([1.0, 1.1, 0.9], F)[:n]),
                                      look_at=T(np.zeros((n, 3), F)))


def test_the_rasteriser_against_the_rays(tdgp):
    """icosphere(1) under two cameras at 128 x 128: the camera rays of renderer.sample_rays through first_hits against the status / tri / depth
    of render_mesh_views.  (status, tri) agree on at least 98 % of the pixels (the rasteriser snaps to 1/256 pixel: only pixels whose centre
    lies within that of an edge may differ); where they agree the depths differ by at most twice what the two numpy restatements show on the
    same pixels."""
    res = 128
    v, t = MR.icosphere(1, 0.3)
    tv, tt = T(v), T(t)
    cams = cameras(tdgp)
    frames = tdgp.mesh.render_mesh_views(tv, tt, cams, res)
    c2w = tdgp.renderer.compute_cam2world_matrix(cams)
    focal = tdgp.mesh.focal_lengths(cams.fov, 2, DEV)
    ray_o, ray_d = tdgp.renderer.sample_rays(c2w, fov=cams.fov, resolution=(res, res))
    o, d = ray_o.reshape(-1, 3).contiguous(), ray_d.reshape(-1, 3).contiguous()
    grid = tdgp.mesh_distance.build_grid(tv, tt)
    hits = tdgp.mesh_rays.first_hits(o, d, grid)
    want = R.scan_rays(H(o), H(d), MD.build_grid(v, t))
    check_hits(hits, want, 'camera rays')
    raster = MR.frames(v, t, H(c2w), H(focal), H(o), H(d), res, res, 1e-3, 'none', 0.0, 0.0)
    status, tri, depth = H(frames.status).reshape(-1), H(frames.tri).reshape(-1), H(frames.depth).reshape(-1)
    cast = (want.triangle >= 0).astype(np.int32)
    agree = (status == cast) & (tri == want.triangle)
    cpu_agree = (raster['status'] == cast) & (raster['tri'] == want.triangle)
    both, cpu_both = agree & (cast == 1), cpu_agree & (cast == 1)
    diff = np.abs(depth[both].astype(D) - H(hits.depth)[both].astype(D)).max()
    cpu_diff = np.abs(raster['t_hit'][cpu_both].astype(D) - want.depth[cpu_both].astype(D)).max()
    report_parity('icosphere(1) at 128 x 128 under 2 cameras: render_mesh_views against first_hits on the same rays', pixels=agree.size, differ=int((~agree).sum()),
                  hit_share=float(cast.mean()), depth_diff_max=float(diff), restatements_differ=int((~cpu_agree).sum()), restatements_depth_diff_max=float(cpu_diff))
    print(f'{(~agree).sum()} of {agree.size} pixels differ ({(~cpu_agree).sum()} between the restatements); depth differs by {diff:.3e} at most ({cpu_diff:.3e})')
    assert cast.mean() > 0.1 and agree.mean() >= 0.98
    assert diff <= 2 * cpu_diff


# ------------------------------------------------------------------------------------------------ occlusion in the frames, the extraction, the tools
def test_render_mesh_views_with_vertex_occlusion(tdgp):
    """icosphere(1) at 64 x 64: the frames with `vertex_occlusion` against the numpy restatement of the raster path fed the multiplied colours, in
    colour mode and in shaded mode (albedo * occlusion through the colour path); without the argument not a byte changes."""
    Me = tdgp.mesh
    res = 64
    v, t = MR.icosphere(1, 0.3)
    tv, tt = T(v), T(t)
    cams = cameras(tdgp)
    rs = np.random.RandomState(9)
    rgbv, occ = rs.rand(len(v), 3).astype(F), rs.rand(len(v)).astype(F)
    shade = dict(ambient=0.25, albedo=(0.9, 0.7, 0.5), background=(1.0, 0.5, -1.0))
    c2w = tdgp.renderer.compute_cam2world_matrix(cams)
    focal = Me.focal_lengths(cams.fov, 2, DEV)
    ray_o, ray_d = tdgp.renderer.sample_rays(c2w, fov=cams.fov, resolution=(res, res))
    args = (v, t, H(c2w), H(focal), H(ray_o).reshape(-1, 3), H(ray_d).reshape(-1, 3), res, res, 1e-3, 'none', 0.0, 0.0)
    for mode, base in (('colour', rgbv), ('shaded', np.asarray(shade['albedo'], F)[None, :])):
        want = MR.frames(*args, vertex_rgb=(base * occ[:, None]).astype(F), mode='colour', **shade)
        kw = dict(vertex_colours=T(rgbv)) if mode == 'colour' else {}
        got = Me.render_mesh_views(tv, tt, cams, res, mode=mode, vertex_occlusion=T(occ), **kw, **shade)
        same_bytes(H(got.rgb).reshape(-1, 3), want['rgb'], f'rgb {mode} with occlusion')
        same_bytes(H(got.status).reshape(-1), want['status'], f'status {mode}')
        plain = MR.frames(*args, vertex_rgb=rgbv if mode == 'colour' else None, mode=mode, **shade)
        same_bytes(H(Me.render_mesh_views(tv, tt, cams, res, mode=mode, **kw, **shade).rgb).reshape(-1, 3), plain['rgb'], f'rgb {mode} without it')
        assert (want['rgb'] != plain['rgb']).any()
        ones = Me.render_mesh_views(tv, tt, cams, res, mode=mode, vertex_occlusion=torch.ones(len(v), device=DEV), **kw, **shade)
        if mode == 'colour':
            same_bytes(H(ones.rgb).reshape(-1, 3), plain['rgb'], 'an occlusion of 1 changes nothing in colour mode')
    ms = Me.render_mesh_views(tv, tt, cams, res, vertex_occlusion=T(occ), samples=4)
    assert ms.rgb.shape == (2, res * res, 3) and ms.coverage.shape == (2, res * res)
    for bad in (dict(mode='normals'), dict(normals='field'), dict(vertex_occlusion=T(occ[:-1].copy())), dict(vertex_occlusion=T(occ.astype(D))),
                dict(vertex_occlusion=torch.as_tensor(occ))):
        with pytest.raises(ValueError, match='vertex_occlusion'):
            Me.render_mesh_views(tv, tt, cams, res, **{**dict(vertex_occlusion=T(occ)), **bad})


B, NV, VOL = 2, 3, 24


@pytest.fixture(scope='module')
def scene(tdgp):
    """config_tiny, seeded weights, 2 samples x 3 cameras, volume_res 24 over the whole field, the level at the grid's median."""
    cfg = tdgp.config.config_tiny()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    G = G.to(DEV).eval()
    inp = tdgp.weights.synthetic_inputs(cfg, batch=B, seed=12)
    ws = G.mapping(T(inp['z']), T(inp['c']))
    cam_np = tdgp.weights.synthetic_inputs(cfg, batch=B * NV, seed=13)['camera']
    cams = tdgp.generator.TensorGroup(**{k: T(v) for k, v in cam_np.items()})
    box = 2.0 * cfg.cube_scale
    with torch.no_grad():
        grid = tdgp.geometry.density_grid(G, ws, volume_res=VOL, cube_size=box)
    return dict(G=G, ws=ws, cams=cams, level=float(grid.median()), box=box, res=G.synthesis.test_resolution)


def test_frames_and_extraction_with_occlusion(tdgp, scene):
    g, Me, M = tdgp.geometry, tdgp.mesh, tdgp.mesh_rays
    sc = scene
    G, res = sc['G'], sc['res']
    kw = dict(level=sc['level'], volume_res=VOL)
    opts = dict(rays=16, radius=0.5 * sc['box'])
    flat = Me.render_mesh_frames(G, sc['ws'], sc['cams'], **kw)
    none = Me.render_mesh_frames(G, sc['ws'], sc['cams'], ao=None, **kw)
    frames, counts = Me.render_mesh_frames(G, sc['ws'], sc['cams'], ao=opts, smooth=dict(iterations=2), return_counts=True, **kw)
    for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
        assert torch.equal(getattr(flat, k), getattr(none, k)), k
    ekw = dict(volume_res=VOL, cube_size=sc['box'], thresh_value=sc['level'], crop=None, normalize=False)
    plain = g.extract_geometry(G, sc['ws'], smooth=dict(iterations=2), units='world', **ekw)
    shapes = g.extract_geometry(G, sc['ws'], smooth=dict(iterations=2), units='world', ao=opts, **ekw)
    index = g.extract_geometry(G, sc['ws'], smooth=dict(iterations=2), ao=opts, **ekw)
    planes = G.synthesis.tri_planes(sc['ws'], noise_mode='const')
    stages = tdgp.mesh_build.check_stages(None, dict(iterations=2), None, None, ao=opts)
    seen = 0
    for b in range(B):
        s = shapes[b]
        assert type(s).__name__ == 'OccludedShape' and s.texture is None and type(plain[b]).__name__ == 'Shape'
        assert torch.equal(s.vertices, plain[b].vertices) and torch.equal(s.triangles, plain[b].triangles) and torch.equal(s.sigma, plain[b].sigma)
        want = M.vertex_occlusion(s.vertices, s.triangles, **opts)                                # on the finished world-space mesh, after every other stage
        assert torch.equal(s.occlusion, want) and torch.equal(index[b].occlusion, want) and s.occlusion.shape == (s.vertices.shape[0],)
        assert float(want.min()) >= 0.0 and float(want.max()) <= 1.0
        seen += int((want < 1).sum())
        # the frames build their mesh from the planes of the whole batch: the same build on those planes, then the views with its occlusion
        m = tdgp.mesh_build.build_mesh(G, tdgp.renderer.HWCPlanes(planes.t[b:b + 1]), stages, volume_res=VOL, voxel_origin=(0.0, 0.0, 0.0), cube_size=sc['box'],
                                       level=sc['level'], crop_slices=None, sheared=True, keep_grid=False)
        assert m.sigma is None and torch.equal(m.occlusion, M.vertex_occlusion(m.world, m.triangles, **opts))
        cams = Me._camera_slice(sc['cams'], DEV, b * NV, (b + 1) * NV)
        views = Me.render_mesh_views(m.world, m.triangles, cams, res, G=G, vertex_occlusion=m.occlusion)
        for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
            assert torch.equal(getattr(frames, k)[b * NV:(b + 1) * NV], getattr(views, k)), (b, k)
        assert counts[b] == m.count == (m.world.shape[0], m.triangles.shape[0])
    print(f'{seen} vertices of the two tiny shapes are occluded within {opts["radius"]:.3f}')
    grid = Me.render_mesh_video_grid(G, sc['ws'], sc['cams'], ao=opts, **kw)                                               # passed through **kw
    strips = Me.render_mesh_strips(G, sc['ws'], sc['cams'], ao=opts, **kw)
    assert grid.dtype == torch.uint8 and grid.shape[0] == NV and strips.dtype == torch.uint8 and strips.shape[0] == B
    for bad in (dict(ao=dict(rays=20)), dict(ao=dict(rays=16, reach=1.0)), dict(ao=dict(rays=16, radius=0.0)), dict(ao=opts, mode='normals'), dict(ao=opts, normals='field'),
                dict(ao=opts, texture=dict(texels=4), mode='colour')):
        with pytest.raises(ValueError):
            Me.render_mesh_frames(G, sc['ws'], sc['cams'], **{**kw, **bad})
    st = tdgp.mesh_build.check_stages(None, None, None, None, ao=dict(rays=64))
    assert st.ao == dict(rays=64, radius=None, bias=None) and st == (None, None, None, None, 'bilinear', None) and tdgp.mesh_build.check_stages(None, None, None, None).ao is None


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_rays_gpu_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_two_command_lines(tdgp, tmp_path, capsys):
    cfg = tdgp.config.config_tiny()
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    ex = _tool('extract_geometry')
    common = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--volume-res', '24', '--cube-size', str(2.0 * cfg.cube_scale), '--thresh-value', '0.0', '--save-ply', '--save-obj',
              '--no-save-mrc']
    ex.main(common + ['--output-dir', str(tmp_path / 'raw')])
    raw_out = capsys.readouterr().out
    ex.main(common + ['--output-dir', str(tmp_path / 'raw2')])
    assert capsys.readouterr().out == raw_out
    ex.main(common + ['--output-dir', str(tmp_path / 'ao'), '--ao-rays', '16'])
    ao_out = capsys.readouterr().out
    extra = [json.loads(ln) for ln in ao_out.splitlines() if ln not in raw_out.splitlines()]
    assert [ln['name'] for ln in extra] == ['0000', '0001'] and all(ln['ao_rays'] == 16 for ln in extra)
    md = _tool('mesh_distance')
    for name in ('0000', '0001'):
        raw_ply, ao_ply = (open(tmp_path / d / f'{name}.ply', 'rb').read() for d in ('raw', 'ao'))
        assert raw_ply == open(tmp_path / 'raw2' / f'{name}.ply', 'rb').read()                     # without the flag: the same bytes
        assert open(tmp_path / 'raw' / f'{name}.obj', 'rb').read() == open(tmp_path / 'ao' / f'{name}.obj', 'rb').read()      # the flag moves no vertex
        assert b'property uchar red' not in raw_ply[:400] and b'property uchar red' in ao_ply[:400]
        (rv, rt), (av, at) = md.read_mesh(str(tmp_path / 'raw' / f'{name}.ply')), md.read_mesh(str(tmp_path / 'ao' / f'{name}.ply'))
        assert rv.tobytes() == av.tobytes() and rt.tobytes() == at.tobytes()
    with pytest.raises(SystemExit):
        ex.main(['--ckpt', str(tmp_path), '--seeds', '0', '--save-obj', '--ao-rays', '16', '--output-dir', str(tmp_path / 'x')])          # needs --save-ply
    with pytest.raises(SystemExit):
        ex.main(common + ['--output-dir', str(tmp_path / 'x'), '--ao-rays', '20'])
    capsys.readouterr()
    rt = _tool('render_trajectory')
    base = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--trajectory', 'front_circle', '--num-frames', '2', '--level', '0.0', '--volume-res', '24', '--seed', '5']
    rt.main(base + ['--vis', 'mesh_grid', '--out', str(tmp_path / 'face.npy')])
    rt.main(base + ['--vis', 'mesh_grid', '--out', str(tmp_path / 'face2.npy')])
    rt.main(base + ['--vis', 'mesh_grid', '--out', str(tmp_path / 'ao.npy'), '--mesh-ao-rays', '16', '--mesh-ao-radius', '0.5'])
    rt.main(base + ['--vis', 'mesh_strips', '--out', str(tmp_path / 'strips.npy'), '--mesh-ao-rays', '32'])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 4 and 'ao_rays' not in lines[0] and lines[2]['ao_rays'] == 16 and lines[2]['ao_radius'] == 0.5 and lines[3]['ao_rays'] == 32 and lines[3]['ao_radius'] is None
    assert lines[2]['shape'] == lines[0]['shape'] and lines[2]['triangles'] == lines[0]['triangles']
    a, b, c = (np.load(tmp_path / f) for f in ('face.npy', 'face2.npy', 'ao.npy'))
    assert a.tobytes() == b.tobytes() and c.shape == a.shape and c.dtype == np.uint8
    for wrong in (['--vis', 'video_grid', '--mesh-ao-rays', '16'], ['--vis', 'shape_grid', '--mesh-ao-radius', '1.0'], ['--vis', 'mesh_grid', '--mesh-ao-radius', '1.0'],
                  ['--vis', 'mesh_grid', '--mesh-ao-rays', '16', '--mesh-normals', 'field'], ['--vis', 'mesh_grid', '--mesh-ao-rays', '24']):
        with pytest.raises(SystemExit):
            rt.main(base + wrong + ['--out', str(tmp_path / 'no.npy')])
    capsys.readouterr()

"""Mesh frames on the GPU: tdgp_mesh_visibility / tdgp_mesh_resolve / tdgp_mesh_shade bit for bit against the numpy restatement of their
contracts (tests/mesh_raster_reference.py) on icospheres and hand-written triangles, the order independence of the 64-bit atomic minimum
(runs, permutations, camera chunks), watertightness, the device's marching cubes end to end against an analytic sphere, and `normals='field'`
with the frame drivers and the CLI on a seeded config_tiny scene."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_raster_reference as MR
import shapes_reference as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADE = dict(ambient=0.25, albedo=(0.9, 0.7, 0.5), background=(1.0, 0.5, -1.0))


def T(a):
    return torch.as_tensor(a).to(DEV)


def H(t):
    return t.detach().cpu().numpy()


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert not (got.dtype.kind == 'f' and np.isnan(got).any()), f'{what}: NaN in an output the contract keeps finite'
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        first = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}')


def cameras(tdgp, n=3):
    """n cameras with non-zero yaw and pitch, different fields of view and radii, looking at the origin."""
    angles = np.array([[0.3, 1.3, 0.0], [-0.5, 1.8, 0.0], [1.1, 1.5, 0.0]], F)[:n]
    return tdgp.generator.TensorGroup(angles=T(angles), fov=T(np.array([40.0, 50.0, 60.0], F)[:n]), radius=T(np.array([1.0, 1.1, 0.9], F)[:n]),
                                      look_at=T(np.zeros((n, 3), F)))


def camera_tensors(tdgp, cams, res):
    c2w = tdgp.renderer.compute_cam2world_matrix(cams)
    focal = tdgp.mesh.focal_lengths(cams.fov, c2w.shape[0], DEV)
    ray_o, ray_d = tdgp.renderer.sample_rays(c2w, fov=cams.fov, resolution=(res, res))
    return c2w, focal, ray_o, ray_d


def device_frames(tdgp, v, t, cam, res, near, cull, step, t_miss, vertex_rgb=None, mode='shaded'):
    """The three wrappers in a row on device tensors -> dict of numpy arrays named as mesh_raster_reference.frames names them."""
    M = tdgp.mesh
    c2w, focal, ray_o, ray_d = cam
    vt, tt = T(np.asarray(v, F).reshape(-1, 3)), T(np.asarray(t, np.int32).reshape(-1, 3))
    vis = M.mesh_visibility(vt, tt, c2w, focal, ray_d, res, near=near, cull=cull)
    n = vis.numel()
    t_hit, status, tri, normal, colour, points = M.mesh_resolve(vis.reshape(n), vt, tt, ray_o.reshape(n, 3), ray_d.reshape(n, 3), step, t_miss,
                                                                vertex_rgb=None if vertex_rgb is None else T(vertex_rgb))
    rgb = M.mesh_shade(normal, status, ray_d.reshape(n, 3), colour=colour, mode=mode, **SHADE)
    return dict(vis=H(vis).reshape(-1).view(np.uint64), t_hit=H(t_hit), status=H(status), tri=H(tri), normal=H(normal),
                colour=None if colour is None else H(colour), points=H(points), rgb=H(rgb))


def compare(tdgp, v, t, cam, res, what, near=0.1, cull='none', vertex_rgb=None, modes=('shaded',)):
    c2w, focal, ray_o, ray_d = cam
    want = None
    for mode in modes:
        got = device_frames(tdgp, v, t, cam, res, near, cull, 1.0 / 64, 2.5, vertex_rgb, mode)
        want = MR.frames(v, t, H(c2w), H(focal), H(ray_o), H(ray_d), res, res, near, cull, 1.0 / 64, 2.5, vertex_rgb, mode, **SHADE)
        for k in ('vis', 't_hit', 'status', 'tri', 'normal', 'points', 'rgb') + (('colour',) if vertex_rgb is not None else ()):
            same_bytes(got[k], want[k], f'{k} ({what}, {mode}, cull={cull})')
    return want


@pytest.fixture(scope='module')
def spheres():
    return {s: MR.icosphere(s, 0.3) for s in (2, 3)}


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize('subdivisions, res', [(2, 33), (3, 33), (2, 64), (3, 64)])
def test_icosphere_bit_for_bit(tdgp, spheres, subdivisions, res):
    """320 and 1280 triangles (no multiples of the 256-lane block), 33^2 rays (no multiple of 64) and 64^2, three cameras: every output of the
    three kernels equals the restatement, with vertex colours, in every shading mode."""
    v, t = spheres[subdivisions]
    rgbv = np.random.RandomState(subdivisions).rand(len(v), 3).astype(F)
    cam = camera_tensors(tdgp, cameras(tdgp), res)
    want = compare(tdgp, v, t, cam, res, f'icosphere {subdivisions} at {res}', vertex_rgb=rgbv, modes=('shaded', 'normals', 'colour'))
    share = want['status'].mean()
    assert 0.05 < share < 0.9 and set(np.unique(want['count'])) == {0, 2}
    compare(tdgp, v, t, cam, res, 'no colours')
    compare(tdgp, v, t, tuple(x[1:2] for x in cam), res, 'one camera', cull='back')


HAND_SMALL = [(-0.1, -0.1, 0), (0.2, -0.1, 0), (-0.1, 0.2, 0)]
HAND_FILL = [(-9, -9, -0.5), (9, -9, -0.5), (0, 9, -0.5)]
HAND_CASES = {
    'small': (HAND_SMALL, [(0, 1, 2)]),
    'two equal vertices': ([HAND_SMALL[0], HAND_SMALL[0], HAND_SMALL[1]], [(0, 1, 2)]),
    'three on a line': ([(-0.2, 0, 0), (0, 0, 0), (0.2, 0, 0)], [(0, 1, 2)]),
    'a vertex behind near': ([HAND_SMALL[0], HAND_SMALL[1], (0, 0, 0.95)], [(0, 1, 2)]),
    'a vertex behind the camera': ([HAND_SMALL[0], HAND_SMALL[1], (0, 0, 1.5)], [(0, 1, 2)]),
    'indices out of range': (HAND_SMALL, [(0, 1, 3), (0, -1, 2), (0, 1, 2), (2 ** 31 - 1, 0, 1)]),
    'coincident': (HAND_SMALL, [(0, 1, 2), (0, 1, 2), (1, 2, 0)]),
    'frame-filling': (HAND_FILL, [(0, 1, 2)]),
    'frame-filling behind small': (HAND_SMALL + HAND_FILL, [(3, 4, 5), (0, 1, 2)]),
    'reversed': (HAND_SMALL, [(0, 2, 1)]),
    'non-finite vertex': ([HAND_SMALL[0], HAND_SMALL[1], (np.nan, 0, 0), (np.inf, 0, 0), (1e30, 1e30, 0)], [(0, 1, 2), (0, 1, 3), (0, 1, 4)]),
}


def test_hand_written_cases_bit_for_bit(tdgp):
    """One camera at (0, 0, 1) looking down -z, 16 x 16: every hand-written case of the CPU tests (and non-finite vertices) under every cull mode."""
    res = 16
    cams = tdgp.generator.TensorGroup(angles=T(np.array([[0.0, np.pi / 2, 0.0]], F)), fov=T(np.array([60.0], F)), radius=T(np.ones(1, F)),
                                      look_at=T(np.zeros((1, 3), F)))
    cam = camera_tensors(tdgp, cams, res)
    hits = {}
    for name, (v, t) in HAND_CASES.items():
        for cull in ('none', 'back', 'front'):
            want = compare(tdgp, np.asarray(v, F), np.asarray(t, np.int32), cam, res, name, cull=cull)
            hits[name, cull] = int(want['status'].sum())
            if name == 'coincident' and cull == 'none':
                assert np.all(want['tri'][want['status'] == 1] == 0)
    n = hits['small', 'none']
    assert 4 <= n <= 30 and hits['small', 'back'] == n and hits['small', 'front'] == 0 and hits['reversed', 'back'] == 0 and hits['reversed', 'front'] == n
    assert hits['frame-filling', 'none'] == res * res and hits['frame-filling behind small', 'none'] == res * res
    for name in ('two equal vertices', 'three on a line', 'a vertex behind near', 'a vertex behind the camera', 'non-finite vertex'):
        assert hits[name, 'none'] == 0, name
    assert hits['indices out of range', 'none'] == n and hits['coincident', 'none'] == n


def test_hand_over_to_the_wave_in_one_launch(tdgp, spheres):
    """Sub-pixel triangles and frame-filling ones in the same launch (the large ones at several places in a wave, behind and in front of the
    sphere), three cameras, 33 x 33: the wave path and the lane path agree with the restatement; T = 0 and V = 0 clear the buffer."""
    v, t = spheres[3]
    big_v = np.array([(-5, -5, -0.6), (5, -5, -0.6), (0, 5, -0.6), (-5, -5, 0.1), (5, -5, 0.1), (0, 5, 0.1), (0.0, 0.0, 0.45), (0.4, 0.0, 0.45), (0.0, 0.4, 0.45)], F)
    n = len(v)
    big_t = np.array([(n, n + 1, n + 2), (n + 3, n + 4, n + 5), (n + 6, n + 7, n + 8)], np.int32)
    tt = np.concatenate([big_t[:1], t[:100], big_t[1:2], t[100:700], big_t[2:], t[700:], big_t[:1]])
    vv = np.concatenate([v, big_v])
    res = 33
    cam = camera_tensors(tdgp, cameras(tdgp), res)
    want = compare(tdgp, vv, tt, cam, res, 'mixed sizes', vertex_rgb=np.random.RandomState(7).rand(len(vv), 3).astype(F), modes=('colour',))
    large = [0, 101, 702]                                     # where the large triangles sit in tt (the last one repeats the first and loses the tie)
    per_camera = np.isin(want['tri'], large).reshape(3, -1).sum(axis=1)
    assert per_camera.max() > 64, per_camera                  # more pixels than a lane takes: they came through the wave (an oblique camera may drop them: no clipper)
    assert len(np.unique(want['tri'])) > 50 and not np.any(want['tri'] == len(tt) - 1)
    empty = compare(tdgp, vv, np.zeros((0, 3), np.int32), cam, res, 'T = 0')
    assert empty['status'].sum() == 0 and np.all(empty['vis'] == MR.EMPTY)
    compare(tdgp, np.zeros((0, 3), F), np.zeros((0, 3), np.int32), cam, res, 'V = 0')
    compare(tdgp, np.zeros((0, 3), F), t, cam, res, 'V = 0 with triangles')


# ------------------------------------------------------------------------------------------------ order independence, watertightness
def test_order_independence_and_chunking(tdgp, spheres):
    M = tdgp.mesh
    v, t = spheres[3]
    res = 33
    R = res * res
    cams = cameras(tdgp)
    vt, tt = T(v), T(t)
    base = M.render_mesh_views(vt, tt, cams, res, **SHADE)
    assert base.rgb.shape == (3, R, 3) and base.depth.shape == (3, R, 1) and base.normal.shape == (3, R, 3) and base.status.shape == (3, R) and base.tri.shape == (3, R)
    assert base.status.dtype == torch.int32 and base.tri.dtype == torch.int32
    again = M.render_mesh_views(vt, tt, cams, res, **SHADE)
    for k in base:
        assert torch.equal(base[k], again[k]), k
    cam = camera_tensors(tdgp, cams, res)
    want = MR.frames(v, t, H(cam[0]), H(cam[1]), H(cam[2]), H(cam[3]), res, res, 1e-3, 'none', 0.0, 0.0, **SHADE)
    for k, name in (('rgb', 'rgb'), ('depth', 't_hit'), ('normal', 'normal'), ('status', 'status'), ('tri', 'tri')):
        same_bytes(H(base[k]).reshape(want[name].shape), want[name], f'render_mesh_views {k}')
    perm = np.random.RandomState(3).permutation(len(t))
    shuffled = M.render_mesh_views(vt, T(t[perm]), cams, res, **SHADE)
    assert torch.equal(shuffled.depth, base.depth) and torch.equal(shuffled.status, base.status) and torch.equal(shuffled.rgb, base.rgb)
    hit = H(base.status) == 1
    assert np.array_equal(perm[H(shuffled.tri)[hit]], H(base.tri)[hit]) and np.all(H(shuffled.tri)[~hit] == -1)
    for chunk in (R, R + 7, 2 * R + res // 2, 5):
        out = M.render_mesh_views(vt, tt, cams, res, max_rays_per_call=chunk, **SHADE)
        for k in base:
            assert torch.equal(base[k], out[k]), (k, chunk)


def test_watertight_on_the_device(tdgp, spheres):
    """A closed mesh: the front faces and the back faces cover the same pixels."""
    M = tdgp.mesh
    for s, res in ((2, 64), (3, 33), (3, 64)):
        v, t = spheres[s]
        back = M.render_mesh_views(T(v), T(t), cameras(tdgp), res, cull='back')
        front = M.render_mesh_views(T(v), T(t), cameras(tdgp), res, cull='front')
        assert torch.equal(back.status, front.status) and 0.05 < float(back.status.float().mean()) < 0.9
        hit = back.status == 1
        assert bool((front.depth[..., 0][hit] > back.depth[..., 0][hit]).all())


# ------------------------------------------------------------------------------------------------ marching cubes end to end
@pytest.mark.parametrize('vol', [32, 48])
def test_marching_cubes_sphere_end_to_end(tdgp, vol):
    """gain * (r - |x|) on the plain lattice of a unit cube -> marching_cubes -> grid_to_world(sheared=False, crop=None) -> mesh frames from a
    camera at distance 1, fov 50, 64 x 64.  On hits with analytic incidence cosine >= 0.3 (at most 12 % left out): |t - t_analytic| <=
    sqrt(3) * voxel_size / cos -- each facet lies inside a cell the surface crosses.  The normals of the stored winding point outward."""
    g, M = tdgp.geometry, tdgp.mesh
    r, cube, res, fov = 0.3, 1.0, 64, 50.0
    voxel = cube / (vol - 1)
    ax = np.arange(vol) * voxel - cube / 2
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    volume = T((200.0 * (r - np.sqrt(x * x + y * y + z * z))).astype(F))
    verts, tris = g.marching_cubes(volume, 0.0)
    world = g.grid_to_world(verts, vol, (0.0, 0.0, 0.0), cube, crop=None, sheared=False)
    assert world.is_cuda and world.dtype == torch.float32 and tris.shape[0] > 500
    assert float((world.double().norm(dim=1) - r).abs().max()) < voxel
    cams = tdgp.generator.TensorGroup(angles=T(np.array([[0.0, np.pi / 2, 0.0]], F)), fov=T(np.array([fov], F)), radius=T(np.ones(1, F)),
                                      look_at=T(np.zeros((1, 3), F)))
    out = M.render_mesh_views(world, tris, cams, res, near=0.1, t_miss=2.0, cull='back')
    c2w, focal, ray_o, ray_d = camera_tensors(tdgp, cams, res)
    o, d = H(ray_o)[0], H(ray_d)[0]
    ahit, t_an, _ = SR.ray_sphere(o, d, r)
    hit = H(out.status)[0] == 1
    both = hit & ahit
    cos = np.where(both, MR.sphere_cosine(o, d, np.where(both, t_an, 1.0), r), 0.0)
    keep = both & (cos >= 0.3)
    left_out = 1.0 - keep.sum() / hit.sum()
    err = np.abs(H(out.depth)[0, :, 0].astype(np.float64) - t_an)[keep] * cos[keep] / (np.sqrt(3.0) * voxel)
    print(f'{vol}^3: {tris.shape[0]} triangles, hit fraction {hit.mean():.4f}, left out {left_out:.4f}, worst |t - t_analytic| = {err.max():.4f} sqrt(3) voxel / cos')
    assert 0.2 <= hit.mean() <= 0.8 and left_out <= 0.12
    assert err.max() <= 1.0
    n = H(out.normal)[0][keep].astype(np.float64)
    p = o[keep] + d[keep] * H(out.depth)[0, keep]
    assert np.all((n * p).sum(1) > 0)


# ------------------------------------------------------------------------------------------------ normals='field', the drivers, the CLI
B, V, VOL = 2, 3, 24


@pytest.fixture(scope='module')
def scene(tdgp):
    """config_tiny, seeded weights, 2 samples x 3 cameras, volume_res 24 over the whole field; the level is the median of the density grids."""
    cfg = tdgp.config.config_tiny()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    G = G.to(DEV).eval()
    inp = tdgp.weights.synthetic_inputs(cfg, batch=B, seed=12)
    ws = G.mapping(T(inp['z']), T(inp['c']))
    cam_np = tdgp.weights.synthetic_inputs(cfg, batch=B * V, seed=13)['camera']
    cams = tdgp.generator.TensorGroup(**{k: T(v) for k, v in cam_np.items()})
    box = 2.0 * cfg.cube_scale
    with torch.no_grad():
        grid = tdgp.geometry.density_grid(G, ws, volume_res=VOL, cube_size=box)
        planes = G.synthesis.tri_planes(ws, noise_mode='const')
    level = float(grid.median())
    return dict(G=G, ws=ws, cams=cams, level=level, grid=grid, planes=planes, box=box, res=G.synthesis.test_resolution)


def test_field_normals_equal_the_restated_chain(tdgp, scene):
    """normals='field': restated visibility + resolve on the device's own mesh, the product's own field values at the restated points and
    shapes_reference.shade, bit for bit, in every mode; frames hold hits and misses; the planes-taking density grid is density_grid's."""
    g, M, Sh = tdgp.geometry, tdgp.mesh, tdgp.shapes
    sc = scene
    G, res = sc['G'], sc['res']
    R = res * res
    cfg = G.cfg
    step = 2.0 * cfg.cube_scale / cfg.tri_plane_res
    point_field = Sh.field_functions(G.synthesis)[1]
    with torch.no_grad():
        syn = G.synthesis
        own = tdgp.renderer.planes_to_hwc(syn.tri_plane_decoder(sc['ws'][:, :syn.tri_plane_decoder.num_ws], hwc=True, noise_mode='const'))
        assert torch.equal(g.density_grid_from_planes(G, own, VOL, cube_size=sc['box']), sc['grid'])
    for b in range(B):
        pb = tdgp.renderer.HWCPlanes(sc['planes'].t[b:b + 1])
        verts, tris = g.marching_cubes(sc['grid'][b], sc['level'])
        world = g.grid_to_world(verts, VOL, (0.0, 0.0, 0.0), sc['box'], crop=None)
        assert tris.shape[0] > 100
        cams = sc['cams'][b * V:(b + 1) * V]
        c2w, focal, ray_o, ray_d = camera_tensors(tdgp, cams, res)
        o, d = H(ray_o).reshape(-1, 3), H(ray_d).reshape(-1, 3)
        vis, _ = MR.visibility(H(world), H(tris), H(c2w), H(focal), d, res, res, cfg.ray_start)
        want = MR.resolve(vis, H(world), H(tris), o, d, step, cfg.ray_end)
        share = want['status'].mean()
        assert 0.02 < share < 0.98, f'sample {b}: {share:.3f} of the rays hit'
        stencil = H(point_field(pb, T(want['points']).reshape(1, -1, 3))).reshape(-1, 7, 4)
        for mode in ('shaded', 'normals', 'colour'):
            rgb, normal = SR.shade(stencil, want['status'], d, mode, **SHADE)
            for chunk in (None, R):
                out = M.render_mesh_views(world, tris, cams, res, mode=mode, normals='field', planes=pb, G=G, max_rays_per_call=chunk, **SHADE)
                tag = f'sample {b} {mode} chunk={chunk}'
                same_bytes(H(out.status).reshape(-1), want['status'], 'status ' + tag)
                same_bytes(H(out.depth).reshape(-1), want['t_hit'], 'depth ' + tag)
                same_bytes(H(out.tri).reshape(-1), want['tri'], 'tri ' + tag)
                same_bytes(H(out.normal).reshape(-1, 3), normal, 'normal ' + tag)
                same_bytes(H(out.rgb).reshape(-1, 3), rgb, 'rgb ' + tag)


def test_extract_geometry_in_world_units(tdgp, scene):
    """units='world' is `grid_to_world` of the index-unit mesh with the call's own arguments, crop offsets included; the default is unchanged."""
    g = tdgp.geometry
    sc = scene
    kw = dict(volume_res=VOL, cube_size=sc['box'], thresh_value=sc['level'])
    for crop in ('reference', None):
        index = g.extract_geometry(sc['G'], sc['ws'], crop=crop, normalize=False, **kw)
        world = g.extract_geometry(sc['G'], sc['ws'], crop=crop, units='world', **kw)
        plain = g.extract_geometry(sc['G'], sc['ws'], crop=crop, units='world', sheared=False, **kw)
        assert len(index) == len(world) == B and world[0]._fields == ('vertices', 'triangles', 'sigma')
        for i, w, p in zip(index, world, plain):
            assert (crop is not None or i.vertices.shape[0] > 0) and torch.equal(w.triangles, i.triangles) and torch.equal(w.sigma, i.sigma)
            assert torch.equal(w.vertices, g.grid_to_world(i.vertices, VOL, (0.0, 0.0, 0.0), sc['box'], crop=crop))
            assert torch.equal(p.vertices, g.grid_to_world(i.vertices, VOL, (0.0, 0.0, 0.0), sc['box'], crop=crop, sheared=False))
            if w.vertices.shape[0]:
                assert float(w.vertices.abs().max()) <= sc['box'] / 2 + 1.1 * sc['box'] / (VOL - 1)          # the shear adds up to one voxel
    # the field's density at the world vertices is the level, to within the variation inside a cell; not so with the plain lattice
    point_field = tdgp.shapes.field_functions(sc['G'].synthesis)[1]
    pb = tdgp.renderer.HWCPlanes(sc['planes'].t[:1])
    cell = float((sc['grid'][0, 1:] - sc['grid'][0, :-1]).abs().median())
    off = lambda v: float((point_field(pb, v.unsqueeze(0))[0, :, 3] - sc['level']).abs().median())      # noqa: E731
    print(f'median |sigma - level| at the vertices: sheared {off(world[0].vertices):.4g}, plain lattice {off(plain[0].vertices):.4g}; median adjacent grid difference {cell:.4g}')
    assert off(world[0].vertices) < cell and off(world[0].vertices) < off(plain[0].vertices)


def test_drivers_grids_and_strips(tdgp, scene):
    M, I, Sh = tdgp.mesh, tdgp.inference, tdgp.shapes
    sc = scene
    G, res = sc['G'], sc['res']
    kw = dict(level=sc['level'], volume_res=VOL, **SHADE)
    frames, counts = M.render_mesh_frames(G, sc['ws'], sc['cams'], return_counts=True, **kw)
    assert frames.rgb.shape == (B * V, res * res, 3) and len(counts) == B and all(v > 0 and t > 0 for v, t in counts)
    assert 0 < int(frames.status.sum()) < frames.status.numel()
    one = M.render_mesh_frames(G, sc['ws'], sc['cams'], plane_batch=1, **kw)
    for k in frames:
        assert torch.equal(frames[k], one[k]), k
    grid = M.render_mesh_video_grid(G, sc['ws'], sc['cams'], **kw)
    assert torch.equal(grid, I.frames_to_grid(frames.rgb, res, res, tiles=B, images=V, stride_image=1, stride_tile=V, nrow=2))
    assert torch.equal(grid, M.render_mesh_video_grid(G, sc['ws'], sc['cams'], **kw))
    shape_grid = Sh.render_shape_video_grid(G, sc['ws'], sc['cams'], level=sc['level'])
    assert grid.dtype == torch.uint8 and grid.shape == shape_grid.shape
    strips = M.render_mesh_strips(G, sc['ws'], sc['cams'], show='depth', as_numpy=True, normals='field', mode='colour', **kw)
    shape_strips = Sh.render_shape_strips(G, sc['ws'], sc['cams'], level=sc['level'], show='depth', as_numpy=True)
    assert isinstance(strips, np.ndarray) and strips.dtype == np.uint8 and strips.shape == shape_strips.shape == (B, res, V * res, 3)
    face_colour = M.render_mesh_frames(G, sc['ws'], sc['cams'], mode='colour', **kw)
    assert torch.equal(face_colour.status, frames.status) and not torch.equal(face_colour.rgb, frames.rgb)
    # agreement with shape frames, printed and not asserted: a random-weight field has structure below a voxel
    shape = Sh.render_shape_views(G, sc['planes'], sc['cams'], level=sc['level'])
    # (status 2 of a shape frame -- the level already met at the near plane, where the mesh shows the surface behind it -- is not a crossing)
    mh, sh = H(frames.status) == 1, H(shape.status) == 1
    both = mh & sh
    diff = np.abs(H(frames.depth)[..., 0] - H(shape.depth)[..., 0])[both]
    q = np.quantile(diff, [0.5, 0.9, 0.99]) if both.any() else [np.nan] * 3
    print(f'mesh hits {mh.mean():.3f}, shape hits {sh.mean():.3f}, both {both.mean():.3f}, either {(mh | sh).mean():.3f}; '
          f'|depth difference| where both hit: median {q[0]:.4f}, 90 % {q[1]:.4f}, 99 % {q[2]:.4f} (voxel {sc["box"] / (VOL - 1):.4f})')


def test_cli_writes_a_mesh_grid(tdgp, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location('render_trajectory_cli', os.path.join(REPO, 'tools', 'render_trajectory.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = tdgp.config.config_tiny()
    sd = tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True)
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **sd)
    common = ['--ckpt', str(tmp_path), '--seeds', '0-3', '--trajectory', 'front_circle', '--num-frames', '4', '--level', '0.0', '--volume-res', '24', '--seed', '5']
    cli.main(common + ['--vis', 'mesh_grid', '--out', str(tmp_path / 'mesh.gif')])
    cli.main(common + ['--vis', 'mesh_strips', '--mesh-normals', 'field', '--shape-mode', 'normals', '--out', str(tmp_path / 'strips.png')])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2 and os.path.getsize(tmp_path / 'mesh.gif') > 0 and os.path.getsize(tmp_path / 'strips.png') > 0
    res = cfg.img_resolution
    assert lines[0]['vis'] == 'mesh_grid' and lines[0]['shape'] == [4, 2 * (res + 2) + 2, 2 * (res + 2) + 2, 3] and lines[0]['volume_res'] == 24
    assert len(lines[0]['vertices']) == 4 and len(lines[0]['triangles']) == 4 and sum(lines[0]['triangles']) > 0
    assert lines[1]['vis'] == 'mesh_strips' and lines[1]['shape'] == [1, 4 * res, 4 * res, 3] and lines[1]['mesh_normals'] == 'field'
    assert lines[1]['triangles'] == lines[0]['triangles']

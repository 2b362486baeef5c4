"""Mesh frames, the parts that need no GPU: the numpy restatement of the rasteriser contracts (tests/mesh_raster_reference.py) against an analytic
sphere -- before the GPU tests trust it --, hand-written triangles, `geometry.grid_to_world` against the reference grid's formula, the Python
layer's refusals before any device call, the CLI's new arguments, the .ply writer's colours, and the three new entry points in header, binding
and library."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_raster_reference as MR
import shapes_reference as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('tdgp_mesh_visibility', 'tdgp_mesh_resolve', 'tdgp_mesh_shade')
F = np.float32


def _cli():
    spec = importlib.util.spec_from_file_location('render_trajectory_cli', os.path.join(REPO, 'tools', 'render_trajectory.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the restatement against an analytic sphere
SPHERE = dict(radius=0.3, fov=50.0, res=64, subdivisions=3, near=0.1, t_miss=2.0)


@pytest.fixture(scope='module')
def sphere():
    p = SPHERE
    v, t = MR.icosphere(p['subdivisions'], p['radius'])
    o, d = SR.pinhole_rays(p['res'], p['fov'])
    c2w, focal = MR.pinhole_camera(p['fov'])
    out = MR.frames(v, t, c2w, focal, o, d, p['res'], p['res'], p['near'], 'none', 1.0 / 64, p['t_miss'])
    return dict(v=v, t=t, o=o, d=d, c2w=c2w, focal=focal, out=out, sag=MR.sagitta(v, t, p['radius']))


def test_icosphere_is_closed_and_wound_outward(sphere):
    v, t = sphere['v'].astype(np.float64), sphere['t']
    assert t.shape == (1280, 3) and v.shape == (642, 3)
    assert np.abs(np.linalg.norm(v, axis=1) - SPHERE['radius']).max() < 1e-6
    P = v[t]
    volume = np.einsum('ni,ni->n', P[:, 0], np.cross(P[:, 1], P[:, 2])).sum() / 6.0
    assert 0.9 * 4 / 3 * np.pi * SPHERE['radius'] ** 3 < volume < 4 / 3 * np.pi * SPHERE['radius'] ** 3
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, n = np.unique(edges, axis=0, return_counts=True)
    assert np.all(n == 2)                                   # every edge is shared by exactly two triangles


def test_restatement_finds_the_analytic_sphere(sphere):
    """Outside a band of (sagitta + one pixel footprint) around the analytic silhouette status equals the analytic hit mask (the polyhedron lies
    between the spheres of radius r - sagitta and r); the band holds at most 10 % of the pixels.  The hit fraction keeps the silhouette inside
    the frame."""
    p, out = SPHERE, sphere['out']
    res = p['res']
    b = MR.impact_parameter(sphere['o'], sphere['d'])
    footprint = 2.0 * np.tan(np.deg2rad(p['fov']) / 2.0) / (res - 1)           # of one pixel at the sphere's centre, a distance of 1 away
    band = np.abs(b - p['radius']) <= sphere['sag'] + footprint
    hit = out['status'] == 1
    wrong = (hit != (b < p['radius'])) & ~band
    print(f'sagitta {sphere["sag"]:.5f}, footprint {footprint:.5f}, band {band.mean():.4f} of the pixels, mismatches outside it {int(wrong.sum())}, '
          f'hit fraction {hit.mean():.4f}')
    assert band.mean() <= 0.10
    assert wrong.sum() == 0
    assert 0.2 <= hit.mean() <= 0.8
    img = hit.reshape(res, res)
    assert not (img[0].any() or img[-1].any() or img[:, 0].any() or img[:, -1].any())
    assert np.array_equal(out['tri'] >= 0, hit) and np.all(out['t_hit'][~hit] == F(p['t_miss'])) and np.all(out['normal'][~hit] == 0)


def test_restatement_fill_rule_covers_a_closed_convex_mesh_twice(sphere):
    """Every covered pixel of a closed convex mesh is covered exactly twice, front and back: a centre on a shared edge goes to one triangle."""
    count = sphere['out']['count']
    assert set(np.unique(count)) == {0, 2}
    assert np.array_equal(count == 2, sphere['out']['status'] == 1)


def test_restatement_depths_against_the_analytic_sphere(sphere):
    """On hits with analytic incidence cosine >= 0.3: |t - t_analytic| <= 1.5 * sagitta / cos (the facet lies at most the sagitta inside the
    sphere; the 1.5 covers the facet-vs-sphere normal difference); at most 12 % of the hits are left out.  The front faces win: every normal
    faces the camera and is a unit vector."""
    p, out = SPHERE, sphere['out']
    ahit, t_an, _ = SR.ray_sphere(sphere['o'], sphere['d'], p['radius'])
    hit = out['status'] == 1
    both = hit & ahit
    cos = np.where(both, MR.sphere_cosine(sphere['o'], sphere['d'], np.where(both, t_an, 1.0), p['radius']), 0.0)
    keep = both & (cos >= 0.3)
    left_out = 1.0 - keep.sum() / hit.sum()
    err = np.abs(out['t_hit'].astype(np.float64) - t_an)[keep] * cos[keep] / sphere['sag']
    print(f'kept {int(keep.sum())} of {int(hit.sum())} hits (left out {left_out:.4f}); worst |t - t_analytic| = {err.max():.3f} sagitta / cos')
    assert left_out <= 0.12
    assert err.max() <= 1.5
    n, d = out['normal'][hit].astype(np.float64), sphere['d'][hit].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6 and np.all((n * d).sum(1) < 0)
    x = out['points'][hit, 0].astype(np.float64)
    assert np.all((n * x).sum(1) > 0)                        # outward: the stored winding's normal


def test_restatement_culling_and_colours(sphere):
    p = SPHERE
    args = (sphere['v'], sphere['t'], sphere['c2w'], sphere['focal'], sphere['o'], sphere['d'], p['res'], p['res'], p['near'])
    rgbv = (sphere['v'] / F(2 * p['radius']) + F(0.5)).astype(F)
    back = MR.frames(*args, 'back', 0.0, p['t_miss'], vertex_rgb=rgbv, mode='colour')
    front = MR.frames(*args, 'front', 0.0, p['t_miss'])
    base = sphere['out']
    assert np.array_equal(back['status'], base['status']) and np.array_equal(front['status'], base['status'])        # watertight either way
    assert np.array_equal(back['t_hit'], base['t_hit']) and np.array_equal(back['tri'], base['tri'])
    hit = base['status'] == 1
    assert np.all(front['t_hit'][hit] > base['t_hit'][hit]) and set(np.unique(back['count'])) == {0, 1} and set(np.unique(front['count'])) == {0, 1}
    # barycentric colours of a linear function of the position reproduce it at the hit point's projection onto the facet.  The hit leaves the
    # facet's plane by at most the snap of the vertices, 1/512 of a pixel's footprint (at a distance below 1), times the function's slope
    # 1 / (2 r); 1e-6 for the fp32 roundings of values below 1
    x = back['points'][hit, 0].astype(np.float64)
    snap = 2.0 * np.tan(np.deg2rad(p['fov']) / 2.0) / (p['res'] - 1) / 512.0
    err = np.abs(back['colour'][hit] - (x / (2 * p['radius']) + 0.5)).max()
    print(f'colour error {err:.3g}, bound {snap / (2 * p["radius"]) + 1e-6:.3g}')
    assert err <= snap / (2 * p['radius']) + 1e-6
    assert np.all(back['colour'][~hit] == 0) and np.all(back['rgb'][~hit] == 1)


# ------------------------------------------------------------------------------------------------ hand-written triangles
RES = 16


def _one_camera(fov=60.0):
    o, d = SR.pinhole_rays(RES, fov)
    c2w, focal = MR.pinhole_camera(fov)
    return o, d, c2w, focal


def _run(v, t, cull='none', near=0.1, **kw):
    o, d, c2w, focal = _one_camera()
    return MR.frames(np.asarray(v, F).reshape(-1, 3), np.asarray(t, np.int32).reshape(-1, 3), c2w, focal, o, d, RES, RES, near, cull, 0.01, 5.0, **kw)


HAND = dict(
    small=[(-0.1, -0.1, 0), (0.2, -0.1, 0), (-0.1, 0.2, 0)],                   # counter-clockwise seen from the camera at z = 1: a front face
    fill=[(-9, -9, -0.5), (9, -9, -0.5), (0, 9, -0.5)],                        # covers the frame
)


def test_hand_written_cases():
    small, fill = HAND['small'], HAND['fill']
    out = _run(small, [(0, 1, 2)])
    n_small = int(out['status'].sum())
    assert 4 <= n_small <= 30 and np.all(out['tri'][out['status'] == 1] == 0)
    assert np.allclose(out['normal'][out['status'] == 1], (0, 0, 1))
    assert np.allclose(out['points'][out['status'] == 1, 0, 2], 0, atol=1e-6)
    # a zero-area triangle (two equal vertices; three on a line)
    for tri_v in ([small[0], small[0], small[1]], [(-0.2, 0, 0), (0, 0, 0), (0.2, 0, 0)]):
        assert _run(tri_v, [(0, 1, 2)])['status'].sum() == 0
    # one vertex behind `near`: dropped whole (z = 0.95 is 0.05 in front of the camera at z = 1)
    assert _run([small[0], small[1], (0, 0, 0.95)], [(0, 1, 2)])['status'].sum() == 0
    assert _run([small[0], small[1], (0, 0, 0.95)], [(0, 1, 2)], near=0.01)['status'].sum() > 0
    assert _run([small[0], small[1], (0, 0, 1.5)], [(0, 1, 2)])['status'].sum() == 0          # behind the camera
    # out-of-range indices skip their triangle, the valid one is drawn
    out = _run(small, [(0, 1, 3), (0, -1, 2), (0, 1, 2)])
    assert int(out['status'].sum()) == n_small and np.all(out['tri'][out['status'] == 1] == 2)
    # coincident triangles: the lower index wins
    out = _run(small, [(0, 1, 2), (0, 1, 2), (1, 2, 0)])
    assert int(out['status'].sum()) == n_small and np.all(out['tri'][out['status'] == 1] == 0) and np.all(out['count'][out['status'] == 1] == 3)
    # a frame-filling triangle, and the small one in front of it
    out = _run(fill, [(0, 1, 2)])
    assert np.all(out['status'] == 1) and np.allclose(out['points'][:, 0, 2], -0.5, atol=1e-6)
    out = _run(small + fill, [(3, 4, 5), (0, 1, 2)])
    assert np.all(out['status'] == 1) and int((out['tri'] == 1).sum()) == n_small
    # culling: `small` is a front face, its reverse a back face
    assert _run(small, [(0, 1, 2)], cull='back')['status'].sum() == n_small and _run(small, [(0, 1, 2)], cull='front')['status'].sum() == 0
    assert _run(small, [(0, 2, 1)], cull='back')['status'].sum() == 0 and _run(small, [(0, 2, 1)], cull='front')['status'].sum() == n_small
    assert np.allclose(_run(small, [(0, 2, 1)])['normal'][out['tri'] == 1], (0, 0, -1))
    # T = 0, V = 0
    out = _run(np.zeros((0, 3)), np.zeros((0, 3)))
    assert out['status'].sum() == 0 and np.all(out['vis'] == MR.EMPTY) and np.all(out['t_hit'] == F(5.0)) and np.all(out['rgb'] == 1)


# ------------------------------------------------------------------------------------------------ grid_to_world
def _voxel_coords_numpy(res, voxel_origin, cube_size):
    """create_voxel_coords' formula (geometry.py's docstring, extract_geometry.py:55-76) in numpy float32: [res^3, 3]."""
    origin = np.array(voxel_origin, np.float64) - cube_size / 2.0
    voxel_size = F(cube_size / (res - 1))
    idx = np.arange(res ** 3, dtype=np.int64)
    c = np.zeros((res ** 3, 3), F)
    fi = idx.astype(F)
    c[:, 2] = (idx % res).astype(F)
    c[:, 1] = np.fmod(fi / F(res), F(res))
    c[:, 0] = np.fmod((fi / F(res)) / F(res), F(res))
    c[:, 0] = c[:, 0] * voxel_size + F(origin[2])
    c[:, 1] = c[:, 1] * voxel_size + F(origin[1])
    c[:, 2] = c[:, 2] * voxel_size + F(origin[0])
    return c


@pytest.mark.parametrize('res, origin, cube', [(8, (0.0, 0.0, 0.0), 0.3), (33, (0.1, -0.2, 0.05), 2.0), (64, (0.0, 0.0, 0.0), 1.0)])
def test_grid_to_world_meets_the_reference_grid(tdgp, res, origin, cube):
    """At integer indices: within 8 fp32 ulps of the largest |coordinate| of create_voxel_coords' formula (about four rounded operations of slack
    on each side); sheared=False is the plain lattice.  With a power-of-two res the formula's `idx.float() / res` is exact and that is the whole
    bound.  Otherwise (res = 33) the formula itself rounds idx / res, a number up to res^2, before it takes `% res`: half an ulp of res^2 in
    index units, one voxel_size of that in world units, is the formula's own error and is added -- grid_to_world is the exact affine map."""
    g = tdgp.geometry
    d, h, w = np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing='ij')
    idx = torch.tensor(np.stack([d, h, w], axis=-1).reshape(-1, 3), dtype=torch.float32)
    want = _voxel_coords_numpy(res, origin, cube)
    got = g.grid_to_world(idx, res, origin, cube, crop=None, sheared=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (res ** 3, 3)
    tol = 8 * np.spacing(F(np.abs(want).max()))
    if res & (res - 1):
        tol = tol + 0.5 * np.spacing(F(res * res)) * cube / (res - 1)
    err = np.abs(got.numpy().astype(np.float64) - want.astype(np.float64)).max()
    print(f'res {res}: max |grid_to_world - formula| = {err:.3g}, bound {tol:.3g}')
    assert err <= tol
    plain = g.grid_to_world(idx, res, origin, cube, crop=None, sheared=False).numpy().astype(np.float64)
    voxel = float(F(cube / (res - 1)))
    org = [float(F(origin[k] - cube / 2.0)) for k in (2, 1, 0)]
    lattice = np.stack([d.reshape(-1) * voxel + org[0], h.reshape(-1) * voxel + org[1], w.reshape(-1) * voxel + org[2]], axis=1)
    assert np.abs(plain - lattice).max() <= np.spacing(F(np.abs(lattice).max()))


def test_grid_to_world_crop_offsets(tdgp):
    """The crop's start offsets use Python's floor semantics; fractional vertices pass through the affine map."""
    g = tdgp.geometry
    v = torch.tensor([[0.0, 0.0, 0.0], [1.5, 2.25, 3.0]])
    for res in (30, 50, 64):
        sl = g.crop_reference(res)
        assert [s.indices(res)[0] for s in sl] == [res // 8, res // 2, 0]
        a = g.grid_to_world(v, res, crop='reference', sheared=False)
        b = g.grid_to_world(v + torch.tensor([res // 8, res // 2, 0.0]), res, crop=None, sheared=False)
        assert torch.equal(a, b)
    neg = (slice(-10, None), slice(-7, -2), slice(3, None))
    a = g.grid_to_world(v, 32, crop=neg)
    b = g.grid_to_world(v + torch.tensor([22.0, 25.0, 3.0]), 32, crop=None)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        g.grid_to_world(v, 32, crop='nonsense')
    with pytest.raises(ValueError):
        g.grid_to_world(v[:, :2], 32)
    with pytest.raises(ValueError):
        g.extract_geometry(None, torch.zeros(1, 2, 4), units='metres')


# ------------------------------------------------------------------------------------------------ the Python layer
def _cams(tdgp, n):
    return tdgp.generator.TensorGroup(angles=torch.zeros(n, 3), fov=torch.full([n], 20.0), radius=torch.ones(n), look_at=torch.zeros(n, 3))


def test_refusals_before_any_device_call(tdgp):
    M = tdgp.mesh
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    cams = _cams(tdgp, 2)
    with pytest.raises(ValueError, match='mode'):
        M.render_mesh_views(v, t, cams, 16, mode='wireframe')
    with pytest.raises(ValueError, match='normals'):
        M.render_mesh_views(v, t, cams, 16, normals='vertex')
    with pytest.raises(ValueError, match='cull'):
        M.render_mesh_views(v, t, cams, 16, cull='both')
    with pytest.raises(ValueError, match='planes'):
        M.render_mesh_views(v, t, cams, 16, normals='field')
    with pytest.raises(ValueError, match='vertex_colours'):
        M.render_mesh_views(v, t, cams, 16, mode='colour')
    with pytest.raises(ValueError, match='max_rays_per_call'):
        M.render_mesh_views(v, t, cams, 16, max_rays_per_call=0)
    with pytest.raises(ValueError, match='fp32'):
        M.render_mesh_views(v.double(), t, cams, 16)
    with pytest.raises(ValueError, match='int32'):
        M.render_mesh_views(v, t.long(), cams, 16)
    with pytest.raises(ValueError, match=r'\[V,3\]'):
        M.render_mesh_views(v.reshape(3, 4), t, cams, 16)
    with pytest.raises(ValueError, match=r'\[T,3\]'):
        M.render_mesh_views(v, t.reshape(3, 2), cams, 16)
    with pytest.raises(TypeError):
        M.render_mesh_views(v.numpy(), t, cams, 16)
    with pytest.raises(RuntimeError, match='GPU'):
        M.render_mesh_views(v, t, cams, 16)                       # a well-formed CPU mesh: refused as such, there is no CPU path
    with pytest.raises(ValueError, match='cull'):
        M.mesh_visibility(v, t, torch.zeros(1, 4, 4), torch.ones(1), torch.zeros(1, 256, 3), 16, cull=3)
    with pytest.raises(ValueError, match='mode'):
        M.mesh_shade(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3), mode='flat')
    with pytest.raises(ValueError, match='colour'):
        M.mesh_shade(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3), mode='colour')
    G = tdgp.generator.Generator(tdgp.config.config_tiny())
    ws = torch.zeros(2, G.num_ws, G.w_dim)
    with pytest.raises(ValueError, match='multiple'):
        M.render_mesh_frames(G.eval(), ws, _cams(tdgp, 3))
    with pytest.raises(ValueError, match='normals'):
        M.render_mesh_frames(G.eval(), ws, _cams(tdgp, 4), normals='smooth')
    with pytest.raises(RuntimeError, match='eval'):
        M.render_mesh_frames(G.train(), ws, _cams(tdgp, 4))
    with pytest.raises(ValueError, match='show'):
        M.render_mesh_strips(G.eval(), ws, _cams(tdgp, 4), show='normal')
    with pytest.raises(ValueError, match='show'):
        M.render_mesh_video_grid(G.eval(), ws, _cams(tdgp, 4), show='normal')


def test_focal_lengths(tdgp):
    f = tdgp.mesh.focal_lengths(torch.tensor([20.0, 50.0, 90.0]), 3, 'cpu')
    want = 1.0 / np.tan(np.deg2rad([20.0, 50.0, 90.0]) / 2.0)
    assert f.dtype == torch.float32 and np.abs(f.numpy() / want - 1).max() < 3e-7
    assert torch.equal(tdgp.mesh.focal_lengths(50.0, 3, 'cpu'), f[1:2].expand(3))
    with pytest.raises(ValueError):
        tdgp.mesh.focal_lengths(torch.ones(2), 3, 'cpu')


def test_cli_takes_the_mesh_modes():
    cli = _cli()
    p = cli.build_parser()
    a = p.parse_args(['--ckpt', 'x', '--out', 'y.gif'])
    assert a.vis == 'video_grid' and a.volume_res == 256 and a.cube_size is None and a.mesh_normals == 'face' and a.level == 25.0
    a = p.parse_args(['--ckpt', 'x', '--out', 'y.gif', '--vis', 'mesh_grid', '--volume-res', '128', '--cube-size', '0.5', '--mesh-normals', 'field'])
    assert a.vis == 'mesh_grid' and a.volume_res == 128 and a.cube_size == 0.5 and a.mesh_normals == 'field'
    opts = cli.mesh_options(a)
    assert opts['volume_res'] == 128 and opts['normals'] == 'field' and opts['level'] == 25.0 and opts['mode'] == 'shaded'
    assert p.parse_args(['--ckpt', 'x', '--out', 'y.png', '--vis', 'mesh_strips']).vis == 'mesh_strips'
    for bad in (['--vis', 'mesh'], ['--mesh-normals', 'vertex']):
        with pytest.raises(SystemExit):
            p.parse_args(['--ckpt', 'x', '--out', 'y.gif'] + bad)


def test_entry_points_in_header_binding_and_library(tdgp):
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NAMES:
        assert re.search(rf'\bint\s+{name}\s*\(', code), name
        assert name in tdgp._lib.EXPORTS
    assert 'mesh_raster.hip' in tdgp.build.SOURCES
    assert 'atomic' in header[header.index('Mesh frames'):header.index('tdgp_mesh_visibility(')]
    lib = tdgp.build.build_native()
    out = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf' T {name}\b', out), name


def test_save_ply_colours(tdgp, tmp_path):
    g = tdgp.geometry
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.25, 2]], F)
    t = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    g.save_ply(tmp_path / 'plain.ply', v, t)
    plain = open(tmp_path / 'plain.ply', 'rb').read()
    head = (b'ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
            b'element face 2\nproperty list uchar int vertex_indices\nend_header\n')
    assert plain == head + v.tobytes() + b''.join(b'\x03' + row.tobytes() for row in t)          # the bytes of the writer before colours existed
    g.save_ply(tmp_path / 'none.ply', v, t, colours=None)
    assert open(tmp_path / 'none.ply', 'rb').read() == plain
    col = np.array([[0.0, 0.5, 1.0], [1.5, -1.0, 0.25], [0.2, 0.4, 0.6], [1, 1, 1]], F)
    want = np.array([[0, 128, 255], [255, 0, 64], [51, 102, 153], [255, 255, 255]], np.uint8)
    for given in (col, torch.tensor(col), want):
        g.save_ply(tmp_path / 'col.ply', torch.tensor(v), torch.tensor(t), colours=given)
        data = open(tmp_path / 'col.ply', 'rb').read()
        header, body = data.split(b'end_header\n', 1)
        assert b'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2' in header
        rec = np.frombuffer(body[:4 * 15], dtype=[('p', '<f4', (3,)), ('c', 'u1', (3,))])
        assert np.array_equal(rec['p'], v) and np.array_equal(rec['c'], want)
        faces = np.frombuffer(body[4 * 15:], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
        assert np.all(faces['n'] == 3) and np.array_equal(faces['i'], t)
    with pytest.raises(ValueError):
        g.save_ply(tmp_path / 'bad.ply', v, t, colours=col[:3])

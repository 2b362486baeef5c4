"""Mesh surfaces without a GPU: the properties of the contract (include/tdgp.h, "Mesh surfaces") measured on its numpy restatement
(tests/mesh_surface_reference.py) -- vertex normals of icospheres against the radial direction, Taubin smoothing of a noisy sphere, the
integer lattice with its rim -- the .obj / .ply writers with normals, and the option validation that needs no device."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_raster_reference as MR
import mesh_surface_reference as SR

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def spheres():
    return {s: MR.icosphere(s) for s in (2, 3)}


def angles(n, r):
    n, r = np.asarray(n, np.float64), np.asarray(r, np.float64)
    c = (n * r).sum(-1) / (np.linalg.norm(n, axis=-1) * np.linalg.norm(r, axis=-1))
    return np.arccos(np.clip(c, -1.0, 1.0))


# ------------------------------------------------------------------------------------------------ the table
def test_corner_table_of_a_tetrahedron_and_of_a_soup():
    start, corner, degree = SR.corner_table(SR.TETRA_T, 4)
    assert degree.tolist() == [3, 3, 3, 3] and start.tolist() == [0, 3, 6, 9, 12]
    assert corner.tolist() == [0, 3, 6, 1, 5, 9, 2, 7, 11, 4, 8, 10]
    tris = np.array([[0, 1, 2], [2, 2, 5], [0, 9, 1], [3, 3, 3], [-1, 0, 1], [2, 1, 0]], np.int32)          # V = 6: triangles 2 and 4 are skipped
    start, corner, degree = SR.corner_table(tris, 6)
    assert degree.tolist() == [2, 2, 4, 3, 0, 1] and int(start[-1]) == 12 == len(corner)
    for v in range(6):
        mine = corner[start[v]:start[v + 1]]
        assert (np.diff(mine) > 0).all() and (tris.reshape(-1)[mine] == v).all()
    assert corner[start[2]:start[3]].tolist() == [2, 3, 4, 15]


# ------------------------------------------------------------------------------------------------ normals
@pytest.mark.parametrize('subdivisions, measured', [(2, (0.024, 0.189)), (3, (0.012, 0.095))])
def test_vertex_normals_of_an_icosphere_beat_its_face_normals(spheres, subdivisions, measured):
    v, t = spheres[subdivisions]
    table = SR.corner_table(t, len(v))
    P = v.astype(np.float64)[t]
    g = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    worst_face = max(float(angles(np.repeat(g[:, None], 3, 1), P).max()), 0.0)          # a face normal against the radius at its three corners
    for weight in (0, 1):
        n = SR.vertex_normals(v, t, table[0], table[1], weight)
        assert n.dtype == F and np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=3e-7)
        ang = angles(n, v)
        print(f'icosphere({subdivisions}) weight {weight}: worst vertex-normal angle {ang.max():.4f} rad, worst face-normal angle at a corner {worst_face:.4f} rad')
        assert ang.max() < worst_face
        assert ((n.astype(np.float64) * v).sum(1) > 0).all()                             # outward
        if weight == 0:
            assert abs(ang.max() - measured[0]) < 2e-3 and abs(worst_face - measured[1]) < 2e-3


def test_vertex_normals_edge_cases():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 0, 0]], F)
    tris = np.array([[0, 1, 2], [0, 1, 4], [0, 1, 7]], np.int32)                          # a triangle, a needle (zero cross product), a skipped one
    start, corner, _ = SR.corner_table(tris, 5)
    for weight in (0, 1):
        n = SR.vertex_normals(v, tris, start, corner, weight)
        assert n[:3].tolist() == [[0, 0, 1]] * 3 and n[3].tolist() == [0, 0, 0] and n[4].tolist() == [0, 0, 0]
    # area weight follows the larger triangle, uniform weight the bisector
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 3]], F)
    tris = np.array([[0, 1, 2], [0, 3, 1]], np.int32)                                     # normals +z (area 1/2) and +y (area 3/2)
    start, corner, _ = SR.corner_table(tris, 4)
    area, uniform = (SR.vertex_normals(v, tris, start, corner, w)[0].astype(np.float64) for w in (0, 1))
    assert np.allclose(area, np.array([0, 3, 1]) / np.sqrt(10), atol=1e-7) and np.allclose(uniform, np.array([0, 1, 1]) / np.sqrt(2), atol=1e-7)
    # a caller's table with corner ids out of range and a range past the end: skipped, clamped
    bad = SR.vertex_normals(v, tris, np.array([0, 2, 4, 5, 99], np.int32), np.array([0, 3, -1, 99, 2, 4], np.int32), 0)
    assert np.isfinite(bad).all()


# ------------------------------------------------------------------------------------------------ smoothing
def test_taubin_smooths_a_noisy_sphere_and_keeps_its_size(spheres):
    for s, (v, t) in spheres.items():
        noisy = (v.astype(np.float64) * (1 + 0.02 * np.random.RandomState(0).randn(len(v), 1))).astype(F)
        table = SR.corner_table(t, len(v))
        assert not SR.boundary_vertices(t, len(v), table[0], table[1]).any()                # closed
        taubin = SR.smooth(noisy, t, iterations=10, lam=0.5, mu=-0.53, table=table)
        laplace = SR.smooth(noisy, t, iterations=10, lam=0.5, mu=None, table=table)
        radius = lambda x: np.linalg.norm(x.astype(np.float64), axis=1)                    # noqa: E731
        dev = lambda x: float(np.sqrt(((radius(x) - radius(x).mean()) ** 2).mean()))       # noqa: E731
        before, after = dev(noisy), dev(taubin)
        move_t, move_l = radius(taubin).mean() / radius(noisy).mean() - 1, radius(laplace).mean() / radius(noisy).mean() - 1
        print(f'icosphere({s}): rms radial deviation {before:.4f} -> {after:.4f}; mean radius {move_t:+.2%} (Taubin) against {move_l:+.2%} (Laplacian)')
        assert after < before
        assert abs(move_t) < abs(move_l)
        if s == 2:
            assert abs(before - 0.0204) < 5e-4 and abs(after - 0.0073) < 5e-4 and abs(move_t - 0.008) < 2e-3 and abs(move_l + 0.20) < 2e-2
        assert np.array_equal(SR.smooth(noisy, t, iterations=0), noisy)


def test_lattice_interior_stays_and_the_rim_is_the_border():
    v, t, border = SR.lattice(6)
    assert len(v) == 36 and len(t) == 50
    start, corner, degree = SR.corner_table(t, 36)
    rim = SR.boundary_vertices(t, 36, start, corner)
    assert np.array_equal(rim.astype(bool), border)
    for factor in (0.5, -0.53, 1.0):
        free = SR.smooth_step(v, t, start, corner, factor)
        assert free[~border].tobytes() == v[~border].tobytes()                              # the umbrella of an interior lattice vertex is symmetric
        assert not np.array_equal(free[border], v[border])                                  # a free rim is pulled inward
        held = SR.smooth_step(v, t, start, corner, factor, pinned=rim)
        assert held.tobytes() == v.tobytes()
    bumped = v.copy()
    bumped[14, 2] = 1.0                                                                     # an interior vertex lifted off the plane
    out = SR.smooth(bumped, t, iterations=3, fix_boundary=True)
    assert out[border].tobytes() == v[border].tobytes() and 0 < out[14, 2] < 1.0
    pinned = np.zeros(36, bool)
    pinned[14] = True
    out = SR.smooth(bumped, t, iterations=3, pinned=pinned)
    assert out[14].tobytes() == bumped[14].tobytes() and out[border].tobytes() == v[border].tobytes()


def test_rim_of_open_and_degenerate_meshes():
    start, corner, _ = SR.corner_table(SR.TETRA_T, 4)
    assert SR.boundary_vertices(SR.TETRA_T, 4, start, corner).tolist() == [0, 0, 0, 0]
    opened = SR.TETRA_T[:3]                                                                 # without the face opposite vertex 0
    start, corner, _ = SR.corner_table(opened, 4)
    assert SR.boundary_vertices(opened, 4, start, corner).tolist() == [0, 1, 1, 1]
    v, t = SR.fan(8)
    start, corner, _ = SR.corner_table(t, 9)
    assert SR.boundary_vertices(t, 9, start, corner).tolist() == [0] + [1] * 8
    twice = np.array([[0, 1, 2], [0, 1, 2], [3, 3, 4], [5, 5, 5]], np.int32)               # a duplicated triangle has no rim; (3, 3, 4) is one triangle on edge 3-4
    start, corner, _ = SR.corner_table(twice, 7)
    assert SR.boundary_vertices(twice, 7, start, corner).tolist() == [0, 0, 0, 1, 1, 0, 0]


# ------------------------------------------------------------------------------------------------ the writers
def read_ply(path):
    raw = open(path, 'rb').read()
    head, body = raw.split(b'end_header\n', 1)
    lines = head.decode('ascii').splitlines()
    nv = int([ln for ln in lines if ln.startswith('element vertex')][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith('element face')][0].split()[-1])
    props = [ln.split()[1:] for ln in lines[lines.index(f'element vertex {nv}') + 1:lines.index(f'element face {nf}')]]
    dt = np.dtype([(name, {'float': '<f4', 'uchar': 'u1'}[kind]) for kind, name in props])
    verts = np.frombuffer(body, dt, nv)
    faces = np.frombuffer(body, np.dtype([('n', 'u1'), ('i', '<i4', (3,))]), nf, offset=nv * dt.itemsize)
    assert len(body) == nv * dt.itemsize + nf * 13
    return [name for _, name in props], verts, faces


def test_writers_with_normals_read_back_and_without_them_are_unchanged(tdgp, tmp_path, spheres):
    g = tdgp.geometry
    v, t = spheres[2]
    table = SR.corner_table(t, len(v))
    n = SR.vertex_normals(v, t, table[0], table[1], 0)
    rgb = np.random.RandomState(4).rand(len(v), 3).astype(F)
    # .obj
    g.save_obj(tmp_path / 'n.obj', v, t, normals=n)
    rows = [ln.split() for ln in open(tmp_path / 'n.obj').read().splitlines()]
    got_v = np.array([[F(x) for x in r[1:]] for r in rows if r[0] == 'v'], F)
    got_n = np.array([[F(x) for x in r[1:]] for r in rows if r[0] == 'vn'], F)
    faces = [r[1:] for r in rows if r[0] == 'f']
    assert got_v.tobytes() == v.tobytes() and got_n.tobytes() == n.tobytes()
    assert [[int(x.split('//')[0]) - 1 for x in f] for f in faces] == t.tolist() and all(x.split('//')[0] == x.split('//')[1] for f in faces for x in f)
    assert [r[0] for r in rows] == ['v'] * len(v) + ['vn'] * len(v) + ['f'] * len(t)
    # .ply with normals, and with normals + colours
    g.save_ply(tmp_path / 'n.ply', torch.from_numpy(v), torch.from_numpy(t), normals=torch.from_numpy(n))
    names, pv, pf = read_ply(tmp_path / 'n.ply')
    assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    assert np.stack([pv[k] for k in 'xyz'], 1).tobytes() == v.tobytes() and np.stack([pv[k] for k in ('nx', 'ny', 'nz')], 1).tobytes() == n.tobytes()
    assert pf['i'].tolist() == t.tolist() and (pf['n'] == 3).all()
    g.save_ply(tmp_path / 'nc.ply', v, t, colours=rgb, normals=n)
    names, pv, pf = read_ply(tmp_path / 'nc.ply')
    assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue']
    assert np.stack([pv[k] for k in 'xyz'], 1).tobytes() == v.tobytes() and np.stack([pv[k] for k in ('nx', 'ny', 'nz')], 1).tobytes() == n.tobytes()
    assert np.array_equal(np.stack([pv[k] for k in ('red', 'green', 'blue')], 1), np.rint(rgb.astype(np.float64) * 255).astype(np.uint8))
    assert pf['i'].tolist() == t.tolist()
    # without normals: the bytes of the writers as they were (the format written out here by hand)
    g.save_obj(tmp_path / 'p.obj', v, t)
    text = lambda x: np.format_float_positional(x, unique=True, trim='-')                  # noqa: E731
    want = ''.join(f'v {text(x)} {text(y)} {text(z)}\n' for x, y, z in v) + ''.join(f'f {a + 1} {b + 1} {c + 1}\n' for a, b, c in t.tolist())
    assert open(tmp_path / 'p.obj').read() == want
    g.save_ply(tmp_path / 'p.ply', v, t)
    faces = np.empty(len(t), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    faces['n'], faces['i'] = 3, t
    header = (f'ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n'
              f'element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n')
    assert open(tmp_path / 'p.ply', 'rb').read() == header.encode('ascii') + v.tobytes() + faces.tobytes()
    g.save_ply(tmp_path / 'c.ply', v, t, colours=rgb)
    rec = np.empty(len(v), dtype=[('p', '<f4', (3,)), ('c', 'u1', (3,))])
    rec['p'], rec['c'] = v, np.rint(rgb.astype(np.float64) * 255).astype(np.uint8)
    header = header.replace('element face', 'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face')
    assert open(tmp_path / 'c.ply', 'rb').read() == header.encode('ascii') + rec.tobytes() + faces.tobytes()
    with pytest.raises(ValueError, match='normals'):
        g.save_ply(tmp_path / 'bad.ply', v, t, normals=n[:-1])
    with pytest.raises(ValueError, match='normals'):
        g.save_obj(tmp_path / 'bad.obj', v, t, normals=n[:, :2])


# ------------------------------------------------------------------------------------------------ options, no device
def _cams(tdgp, n):
    return tdgp.generator.TensorGroup(angles=torch.zeros(n, 3), fov=torch.full([n], 20.0), radius=torch.ones(n), look_at=torch.zeros(n, 3))


def test_option_validation_needs_no_device(tdgp):
    M, S = tdgp.mesh, tdgp.mesh_surface
    assert M.NORMALS == ('face', 'field', 'vertex')
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    cams = _cams(tdgp, 2)
    with pytest.raises(ValueError, match='vertex_colours'):
        M.render_mesh_views(v, t, cams, 16, normals='vertex', mode='colour')
    with pytest.raises(ValueError, match='vertex_normals'):
        M.render_mesh_views(v, t, cams, 16, normals='face', vertex_normals=torch.zeros(4, 3))
    with pytest.raises(ValueError, match='vertex_normals'):
        M.render_mesh_views(v, t, cams, 16, normals='vertex', vertex_normals=torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='vertex_normals'):
        M.render_mesh_views(v, t, cams, 16, normals='vertex', vertex_normals=np.zeros((4, 3), F))
    with pytest.raises(ValueError, match='normals'):
        M.render_mesh_views(v, t, cams, 16, normals='smooth')
    with pytest.raises(ValueError, match="normals='vertex' takes a mesh on the GPU"):
        M.render_mesh_views(v, t, cams, 16, normals='vertex')                              # well-formed, on the CPU: this mode has no CPU path
    with pytest.raises(TypeError):
        M.render_mesh_views(v.numpy(), t, cams, 16, normals='vertex')
    with pytest.raises(ValueError, match='int32'):
        S.corner_table(t.long(), 4)
    with pytest.raises(ValueError, match=r'\[T,3\]'):
        S.corner_table(t.reshape(3, 2), 4)
    with pytest.raises(TypeError):
        S.corner_table(t.numpy(), 4)
    with pytest.raises(ValueError, match='num_vertices'):
        S.corner_table(t, -1)
    with pytest.raises(ValueError, match='fp32'):
        S.vertex_normals(v.double(), t)
    with pytest.raises(ValueError, match='weight'):
        S.vertex_normals(v, t, weight='angle')
    with pytest.raises(ValueError, match='iterations'):
        S.smooth(v, t, iterations=-1)
    with pytest.raises(ValueError, match='finite'):
        S.smooth(v, t, lam=float('nan'))
    with pytest.raises(RuntimeError, match='GPU'):
        S.smooth(v, t)
    with pytest.raises(RuntimeError, match='GPU'):
        S.boundary_vertices(t, 4)


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_ms_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_parse_the_new_flags():
    ex = _tool('extract_geometry')
    a = ex.parse_args(['--seeds', '0'])
    assert ex.smooth_options(a) is None and not hasattr(a, 'vertex_normals') and not hasattr(a, 'smooth_iters')
    a = ex.parse_args(['--seeds', '0', '--smooth-iters', '7', '--vertex-normals'])
    assert ex.smooth_options(a) == dict(iterations=7, lam=0.5, mu=-0.53, fix_boundary=True) and a.vertex_normals is True
    a = ex.parse_args(['--seeds', '0', '--smooth-iters', '2', '--smooth-lambda', '0.3', '--smooth-mu', '-0.31', '--smooth-free-boundary'])
    assert ex.smooth_options(a) == dict(iterations=2, lam=0.3, mu=-0.31, fix_boundary=False)
    rt = _tool('render_trajectory')
    base = ['--ckpt', 'dir', '--out', 'x.npy', '--vis', 'mesh_grid']
    a = rt.build_parser().parse_args(base + ['--mesh-normals', 'vertex', '--mesh-smooth-iters', '3'])
    opts = rt.mesh_options(a)
    assert opts['normals'] == 'vertex' and opts['smooth'] == dict(iterations=3)
    assert rt.mesh_options(rt.build_parser().parse_args(base))['smooth'] is None
    for bad in (['--mesh-normals', 'vertex'], ['--mesh-smooth-iters', '2'], ['--vis', 'mesh_grid', '--mesh-smooth-iters', '-1']):      # surface options without mesh frames
        with pytest.raises(SystemExit):
            rt.build_parser().parse_args(['--ckpt', 'dir', '--out', 'x.npy'] + bad)

"""Mesh simplification without a GPU: the properties of the numpy restatement (tests/mesh_simplify_reference.py) that make it worth being the
yardstick -- quadric placement keeps the faces, edges and corners of a box that cell means round off; the output is a valid indexed mesh --
and the host logic of 3dgp_amd/mesh_simplify.py: argument validation before any launch, the ladder of `cell_for_triangles`, the `simplify=`
option of the drivers, the two command lines' usage errors, the ABI."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import mesh_raster_reference as MR
import mesh_simplify_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ['tdgp_mesh_cluster_keys', 'tdgp_mesh_cluster_ids_workspace_bytes', 'tdgp_mesh_cluster_ids', 'tdgp_mesh_cluster_triangles_relabel',
       'tdgp_mesh_cluster_triangles_workspace_bytes', 'tdgp_mesh_cluster_triangles_count', 'tdgp_mesh_cluster_triangles_emit', 'tdgp_mesh_cluster_place',
       'tdgp_mesh_cluster_attribute']


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_simplify_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def valid_mesh(s, T):
    """Triangles index [0, C), none is degenerate, none repeats up to rotation, triangle_map is strictly increasing inside [0, T)."""
    C = len(s.vertices)
    t = np.asarray(s.triangles)
    assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 3 and len(s.triangle_map) == len(t)
    if len(t):
        assert t.min() >= 0 and t.max() < C
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
        assert len({R.rotate(x) for x in t}) == len(t)
        m = np.asarray(s.triangle_map, np.int64)
        assert (np.diff(m) > 0).all() and m[0] >= 0 and m[-1] < T


def test_quadric_placement_keeps_a_box_and_means_do_not():
    """The unit-tessellated 12^3 box shifted off the lattice of cell 4: 1728 -> 108 triangles.  The box's planes are exact in fp32 and the
    double chain's error is far below an fp32 ulp, so a quadric vertex is the exact point rounded once: at most 0.87 ulp of the largest
    coordinate in norm; 2 ulps are allowed."""
    v, t, lo, hi = R.box()
    assert len(t) == 1728 and len(v) == 866
    q, m = R.simplify(v, t, 4.0, placement='quadric'), R.simplify(v, t, 4.0, placement='mean')
    assert len(q.triangles) == len(m.triangles) == 108 and len(q.vertices) == 56
    ulp = float(np.spacing(F(np.abs(np.concatenate([lo, hi])).max())))
    d = R.box_surface_distance(q.vertices, lo, hi)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    to_corner = np.sqrt(((corners[:, None, :] - q.vertices[None].astype(np.float64)) ** 2).sum(-1)).min(axis=1)
    print(f'quadric: worst distance from the surface {d.max():.3g}, of a corner from the nearest vertex {to_corner.max():.3g}, ulp {ulp:.3g}; '
          f'mean: {R.box_surface_distance(m.vertices, lo, hi).max():.4g}; fallbacks {int(q.fallback.sum())}')
    assert d.max() <= 2 * ulp and to_corner.max() <= 2 * ulp
    assert not q.fallback.any()
    assert R.box_surface_distance(m.vertices, lo, hi).max() > 1.0
    for s in (q, m):
        valid_mesh(s, len(t))
    assert np.array_equal(q.cluster, m.cluster) and np.array_equal(q.triangles, m.triangles)


def test_quadric_placement_keeps_a_rotated_box():
    """The same box turned off the axes (the Jacobi rotations have work to do): vertices are rounded to fp32, so the planes are exact only to
    about an ulp of the coordinates (1e-6) and the placement to that times the conditioning of a cluster's planes; 1e-4 is allowed.  Every
    corner of the box has an output vertex that close to it, and so is every vertex that did not take the fallback (an edge or face cluster
    whose optimum leaves its cell takes its mean: the contract's fallback)."""
    v, t, lo, hi = R.box()
    a, b = 0.4, 0.7
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    back = lambda p: np.asarray(p, np.float64) @ rot                                                  # noqa: E731  (rows: rot^T applied)
    vr = (v.astype(np.float64) @ rot.T).astype(F)
    q = R.simplify(vr, t, 4.0, placement='quadric')
    dq = R.box_surface_distance(back(q.vertices), lo, hi)
    print(f'rotated box: quadric worst without fallback {dq[q.fallback == 0].max():.3g} ({int(q.fallback.sum())} fallbacks of {len(q.vertices)})')
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    to_corner = np.sqrt(((corners[:, None, :] - back(q.vertices)[None]) ** 2).sum(-1)).min(axis=1)
    assert to_corner.max() < 1e-4 and dq[q.fallback == 0].max() < 1e-4 and q.fallback.sum() < len(q.vertices) // 4
    valid_mesh(q, len(t))


def test_the_fixed_jacobi_diagonalises():
    """8 cyclic sweeps on symmetric 3x3 matrices of rank 1, 2 and 3 (sums of n n^T, as the quadrics are): eigenvalues against numpy's to
    1e-12 of the largest, orthonormal eigenvectors, A u = l u."""
    rs = np.random.RandomState(0)
    for rank in (1, 2, 3, 3, 3):
        n = rs.randn(rank, 3) * 10.0 ** rs.randint(-3, 4)
        A = sum(np.outer(x, x) for x in n)
        a, u = [[np.float64(x) for x in row] for row in A], [[np.float64(i == j) for j in range(3)] for i in range(3)]
        with np.errstate(all='ignore'):                                                           # theta * theta may overflow: t is then 0, as it should be
            for _ in range(8):
                R._jacobi_rotate(a, u, 0, 1, 2)
                R._jacobi_rotate(a, u, 0, 2, 1)
                R._jacobi_rotate(a, u, 1, 2, 0)
        lam, U = np.array([a[i][i] for i in range(3)]), np.array(u)
        scale = np.abs(np.linalg.eigvalsh(A)).max()
        assert np.abs(np.sort(lam) - np.linalg.eigvalsh(A)).max() <= 1e-12 * scale
        assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-14 and np.abs(A @ U - U * lam).max() <= 1e-12 * scale


def test_clusters_and_triangles_of_the_restatement():
    v, t = MR.icosphere(2)
    s = R.simplify(v, t, 0.5, attributes=(v * 2,))
    C = len(s.key)
    assert 8 < C < len(v) and (np.diff(s.key) > 0).all() and s.start[0] == 0 and s.start[-1] == len(v)
    for c in range(C):
        members = s.order[s.start[c]:s.start[c + 1]]
        assert (np.diff(members) > 0).all() and (s.cluster[members] == c).all()
    valid_mesh(s, len(t))
    assert 0 < len(s.triangles) < len(t)
    assert np.abs(s.attributes[0] - 2 * R.simplify(v, t, 0.5, placement='mean').vertices).max() < 1e-6
    # keys: a negative cell index, a vertex on a lattice plane, NaN, and the two ends of the lattice
    pts = np.array([[-0.5, 0, 0], [2.0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [2.0 ** 21 - 2.0, 0, 0], [2.0 ** 21, 0, 0], [-2.0 ** 21, 0, 0], [-2.0 ** 21 - 2, 0, 0]], F)
    key = R.cell_keys(pts, 2.0)
    assert key.tolist()[2:4] == [-1, -1] and key[5] == -1 and key[7] == -1 and (key[[0, 1, 4, 6]] >= 0).all()
    mid = (2 ** 20 * 2 ** 21 + 2 ** 20) * 2 ** 21
    assert key[0] == mid + 2 ** 20 - 1 and key[1] == mid + 2 ** 20 + 1 and key[4] == mid + 2 ** 21 - 1 and key[6] == mid
    # dedup: the same triple twice, a rotation of it and its flip -> the first and the flip
    sq = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F)
    tt = np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0], [0, 2, 1]], np.int32)
    assert R.simplify(sq, tt, 1.0).triangle_map.tolist() == [0, 3] and R.simplify(sq, tt, 1.0, dedup=False).triangle_map.tolist() == [0, 1, 2, 3]


def test_arguments_are_checked_before_any_launch(tdgp):
    S = tdgp.mesh_simplify
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    bad = [lambda: S.simplify(v.double(), t, 1.0), lambda: S.simplify(v[:, :2], t, 1.0), lambda: S.simplify(v, t.long(), 1.0), lambda: S.simplify(v, t.reshape(6), 1.0),
           lambda: S.simplify(v, t, 0.0), lambda: S.simplify(v, t, -1.0), lambda: S.simplify(v, t, float('nan')), lambda: S.simplify(v, t, float('inf')),
           lambda: S.simplify(v, t, (1.0, 2.0)), lambda: S.simplify(v, t, (1.0, 0.0, 1.0)), lambda: S.simplify(v, t, 1.0, origin=(0, float('inf'), 0)),
           lambda: S.simplify(v, t, 1.0, placement='median'), lambda: S.simplify(v, t, 1.0, rank_tol=-1.0), lambda: S.cluster_vertices(v.half(), 1.0),
           lambda: S.cluster_vertices(v, 'wide'), lambda: S.cell_for_triangles(v, t, -1), lambda: S.cell_for_triangles(v, t, 10, cell_min=0.0),
           lambda: S.cell_for_triangles(v, t, 10, steps=0), lambda: S.check_options(dict(cell=2.0, max_triangles=100)), lambda: S.check_options(dict()),
           lambda: S.check_options(dict(cell=2.0, steps=3)), lambda: S.check_options(dict(cell=2.0, colour='red')), lambda: S.check_options(dict(cell=-2.0)),
           lambda: S.check_options(dict(max_triangles=1.5)), lambda: S.check_options(dict(cell=1.0, placement='best')),
           lambda: tdgp.geometry.extract_geometry(None, None, simplify=dict(cell=2.0, max_triangles=100))]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'call {k} did not raise')
    with pytest.raises(TypeError):
        S.check_options(2.0)
    for call in (lambda: S.simplify(v, t, 1.0), lambda: S.cluster_vertices(v, 1.0), lambda: S.cell_for_triangles(v, t, 10)):
        with pytest.raises(RuntimeError, match='GPU'):                                            # well-formed, on the host: the kernels have no CPU path
            call()
    assert S.check_options(dict(cell=(2, 3, 4), placement='mean', dedup=False)) == dict(cell=(2, 3, 4), placement='mean', dedup=False)
    assert S.check_options(dict(max_triangles=1000, cell_min=1.5, steps=4))['steps'] == 4
    c = tdgp.geometry.MeshCount(7, 9, 30)
    assert c == (7, 9) and tuple(c) == (7, 9) and c.triangles_before == 30 and tdgp.geometry.MeshCount(7, 9).triangles_before == 9


def test_cell_for_triangles_walks_the_ladder(tdgp, monkeypatch):
    """The host logic of `cell_for_triangles` on counts taken from the restatement (the device count stands behind `count_triangles`)."""
    S = tdgp.mesh_simplify
    v, t = MR.icosphere(2)
    cells = R.ladder(0.125, 8)
    assert S.ladder(0.125, 8) == cells and cells[2] == 0.25 and abs(cells[1] - 0.125 * 2 ** 0.5) < 1e-15
    counts = [R.count_triangles(v, t, c) for c in cells]
    print('cells', [round(c, 4) for c in cells], 'triangles', counts)
    assert counts[0] == len(t) and counts[-1] < 40 and len(set(counts)) >= 5
    asked = []

    def fake(vertices, triangles, cell, origin=(0, 0, 0), dedup=True):
        asked.append(cell)
        return R.count_triangles(vertices.numpy(), triangles.numpy(), cell, origin, dedup)

    monkeypatch.setattr(S, 'count_triangles', fake)
    tv, tt = torch.as_tensor(v), torch.as_tensor(t)
    for j in (0, 3, 5, 7):
        want = next(i for i, c in enumerate(counts) if c <= counts[j])                            # the FIRST rung that is small enough
        asked.clear()
        assert S.cell_for_triangles(tv, tt, counts[j], cell_min=0.125, steps=8) == cells[want] and asked == cells[:want + 1]
        assert R.cell_for_triangles(v, t, counts[j], 0.125, 8)[0] == cells[want]
    with pytest.raises(ValueError, match=f'the last leaves {counts[3]}'):
        S.cell_for_triangles(tv, tt, counts[3] - 1, cell_min=0.125, steps=4)


def test_tools_usage_errors(capsys):
    ex, rt = _tool('extract_geometry'), _tool('render_trajectory')
    base = ['--seeds', '0']
    a = ex.parse_args(base)
    assert ex.simplify_options(a) is None and not any(k.startswith('simplify') for k in vars(a))
    assert ex.simplify_options(ex.parse_args(base + ['--simplify-cell', '2.5'])) == dict(cell=2.5, placement='quadric')
    assert ex.simplify_options(ex.parse_args(base + ['--simplify-max-triangles', '1000', '--simplify-placement', 'mean'])) == dict(max_triangles=1000, placement='mean')
    for extra in (['--simplify-cell', '2', '--simplify-max-triangles', '1000'], ['--simplify-cell', '0'], ['--simplify-cell', 'nan'], ['--simplify-max-triangles', '-4'],
                  ['--simplify-placement', 'mean'], ['--simplify-cell', '2', '--simplify-placement', 'median']):
        with pytest.raises(SystemExit):
            ex.parse_args(base + extra)
    p = rt.build_parser()
    base = ['--ckpt', 'x', '--out', 'y.npy']
    a = p.parse_args(base + ['--vis', 'mesh_grid', '--mesh-simplify-cell', '3'])
    assert rt.mesh_options(a)['simplify'] == dict(cell=3.0) and rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_strips']))['simplify'] is None
    for extra in (['--mesh-simplify-cell', '2'], ['--vis', 'shape_grid', '--mesh-simplify-cell', '2'], ['--vis', 'mesh_grid', '--mesh-simplify-cell', '0'],
                  ['--vis', 'mesh_grid', '--mesh-simplify-cell', 'inf']):
        with pytest.raises(SystemExit):
            p.parse_args(base + extra)
    capsys.readouterr()


def test_entry_points_are_declared_bound_and_refuse_what_they_cannot_index(tdgp):
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    for name in NEW:
        assert re.search(rf'\b{name}\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)) and name in tdgp._lib.EXPORTS
    assert 'mesh_simplify.hip' in tdgp.build.SOURCES
    lib = tdgp._lib.load()
    assert lib.tdgp_mesh_cluster_ids_workspace_bytes(2 ** 31 - 1) == -1 and lib.tdgp_mesh_cluster_ids_workspace_bytes(-1) == -1
    assert lib.tdgp_mesh_cluster_triangles_workspace_bytes(2 ** 31 // 3 + 1) == -1
    assert lib.tdgp_mesh_cluster_ids_workspace_bytes(0) == 64 and lib.tdgp_mesh_cluster_ids_workspace_bytes(257) == 128
    assert lib.tdgp_mesh_cluster_triangles_workspace_bytes(2 ** 31 // 3) > 0
    # the argument checks of the C side come before any launch: they answer without a device
    import ctypes
    three = ctypes.c_double * 3
    assert lib.tdgp_mesh_cluster_keys(None, 4, three(1, 0, 1), three(0, 0, 0), None, None) == -1 and b'cell' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_cluster_keys(None, 2 ** 31 - 1, three(1, 1, 1), three(0, 0, 0), None, None) == -1 and b'2^31 - 2' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_cluster_place(None, 4, None, None, None, 5, three(1, 1, 1), three(0, 0, 0), None, 0, None, None, 0, 1e-3, None, None) == -1
    assert lib.tdgp_mesh_cluster_place(None, 4, None, None, None, 2, three(1, 1, 1), three(0, 0, 0), None, 0, None, None, 2, 1e-3, None, None) == -1
    assert lib.tdgp_mesh_cluster_attribute(None, 65, 4, None, None, 2, None, None) == -1 and b'channels' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_cluster_triangles_emit(None, 4, None, None, 0, None, 5, None, None) == -1

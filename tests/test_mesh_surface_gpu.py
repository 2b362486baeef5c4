"""Mesh surfaces on the GPU: tdgp_mesh_corner_table / _vertex_normals / _boundary_vertices / _smooth_step / _interp_normals bit for bit against the
numpy restatement of their contracts (tests/mesh_surface_reference.py) on closed, open, degenerate and marching-cubes meshes at the block
edges of the kernels, `normals='vertex'` frames against resolve -> interp -> shade, and the `smooth=` / `normals='vertex'` options of
geometry.extract_geometry, mesh.render_mesh_frames and the two command lines on a seeded config_tiny scene."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_components_reference as CR
import mesh_raster_reference as MR
import mesh_surface_reference as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADE = dict(ambient=0.25, albedo=(0.9, 0.7, 0.5), background=(1.0, 0.5, -1.0))


def T(a):
    if isinstance(a, np.ndarray) and not a.flags.writeable:              # the shared, read-only test meshes
        a = a.copy()
    return torch.as_tensor(a).to(DEV)


def H(t):
    return t.detach().cpu().numpy()


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        g, w = (a.view(np.uint32) if a.dtype == np.float32 else a for a in (got, want))
        bad = np.argwhere(g != w)
        first = tuple(bad[0]) if len(bad) else ()
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}')


# ------------------------------------------------------------------------------------------------ the meshes
def _random_vertices(V, seed):
    return (np.random.RandomState(seed).randn(V, 3) * 2).astype(F)


def _mc_mesh():
    tdgp = importlib.import_module('3dgp_amd')
    v, t = tdgp.geometry.marching_cubes(T(CR.speck_volume(24)), 0.0)
    return H(v), H(t)


def _soup():
    """Random triples over 40 of 42 vertices (41 and 42 stay unnamed), then indices out of range, degenerate triangles and a duplicate."""
    t = CR.soup(40, 60, 7)
    extra = np.array([[0, 1, 42], [3, -1, 5], [2 ** 31 - 1, 0, 1], [7, 7, 9], [11, 11, 11], [4, 9, 4], t[5], t[5], [0, 1, 2], [2, 1, 0]], np.int32)
    return _random_vertices(42, 21), np.concatenate([t[:30], extra, t[30:]]).astype(np.int32)


MESHES = {
    'tetrahedron': lambda: (SR.TETRA_V, SR.TETRA_T),
    'icosphere': lambda: MR.icosphere(2),
    'lattice': lambda: SR.lattice(6)[:2],
    'soup': _soup,
    'fan of 4096': lambda: SR.fan(4096),
    'marching cubes': _mc_mesh,
}
for _V in (255, 256, 257, 1023, 1024, 1025):                             # one block of vertices less one / exactly / plus one, and four blocks likewise
    MESHES[f'strip V={_V}'] = lambda V=_V: (_random_vertices(V, V), CR.strip(V - 2)[0])


@functools.lru_cache(maxsize=None)
def named_mesh(name):
    """(vertices, triangles, reference dict): computed once, shared, never written."""
    v, t = MESHES[name]()
    v, t = np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32)
    V = len(v)
    start, corner, degree = SR.corner_table(t, V)
    pinned = np.random.RandomState(V).rand(V) < 0.3
    ref = dict(start=start, corner=corner, degree=degree, rim=SR.boundary_vertices(t, V, start, corner), pinned=pinned)
    table = (start, corner, degree)
    for w, name_w in ((0, 'area'), (1, 'uniform')):
        ref[name_w] = SR.vertex_normals(v, t, start, corner, w)
    for f in (0.5, -0.53):
        ref['step', f] = SR.smooth_step(v, t, start, corner, f)
    ref['smooth3'] = SR.smooth(v, t, iterations=3, table=table)
    ref['smooth3 pinned'] = SR.smooth(v, t, iterations=3, pinned=pinned, fix_boundary=False, table=table)
    for a in [v, t] + [x for x in ref.values()]:
        a.setflags(write=False)
    return v, t, ref


def check_mesh(tdgp, v, t, ref, what):
    S = tdgp.mesh_surface
    tv, tt = T(v), T(t)
    V = len(v)
    table = S.corner_table(tt, V)
    assert isinstance(table, S.CornerTable) and table._fields == ('start', 'corner', 'degree')
    same_bytes(H(table.degree), ref['degree'], 'degree ' + what)
    same_bytes(H(table.start), ref['start'], 'start ' + what)
    same_bytes(H(table.corner), ref['corner'], 'corner ' + what)
    again = S.corner_table(tt, V)
    assert all(torch.equal(a, b) for a, b in zip(table, again)), 'the table differs between two calls'
    for weight in ('area', 'uniform'):
        n = S.vertex_normals(tv, tt, weight=weight, table=table)
        same_bytes(H(n), ref[weight], f'{weight} normals {what}')
        assert torch.equal(n, S.vertex_normals(tv, tt, weight=weight)), 'normals with and without a given table differ'
    rim = S.boundary_vertices(tt, V, table=table)
    assert rim.dtype == torch.bool
    same_bytes(H(rim).astype(np.uint8), ref['rim'], 'rim ' + what)
    for f in (0.5, -0.53):
        one = S.smooth(tv, tt, iterations=1, lam=f, mu=None, fix_boundary=False, table=table)
        same_bytes(H(one), ref['step', f], f'one step of factor {f} {what}')
    before = tv.clone()
    out = S.smooth(tv, tt, iterations=3)
    same_bytes(H(out), ref['smooth3'], 'smooth(iterations=3) ' + what)
    assert torch.equal(out, S.smooth(tv, tt, iterations=3, table=table)), 'two calls of smooth differ'
    out = S.smooth(tv, tt, iterations=3, pinned=T(ref['pinned']), fix_boundary=False, table=table)
    same_bytes(H(out), ref['smooth3 pinned'], 'smooth(iterations=3, pinned) ' + what)
    assert torch.equal(tv, before), 'smooth wrote its input'
    same = S.smooth(tv, tt, iterations=0)
    assert torch.equal(same, tv) and same.data_ptr() != tv.data_ptr()
    return table


@pytest.mark.parametrize('name', list(MESHES))
def test_bit_for_bit(tdgp, name):
    v, t, ref = named_mesh(name)
    table = check_mesh(tdgp, v, t, ref, name)
    if name == 'fan of 4096':
        assert int(table.degree[0]) == 4096 and H(table.corner[:4096]).tolist() == list(range(0, 3 * 4096, 3))
        assert ref['rim'].tolist() == [0] + [1] * 4096
    if name == 'lattice':
        assert np.array_equal(ref['rim'].astype(bool), SR.lattice(6)[2])
        assert ref['step', 0.5][~SR.lattice(6)[2]].tobytes() == v[~SR.lattice(6)[2]].tobytes()
    if name == 'soup':
        assert ref['degree'][40:].tolist() == [0, 0] and int(ref['start'][-1]) == 3 * (len(t) - 3)
    if name in ('icosphere', 'tetrahedron', 'marching cubes'):
        assert not ref['rim'].any()                                       # closed surfaces
    if name == 'marching cubes':
        assert len(v) > 256 and (ref['degree'] >= 3).all()


def test_more_than_1024_blocks_of_vertices(tdgp):
    """The one-block scan of the block sums takes runs of 2 sums per thread from 1025 blocks on: a strip of 257 triangles on 1024 * 256 + 257
    vertices.  The restatement is local, so it runs on the first 300 vertices; every other vertex has no corner: degree 0, normal 0, not on a
    rim, copied bit for bit by a step."""
    S = tdgp.mesh_surface
    nt, V, head = 257, 1024 * 256 + 257, 300
    assert -(-V // 256) == 1026
    t, _ = CR.strip(nt, V=V)
    v = _random_vertices(V, 5)
    start, corner, degree = SR.corner_table(t, head)
    tv, tt = T(v), T(t)
    table = S.corner_table(tt, V)
    same_bytes(H(table.degree), np.concatenate([degree, np.zeros(V - head, np.int32)]), 'degree')
    same_bytes(H(table.start), np.concatenate([start, np.full(V - head, start[-1], np.int32)]), 'start')
    same_bytes(H(table.corner), corner, 'corner')
    pad = lambda a, rest: np.concatenate([a, rest])                        # noqa: E731
    same_bytes(H(S.vertex_normals(tv, tt, table=table)), pad(SR.vertex_normals(v[:head], t, start, corner, 0), np.zeros((V - head, 3), F)), 'normals')
    same_bytes(H(S.boundary_vertices(tt, V, table=table)).astype(np.uint8), pad(SR.boundary_vertices(t, head, start, corner), np.zeros(V - head, np.uint8)), 'rim')
    same_bytes(H(S.smooth(tv, tt, iterations=2, table=table)), pad(SR.smooth(v[:head], t, iterations=2), v[head:]), 'smooth')


def test_a_callers_table_is_clamped_and_skipped(tdgp):
    """Corner ids outside [0, 3T), corners of a skipped triangle and ranges past the end of `corner`: nothing is dereferenced, the restatement's bytes."""
    S = tdgp.mesh_surface
    v = _random_vertices(5, 3)
    t = np.array([[0, 1, 2], [0, 3, 1], [2, 9, 4]], np.int32)
    start = np.array([0, 3, 5, 8, 7, 50], np.int32)                        # a range running backwards, one running past the end, start[V] beyond 3T
    corner = np.array([0, 3, -1, 99, 2, 4, 6, 8, 1], np.int32)
    table = S.CornerTable(T(start), T(corner), None)
    tv, tt = T(v), T(t)
    for w, name in ((0, 'area'), (1, 'uniform')):
        same_bytes(H(S.vertex_normals(tv, tt, weight=name, table=table)), SR.vertex_normals(v, t, start, corner, w), name)
    same_bytes(H(S.boundary_vertices(tt, 5, table=table)).astype(np.uint8), SR.boundary_vertices(t, 5, start, corner), 'rim')
    same_bytes(H(S.smooth(tv, tt, iterations=1, mu=None, fix_boundary=False, table=table)), SR.smooth_step(v, t, start, corner, 0.5), 'step')


def test_empty_meshes_are_no_ops_and_bad_arguments_raise_before_any_launch(tdgp):
    S = tdgp.mesh_surface
    e_v, e_t = torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV)
    table = S.corner_table(e_t, 0)
    assert H(table.start).tolist() == [0] and tuple(table.corner.shape) == (0,) and tuple(table.degree.shape) == (0,)
    assert tuple(S.vertex_normals(e_v, e_t).shape) == (0, 3) and tuple(S.boundary_vertices(e_t, 0).shape) == (0,) and tuple(S.smooth(e_v, e_t).shape) == (0, 3)
    v = T(_random_vertices(7, 1))
    table = S.corner_table(e_t, 7)                                         # vertices without triangles
    assert H(table.start).tolist() == [0] * 8 and H(table.degree).tolist() == [0] * 7 and tuple(table.corner.shape) == (0,)
    assert not S.vertex_normals(v, e_t).any() and not S.boundary_vertices(e_t, 7).any() and torch.equal(S.smooth(v, e_t, iterations=2), v)
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    for call in (lambda: S.corner_table(t.long(), 7), lambda: S.corner_table(t.reshape(3), 7), lambda: S.vertex_normals(v.double(), t),
                 lambda: S.vertex_normals(v[:, :2], t), lambda: S.smooth(v, t.to(torch.int16)), lambda: S.smooth(v, t, pinned=torch.zeros(6, dtype=torch.bool, device=DEV)),
                 lambda: S.smooth(v, t, pinned=torch.zeros(7, device=DEV)), lambda: S.vertex_normals(v, t, table=S.CornerTable(table.start[:-1], table.corner, None)),
                 lambda: S.vertex_normals(v, t, table=S.CornerTable(table.start.long(), table.corner, None)), lambda: S.boundary_vertices(t, 2 ** 31),
                 lambda: S.vertex_normals(v, t, weight='angle')):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match='GPU'):
        S.vertex_normals(v.cpu(), t.cpu())
    lib = tdgp._lib
    assert lib.load().tdgp_mesh_corner_table_workspace_bytes(2 ** 31 // 3 + 1, 4) == -1 and lib.load().tdgp_mesh_corner_table_workspace_bytes(4, 2 ** 31 - 1) == -1
    with pytest.raises(RuntimeError, match='overlap'):                     # the C side refuses an in-place step
        full = S.corner_table(t, 7)
        lib.call('tdgp_mesh_smooth_step', v.data_ptr(), t.data_ptr(), 1, 7, full.start.data_ptr(), full.corner.data_ptr(), 0.5, None, v.data_ptr(), lib.stream_of(v))


# ------------------------------------------------------------------------------------------------ frames
def cameras(tdgp, n=3):
    angles = np.array([[0.3, 1.3, 0.0], [-0.5, 1.8, 0.0], [1.1, 1.5, 0.0]], F)[:n]
    return tdgp.generator.TensorGroup(angles=T(angles), fov=T(np.array([40.0, 50.0, 60.0], F)[:n]), radius=T(np.array([1.0, 1.1, 0.9], F)[:n]),
                                      look_at=T(np.zeros((n, 3), F)))


@pytest.fixture(scope='module')
def sphere_frames(tdgp):
    """icosphere(3) of radius 0.3 at 32 x 32 under 3 cameras: the restatement's frames in the three modes, computed once."""
    res = 32
    v, t = MR.icosphere(3, 0.3)
    rgbv = np.random.RandomState(3).rand(len(v), 3).astype(F)
    cams = cameras(tdgp)
    c2w = tdgp.renderer.compute_cam2world_matrix(cams)
    focal = tdgp.mesh.focal_lengths(cams.fov, 3, DEV)
    ray_o, ray_d = tdgp.renderer.sample_rays(c2w, fov=cams.fov, resolution=(res, res))
    start, corner, _ = SR.corner_table(t, len(v))
    vn = SR.vertex_normals(v, t, start, corner, 0)
    want = {mode: SR.frames(v, t, H(c2w), H(focal), H(ray_o), H(ray_d), res, res, 0.1, 'none', 1.0 / 64, 2.5, vn, rgbv, mode, **SHADE)
            for mode in ('shaded', 'normals', 'colour')}
    face = MR.frames(v, t, H(c2w), H(focal), H(ray_o), H(ray_d), res, res, 0.1, 'none', 1.0 / 64, 2.5, rgbv, 'shaded', **SHADE)
    return dict(v=v, t=t, rgbv=rgbv, cams=cams, res=res, vn=vn, want=want, face=face, ray_o=ray_o, ray_d=ray_d)


def test_vertex_normal_frames_bit_for_bit(tdgp, sphere_frames):
    sf = sphere_frames
    M = tdgp.mesh
    tv, tt, R = T(sf['v']), T(sf['t']), sf['res'] ** 2
    kw = dict(near=0.1, t_miss=2.5, step=1.0 / 64, vertex_colours=T(sf['rgbv']), **SHADE)
    for mode, want in sf['want'].items():
        got = M.render_mesh_views(tv, tt, sf['cams'], sf['res'], mode=mode, normals='vertex', **kw)
        for k, wk in (('rgb', 'rgb'), ('normal', 'normal'), ('depth', 't_hit'), ('status', 'status'), ('tri', 'tri')):
            same_bytes(H(getattr(got, k)).reshape(want[wk].shape), want[wk], f'{k} ({mode})')
        chunked = M.render_mesh_views(tv, tt, sf['cams'], sf['res'], mode=mode, normals='vertex', max_rays_per_call=R, **kw)
        given = M.render_mesh_views(tv, tt, sf['cams'], sf['res'], mode=mode, normals='vertex', vertex_normals=T(sf['vn']), **kw)
        for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
            assert torch.equal(getattr(chunked, k), getattr(got, k)), f'{k} differs under camera chunking ({mode})'
            assert torch.equal(getattr(given, k), getattr(got, k)), f'{k} differs with the normals handed in ({mode})'
    want = sf['want']['shaded']
    hit = want['status'] == 1
    assert 0.05 < hit.mean() < 0.9
    assert (want['normal'][hit] != want['face_normal'][hit]).any(axis=1).mean() > 0.9          # smooth normals are not the facets'
    x = H(sf['ray_o']).reshape(-1, 3)[hit] + H(sf['ray_d']).reshape(-1, 3)[hit] * want['t_hit'][hit, None]
    cos = lambda n: (n.astype(np.float64) * x).sum(1) / np.linalg.norm(x, axis=1)             # noqa: E731
    print(f'worst angle to the radius at the hits: vertex normals {np.arccos(cos(want["normal"][hit]).min()):.4f} rad, face normals {np.arccos(cos(want["face_normal"][hit]).min()):.4f} rad')
    assert np.arccos(cos(want['normal'][hit]).min()) < np.arccos(cos(want['face_normal'][hit]).min())
    # face normals: the restatement of the three kernels as they were
    face = M.render_mesh_views(tv, tt, sf['cams'], sf['res'], mode='shaded', normals='face', **kw)
    same_bytes(H(face.rgb).reshape(-1, 3), sf['face']['rgb'], 'rgb (face)')
    same_bytes(H(face.normal).reshape(-1, 3), sf['face']['normal'], 'normal (face)')


def test_interp_normals_leaves_misses_and_bad_triangles_alone(tdgp, sphere_frames):
    sf = sphere_frames
    S = tdgp.mesh_surface
    want = sf['want']['shaded']
    rays = len(want['status'])
    tri = want['tri'].copy()
    hits = np.flatnonzero(want['status'] == 1)
    tri[hits[0]], tri[hits[1]] = len(sf['t']), -3                           # status 1 with a triangle out of range: not touched either
    sentinel = np.full((rays, 3), 7.0, F)
    normal = T(sentinel)
    zero_vn = np.zeros_like(sf['vn'])
    args = (T(tri), T(want['status']), T(want['t_hit']), sf['ray_o'].reshape(rays, 3).contiguous(), sf['ray_d'].reshape(rays, 3).contiguous(), T(sf['v']), T(sf['t']))
    S.interp_normals(*args, T(sf['vn']), normal)
    ref = SR.interp_normals(tri, want['status'], want['t_hit'], H(sf['ray_o']), H(sf['ray_d']), sf['v'], sf['t'], sf['vn'], sentinel)
    same_bytes(H(normal), ref, 'interp over a sentinel')
    untouched = np.ones(rays, bool)
    untouched[hits[2:]] = False
    assert (H(normal)[untouched] == 7.0).all() and (H(normal)[hits[2:]] != 7.0).any(axis=1).all()
    normal = T(sentinel)
    S.interp_normals(*args, T(zero_vn), normal)                             # a vanishing interpolated normal: the normal already there stays
    assert (H(normal) == 7.0).all()


# ------------------------------------------------------------------------------------------------ wiring
B, NV, VOL = 2, 3, 24
SMOOTH = dict(iterations=2, lam=0.5, mu=-0.53)


@pytest.fixture(scope='module')
def scene(tdgp):
    """The scene of test_mesh_components_gpu.py, rebuilt: config_tiny, seeded weights, 2 samples x 3 cameras, volume_res 24 over the whole field;
    a level at which every sample's level set has at least two components with triangles, or `specks` added to sigma to make some."""
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

    def pieces(vol, level):
        v, t = tdgp.geometry.marching_cubes(vol, level)
        return int((tdgp.mesh_components.components(v, t).triangles > 0).sum()) if v.shape[0] else 0

    level, specks = None, None
    for q in (0.5, 0.6, 0.7, 0.8, 0.9, 0.4, 0.3):
        cand = float(grid.flatten().quantile(q))
        if all(pieces(grid[b], cand) >= 2 for b in range(B)):
            level = cand
            break
    if level is None:
        level = float(grid.median())
        specks = torch.zeros(VOL, VOL, VOL, device=DEV)
        lift = float(grid.max() - grid.min()) + 1.0
        below = (grid < level).all(dim=0)
        low = below[1:-1, 1:-1, 1:-1]
        for shift, axis in ((1, 0), (-1, 0), (1, 1), (-1, 1), (1, 2), (-1, 2)):
            low = low & below.roll(shift, axis)[1:-1, 1:-1, 1:-1]
        idx = low.nonzero()[:3] + 1
        assert len(idx) >= 1, 'no room for a speck'
        for d, h, w in idx.tolist():
            specks[d, h, w] = lift
    return dict(G=G, ws=ws, cams=cams, level=level, specks=specks, box=box, res=G.synthesis.test_resolution)


@pytest.fixture
def patched(tdgp, scene, monkeypatch):
    if scene['specks'] is not None:
        g = tdgp.geometry
        grid_fn, planes_fn = g.density_grid, g.density_grid_from_planes
        monkeypatch.setattr(g, 'density_grid', lambda *a, **k: grid_fn(*a, **k) + scene['specks'])
        monkeypatch.setattr(g, 'density_grid_from_planes', lambda *a, **k: planes_fn(*a, **k) + scene['specks'])
    return scene


def test_extract_geometry_with_smoothing(tdgp, patched):
    g, M, S = tdgp.geometry, tdgp.mesh_components, tdgp.mesh_surface
    sc = patched
    kw = dict(volume_res=VOL, cube_size=sc['box'], thresh_value=sc['level'], crop=None)
    smooth = g.extract_geometry(sc['G'], sc['ws'], components=dict(keep=1), smooth=SMOOTH, **kw)
    world = g.extract_geometry(sc['G'], sc['ws'], smooth=SMOOTH, units='world', **kw)
    plain = g.extract_geometry(sc['G'], sc['ws'], **kw)
    none = g.extract_geometry(sc['G'], sc['ws'], smooth=None, **kw)
    assert smooth[0]._fields == ('vertices', 'triangles', 'sigma')
    for b in range(B):
        for f in ('vertices', 'triangles', 'sigma'):
            assert torch.equal(getattr(plain[b], f), getattr(none[b], f)), f
        v, t = g.marching_cubes(plain[b].sigma, sc['level'])
        cv, ct, _, _ = M.clean_mesh(v, t, keep=1)
        sv = S.smooth(cv, ct, **SMOOTH)
        assert not torch.equal(sv, cv)
        diag = (sv.max(dim=0).values - sv.min(dim=0).values).norm()
        assert torch.equal(smooth[b].vertices, sv / diag) and torch.equal(smooth[b].triangles, ct)
        assert torch.equal(world[b].vertices, g.grid_to_world(S.smooth(v, t, **SMOOTH), VOL, (0.0, 0.0, 0.0), sc['box'], None)) and torch.equal(world[b].triangles, t)


def test_render_mesh_frames_with_vertex_normals_and_smoothing(tdgp, patched):
    g, M, S, Me = tdgp.geometry, tdgp.mesh_components, tdgp.mesh_surface, tdgp.mesh
    sc = patched
    G, res = sc['G'], sc['res']
    kw = dict(level=sc['level'], volume_res=VOL)
    frames, counts = Me.render_mesh_frames(G, sc['ws'], sc['cams'], normals='vertex', smooth=SMOOTH, components=dict(keep=1), return_counts=True, **kw)
    coloured = Me.render_mesh_frames(G, sc['ws'], sc['cams'], normals='vertex', smooth=SMOOTH, components=dict(keep=1), mode='colour', **kw)
    flat = Me.render_mesh_frames(G, sc['ws'], sc['cams'], components=dict(keep=1), **kw)
    flat_none = Me.render_mesh_frames(G, sc['ws'], sc['cams'], components=dict(keep=1), smooth=None, normals='face', **kw)
    for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
        assert torch.equal(getattr(flat, k), getattr(flat_none, k)), k
    planes = G.synthesis.tri_planes(sc['ws'], noise_mode='const')
    for b in range(B):
        pb = tdgp.renderer.HWCPlanes(planes.t[b:b + 1])
        sigma = g.density_grid_from_planes(G, pb, VOL, (0.0, 0.0, 0.0), sc['box'])[0]
        v, t = g.marching_cubes(sigma, sc['level'])
        cv, ct, _, _ = M.clean_mesh(v, t, keep=1)
        assert counts[b] == (cv.shape[0], ct.shape[0])
        world = g.grid_to_world(S.smooth(cv, ct, **SMOOTH), VOL, (0.0, 0.0, 0.0), sc['box'], None)
        cams = Me._camera_slice(sc['cams'], DEV, b * NV, (b + 1) * NV)
        want = Me.render_mesh_views(world, ct, cams, res, G=G, normals='vertex', vertex_normals=S.vertex_normals(world, ct))
        want_c = Me.render_mesh_views(world, ct, cams, res, G=G, normals='vertex', mode='colour', vertex_colours=Me.vertex_colours(G, pb, world))
        for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
            assert torch.equal(getattr(frames, k)[b * NV:(b + 1) * NV], getattr(want, k)), (b, k)
            assert torch.equal(getattr(coloured, k)[b * NV:(b + 1) * NV], getattr(want_c, k)), (b, k, 'colour')
    assert int(frames.status.sum()) > 0 and not torch.equal(frames.normal, flat.normal)
    grid = Me.render_mesh_video_grid(G, sc['ws'], sc['cams'], normals='vertex', smooth=SMOOTH, **kw)                 # passed through **kw
    strips = Me.render_mesh_strips(G, sc['ws'], sc['cams'], normals='vertex', **kw)
    assert grid.dtype == torch.uint8 and grid.shape[0] == NV and strips.dtype == torch.uint8 and strips.shape[0] == B


# ------------------------------------------------------------------------------------------------ the tools
def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_ms_gpu_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_take_the_surface_flags(tdgp, tmp_path, capsys):
    """Both command lines on a seeded config_tiny checkpoint: the extraction tool smooths the mesh and writes a .ply with normals that are the
    vertex normals of the vertices it wrote; the trajectory tool draws smoothed meshes with vertex normals and names both in its JSON line."""
    cfg = tdgp.config.config_tiny()
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    ex = _tool('extract_geometry')
    common = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--volume-res', '24', '--cube-size', str(2.0 * cfg.cube_scale), '--thresh-value', '0.0', '--save-ply', '--save-obj',
              '--no-save-mrc']
    ex.main(common + ['--output-dir', str(tmp_path / 'raw')])
    ex.main(common + ['--output-dir', str(tmp_path / 'smooth'), '--smooth-iters', '2', '--smooth-lambda', '0.4', '--smooth-mu', '-0.42', '--smooth-free-boundary', '--vertex-normals'])
    capsys.readouterr()
    checked = 0
    for name in ('0000', '0001'):
        raw, smooth = (open(tmp_path / d / f'{name}.ply', 'rb').read() for d in ('raw', 'smooth'))
        head_raw, head = raw.split(b'end_header\n')[0].decode(), smooth.split(b'end_header\n')[0].decode()
        assert 'property float nx' not in head_raw and 'property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face' in head
        nv = int(head.split('element vertex ')[1].split()[0])
        nf = int(head.split('element face ')[1].split()[0])
        assert f'element vertex {nv}\n' in head_raw and f'element face {nf}\n' in head_raw             # smoothing keeps the topology
        if nv == 0:
            continue
        checked += 1
        rec = np.frombuffer(smooth.split(b'end_header\n', 1)[1], '<f4', nv * 6).reshape(nv, 6)
        faces = np.frombuffer(smooth.split(b'end_header\n', 1)[1], np.dtype([('n', 'u1'), ('i', '<i4', (3,))]), nf, offset=nv * 24)
        raw_v = np.frombuffer(raw.split(b'end_header\n', 1)[1], '<f4', nv * 3).reshape(nv, 3)
        assert not np.array_equal(rec[:, :3], raw_v)
        want_n = tdgp.mesh_surface.vertex_normals(T(np.ascontiguousarray(rec[:, :3])), T(np.ascontiguousarray(faces['i'])))
        same_bytes(np.ascontiguousarray(rec[:, 3:]), H(want_n), 'normals in the .ply')
        obj = open(tmp_path / 'smooth' / f'{name}.obj').read()
        assert obj.count('\nvn ') == nv and '//' in obj and 'vn ' not in open(tmp_path / 'raw' / f'{name}.obj').read()
    assert checked >= 1
    rt = _tool('render_trajectory')
    base = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--trajectory', 'front_circle', '--num-frames', '2', '--level', '0.0', '--volume-res', '24', '--seed', '5', '--vis', 'mesh_grid']
    rt.main(base + ['--out', str(tmp_path / 'face.npy')])
    rt.main(base + ['--out', str(tmp_path / 'vertex.npy'), '--mesh-normals', 'vertex', '--mesh-smooth-iters', '2'])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2 and lines[0]['mesh_normals'] == 'face' and lines[0]['mesh_smooth_iters'] == 0
    assert lines[1]['mesh_normals'] == 'vertex' and lines[1]['mesh_smooth_iters'] == 2 and lines[1]['shape'] == lines[0]['shape'] and lines[1]['triangles'] == lines[0]['triangles']
    a, b = np.load(tmp_path / 'face.npy'), np.load(tmp_path / 'vertex.npy')
    assert a.shape == b.shape == tuple(lines[1]['shape']) and a.dtype == b.dtype == np.uint8      # whether the tiny scene's level set is in view is not this test's business

"""Multisampled mesh frames on the GPU: tdgp_mesh_visibility_ms / tdgp_mesh_resolve_ms bit for bit against the numpy restatement of their
contracts (tests/mesh_msaa_reference.py) on an icosphere and hand-written triangles, for both patterns, every cull mode, face and vertex
normals, vertex colours and a texture under both filters, in every shading mode; the invariance of the frames under runs, triangle
permutations and camera chunks; exact coverage fractions of an axis-aligned quad; `samples=1` as the untouched one-sample route; and the
frame drivers on a seeded config_tiny scene."""
import numpy as np
import pytest
import torch

import mesh_msaa_reference as R
import mesh_raster_reference as MR
import mesh_texture_reference as TR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
D = np.float64
SHADE = dict(ambient=0.25, albedo=(0.9, 0.7, 0.5), background=(1.0, 0.5, -1.0))
OUTPUTS = ('rgb', 'coverage', 'status', 'depth', 'tri', 'normal')
NEAR, T_MISS = 0.1, 2.5


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


def front_camera(tdgp, fov=60.0):
    """One camera at (0, 0, 1) looking down -z."""
    return tdgp.generator.TensorGroup(angles=T(np.array([[0.0, np.pi / 2, 0.0]], F)), fov=T(np.array([fov], F)), radius=T(np.ones(1, F)),
                                      look_at=T(np.zeros((1, 3), F)))


def camera_tensors(tdgp, cams):
    c2w = tdgp.renderer.compute_cam2world_matrix(cams)
    return c2w, tdgp.mesh.focal_lengths(cams.fov, c2w.shape[0], DEV)


def make_texture(tdgp, n_tri, seed):
    """A 4-texel texture of random bytes for a mesh of n_tri triangles -> (the device Texture, the host image, the restatement's Atlas)."""
    Tx = tdgp.mesh_texture
    atlas = Tx.atlas_layout(n_tri, 4)
    image = np.random.RandomState(seed).randint(0, 256, (atlas.height, atlas.width, 3)).astype(np.uint8)
    assert tuple(atlas) == tuple(TR.atlas_layout(n_tri, 4))
    return Tx.Texture(T(image), Tx.atlas_uvs(n_tri, atlas), atlas), image, TR.atlas_layout(n_tri, 4)


def compare(tdgp, v, t, cam, w, h, S, what, cull='none', configs=(dict(),)):
    """vis and, per config (keyword arguments of both resolves), the six outputs: device against restatement -> the restated vis and last frame."""
    M = tdgp.mesh
    c2w, focal = cam
    vt, tt = T(np.asarray(v, F).reshape(-1, 3)), T(np.asarray(t, np.int32).reshape(-1, 3))
    vis = M.mesh_visibility_ms(vt, tt, c2w, focal, (w, h), S, near=NEAR, cull=cull)
    want_vis = R.visibility_ms(v, t, H(c2w), H(focal), h, w, S, NEAR, cull)
    assert vis.shape == (c2w.shape[0], h * w, S) and vis.dtype == torch.int64
    same_bytes(H(vis).view(np.uint64), want_vis, f'vis ({what}, S={S}, cull={cull})')
    want = None
    for cfg in configs:
        host = dict(cfg)
        dev = {k: (T(a) if isinstance(a, np.ndarray) else a) for k, a in cfg.items() if k not in ('image', 'atlas', 'texture')}
        if 'texture' in cfg:
            dev['texture'] = cfg['texture']
            host.pop('texture')
        names = {'vertex_normals': 'vertex_normal', 'texture_filter': 'filter'}
        host = {names.get(k, k): a for k, a in host.items()}
        got = M.mesh_resolve_ms(vis, vt, tt, c2w, focal, (w, h), T_MISS, **dev, **SHADE)
        want = R.resolve_ms(want_vis, v, t, H(c2w), H(focal), h, w, T_MISS, **host, **SHADE)
        tag = ', '.join(f'{k}' if isinstance(a, np.ndarray) or k == 'texture' else f'{k}={a}' for k, a in cfg.items() if k not in ('image', 'atlas'))
        for k, g in zip(OUTPUTS, got):
            same_bytes(H(g), want[k], f'{k} ({what}, S={S}, cull={cull}, {tag or "face normals"})')
    return want_vis, want


@pytest.fixture(scope='module')
def sphere():
    return MR.icosphere(2, 0.3)


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize('S', [4, 16])
def test_icosphere_bit_for_bit(tdgp, sphere, S):
    """320 sub-pixel triangles at 16 x 16 under three cameras with different fields of view (the per-lane path): the keys of every sample and
    every output of the fused resolve equal the restatement, for every source of normals and colour, every mode and every cull."""
    v, t = sphere
    rs = np.random.RandomState(5)
    rgbv = rs.rand(len(v), 3).astype(F)
    vn = (v / np.linalg.norm(v, axis=1, keepdims=True) + 0.2 * rs.randn(len(v), 3)).astype(F)
    vn[7] = 0.0                                                                      # vertex normals that may cancel: the face normal stays there
    tex, image, atlas = make_texture(tdgp, len(t), 11)
    cam = camera_tensors(tdgp, cameras(tdgp))
    textured = [dict(mode='colour', texture=tex, image=image, atlas=atlas, texture_filter=f) for f in ('nearest', 'bilinear')]
    configs = [dict(mode='shaded'), dict(mode='normals'), dict(mode='colour', vertex_rgb=rgbv), dict(mode='shaded', vertex_normals=vn),
               dict(mode='normals', vertex_normals=vn), dict(mode='colour', vertex_normals=vn, vertex_rgb=rgbv), dict(mode='shaded', light=(0.3, 0.5, 0.8)),
               textured[0], textured[1], dict(textured[1], vertex_normals=vn)]
    vis, want = compare(tdgp, v, t, cam, 16, 16, S, 'icosphere 2 at 16', configs=configs)
    cov = want['coverage']
    assert (cov == 1).any() and (cov == 0).any() and ((cov > 0) & (cov < 1)).sum() > 20       # interior, outside and silhouette pixels
    assert len(np.unique(want['tri'])) > 50
    front, _ = compare(tdgp, v, t, cam, 16, 16, S, 'icosphere 2 at 16', cull='back', configs=[dict(mode='colour', vertex_rgb=rgbv)])
    back, _ = compare(tdgp, v, t, cam, 16, 16, S, 'icosphere 2 at 16', cull='front', configs=[dict(mode='shaded', vertex_normals=vn)])
    assert np.array_equal(front, vis) and np.array_equal(back != R.EMPTY, vis != R.EMPTY) and np.all(back[back != R.EMPTY] > vis[back != R.EMPTY])
    compare(tdgp, v, t, tuple(x[1:2] for x in cam), 16, 16, S, 'one camera')


HAND_SMALL = [(-0.1, -0.1, 0), (0.2, -0.1, 0), (-0.1, 0.2, 0)]
HAND_FILL = [(-9, -9, -0.5), (9, -9, -0.5), (0, 9, -0.5)]
HAND_WIDE = [(-0.45, -0.2, 0.1), (0.4, -0.25, -0.2), (0.1, 0.3, 0.2)]
HAND_CORNER = [(-1.2, 0.2, 0), (-0.2, 1.2, 0), (-0.2, 0.2, 0)]
HAND_CASES = {
    'small': (HAND_SMALL, [(0, 1, 2)]),
    'wider than 8 pixels': (HAND_WIDE, [(0, 1, 2)]),
    'frame-filling behind small': (HAND_SMALL + HAND_FILL, [(3, 4, 5), (0, 1, 2)]),
    'across two frame edges': (HAND_CORNER, [(0, 1, 2)]),
    'two equal vertices': ([HAND_SMALL[0], HAND_SMALL[0], HAND_SMALL[1]], [(0, 1, 2)]),
    'three on a line': ([(-0.2, 0, 0), (0, 0, 0), (0.2, 0, 0)], [(0, 1, 2)]),
    'a vertex behind near': ([HAND_SMALL[0], HAND_SMALL[1], (0, 0, 0.95)], [(0, 1, 2)]),
    'indices out of range': (HAND_SMALL, [(0, 1, 3), (0, -1, 2), (0, 1, 2), (2 ** 31 - 1, 0, 1)]),
    'coincident': (HAND_SMALL, [(0, 1, 2), (0, 1, 2), (1, 2, 0)]),
    'non-finite vertex': ([HAND_SMALL[0], HAND_SMALL[1], (np.nan, 0, 0), (np.inf, 0, 0), (1e30, 1e30, 0)], [(0, 1, 2), (0, 1, 3), (0, 1, 4)]),
}


@pytest.mark.parametrize('S', [4, 16])
def test_hand_written_cases_bit_for_bit(tdgp, S):
    """One camera at (0, 0, 1) looking down -z, 24 x 17 (not square, an odd height): triangles whose pixel box exceeds 8 x 8 go through the wave;
    a triangle across the left and the top frame edge is clamped; degenerate triangles and bad indices leave no key."""
    w, h = 24, 17
    cam = camera_tensors(tdgp, front_camera(tdgp))
    hits = {}
    for name, (v, t) in HAND_CASES.items():
        v, t = np.asarray(v, F), np.asarray(t, np.int32)
        rgbv = np.random.RandomState(len(name)).rand(len(v), 3).astype(F)
        for cull in ('none', 'back', 'front'):
            vis, want = compare(tdgp, v, t, cam, w, h, S, name, cull=cull, configs=[dict(mode='colour', vertex_rgb=rgbv), dict(mode='shaded')])
            hits[name, cull] = int((vis != R.EMPTY).sum())
            if cull == 'none':
                cov = want['coverage'].reshape(h, w)
                if name == 'coincident':
                    assert np.all(want['tri'][want['status'] == 1] == 0)             # a tie in t goes to the lower triangle index
                if name == 'wider than 8 pixels':
                    assert (cov > 0).any(axis=0).sum() > 8 and (cov == 1).sum() > 10
                if name == 'across two frame edges':
                    assert cov[0, 0] > 0 and cov[0, :3].min() > 0 and cov[:3, 0].min() > 0 and cov[-1].max() == 0 and cov[:, -1].max() == 0
    n = hits['small', 'none']
    assert 4 * S <= n <= 40 * S and hits['small', 'back'] == n and hits['small', 'front'] == 0
    assert hits['frame-filling behind small', 'none'] == h * w * S and hits['indices out of range', 'none'] == n and hits['coincident', 'none'] == n
    for name in ('two equal vertices', 'three on a line', 'a vertex behind near', 'non-finite vertex'):
        assert hits[name, 'none'] == 0, name
    # T = 0 and V = 0 only clear the buffer
    for v, t, what in ((np.zeros((3, 3), F), np.zeros((0, 3), np.int32), 'T = 0'), (np.zeros((0, 3), F), np.asarray([(0, 1, 2)], np.int32), 'V = 0')):
        vis, want = compare(tdgp, v, t, cam, w, h, S, what)
        assert np.all(vis == R.EMPTY) and want['status'].sum() == 0 and np.all(want['rgb'] == np.asarray(SHADE['background'], F))


# ------------------------------------------------------------------------------------------------ invariance
@pytest.mark.parametrize('S', [4, 16])
def test_runs_permutations_and_chunks_give_the_same_bytes(tdgp, sphere, S):
    M = tdgp.mesh
    v, t = sphere
    w, h = 16, 16
    Rr = w * h
    cams = cameras(tdgp)
    vt, tt = T(v), T(t)
    rgbv = T(np.random.RandomState(2).rand(len(v), 3).astype(F))
    kw = dict(mode='colour', normals='vertex', vertex_colours=rgbv, samples=S, near=NEAR, t_miss=T_MISS, **SHADE)
    base = M.render_mesh_views(vt, tt, cams, (w, h), **kw)
    assert set(base.keys()) == {'rgb', 'depth', 'normal', 'status', 'tri', 'coverage'}
    assert base.rgb.shape == (3, Rr, 3) and base.depth.shape == (3, Rr, 1) and base.normal.shape == (3, Rr, 3) and base.status.shape == (3, Rr)
    assert base.tri.shape == (3, Rr) and base.coverage.shape == (3, Rr) and base.coverage.dtype == torch.float32 and base.status.dtype == torch.int32
    # the views are the two kernels: restated once, with the vertex normals the call computed for itself
    c2w, focal = camera_tensors(tdgp, cams)
    vn = H(tdgp.mesh_surface.vertex_normals(vt, tt))
    want = R.frames_ms(v, t, H(c2w), H(focal), h, w, S, NEAR, 'none', T_MISS, vertex_normal=vn, vertex_rgb=H(rgbv), mode='colour', **SHADE)
    for k in OUTPUTS:
        same_bytes(H(base[k]).reshape(want[k].shape), want[k], f'render_mesh_views {k} (S={S})')
    again = M.render_mesh_views(vt, tt, cams, (w, h), **kw)
    for k in base:
        assert torch.equal(base[k], again[k]), k
    perm = np.random.RandomState(3).permutation(len(t))
    shuffled = M.render_mesh_views(vt, T(t[perm]), cams, (w, h), **kw)
    for k in ('rgb', 'depth', 'normal', 'status', 'coverage'):
        assert torch.equal(shuffled[k], base[k]), k
    hit = H(base.status) == 1
    assert np.array_equal(perm[H(shuffled.tri)[hit]], H(base.tri)[hit]) and np.all(H(shuffled.tri)[~hit] == -1)
    for chunk in (Rr, 1, 2 * Rr * S + 5):                                            # one frame per call (twice) and two
        out = M.render_mesh_views(vt, tt, cams, (w, h), max_rays_per_call=chunk, **kw)
        for k in base:
            assert torch.equal(base[k], out[k]), (k, chunk)


# ------------------------------------------------------------------------------------------------ exact coverage
def test_exact_coverage_of_an_axis_aligned_quad(tdgp):
    """A quad in the plane z = 0 whose edges project to pixel coordinates c + k/4, k = 0..3, under the front camera at 16 x 16: coverage is
    exactly the share of each pixel's samples inside [x0, x1) x [y0, y1); a fully covered pixel of a flat unlit mesh has the one-sample colour."""
    M = tdgp.mesh
    w = h = 16
    cams = front_camera(tdgp)
    c2w, focal = camera_tensors(tdgp, cams)
    x0, x1, y0, y1 = 3 * 256 + 64, 11 * 256 + 192, 2 * 256 + 0, 9 * 256 + 128          # k = 1, 3, 0, 2
    m, fc = H(c2w)[0].astype(D), D(H(focal)[0])
    corners = []
    for X, Y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)):
        u, vv = (X / (256.0 * (w - 1) * 0.5) - 1.0) / fc, (1.0 - Y / (256.0 * (h - 1) * 0.5)) / fc
        corners.append(m[:3, 3] + u * m[:3, 0] + vv * m[:3, 1] - m[:3, 2])             # camera depth 1: the plane z = 0
    v, t = np.asarray(corners, F), np.asarray([(0, 2, 1), (0, 3, 2)], np.int32)
    assert np.abs(v[:, 2]).max() < 1e-6
    colour = np.tile(np.asarray([[0.3, 0.6, 0.9]], F), (4, 1))
    kw = dict(mode='colour', vertex_colours=T(colour), ambient=1.0, background=(1.0, 0.5, -1.0), near=NEAR, t_miss=T_MISS)
    one = M.render_mesh_views(T(v), T(t), cams, (w, h), **kw)
    assert 'coverage' not in one
    for S in (4, 16):
        out = M.render_mesh_views(T(v), T(t), cams, (w, h), samples=S, **kw)
        ox, oy = R.offsets(S)
        sx = (np.arange(w) << 8)[None, :, None] + ox[None, None, :]
        sy = (np.arange(h) << 8)[:, None, None] + oy[None, None, :]
        n = ((sx >= x0) & (sx < x1) & (sy >= y0) & (sy < y1)).sum(axis=2)
        cov = H(out.coverage).reshape(h, w)
        same_bytes(cov, (n.astype(F) / F(S)).astype(F), f'coverage (S={S})')
        assert set(np.unique(n)) >= {0, S} and len(np.unique(n)) > 3                   # outside, interior and several partial fractions
        if S == 16:
            assert n[2, 3] == 2 * 1 and n[2, 5] == 2 * 4 and n[5, 3] == 4 * 1 and n[9, 12] == 4 * 1 and n[5, 5] == 16 and n[10, 5] == 0
        assert np.all(cov[4:9, 5:11] == 1) and np.all(cov[:2] == 0) and np.all(cov[:, :3] == 0) and np.all(cov[10:] == 0) and np.all(cov[:, 13:] == 0)
        rgb = H(out.rgb).reshape(h, w, 3)
        assert np.all(rgb[n == 0] == np.asarray(kw['background'], F)) and np.all(H(out.status).reshape(h, w) == (n > 0))
        full = n == S
        assert full.sum() >= 30 and np.all(H(one.status).reshape(h, w)[full] == 1)
        same_bytes(rgb[full], H(one.rgb).reshape(h, w, 3)[full], f'rgb of the fully covered pixels (S={S})')
        # a partly covered pixel lies between the surface colour and the background
        part = (n > 0) & (n < S)
        lo, hi = np.minimum(rgb[full][0], kw['background']), np.maximum(rgb[full][0], kw['background'])
        assert part.any() and np.all(rgb[part] >= lo - 1e-6) and np.all(rgb[part] <= hi + 1e-6)


# ------------------------------------------------------------------------------------------------ samples = 1, drivers
def test_one_sample_is_the_untouched_route(tdgp, sphere):
    M = tdgp.mesh
    v, t = sphere
    cams = cameras(tdgp)
    rgbv = T(np.random.RandomState(2).rand(len(v), 3).astype(F))
    for kw in (dict(), dict(mode='colour', normals='vertex', vertex_colours=rgbv), dict(mode='normals', cull='back', max_rays_per_call=300)):
        plain = M.render_mesh_views(T(v), T(t), cams, 16, **kw, **SHADE)
        one = M.render_mesh_views(T(v), T(t), cams, 16, samples=1, **kw, **SHADE)
        assert list(one.keys()) == list(plain.keys()) == ['rgb', 'depth', 'normal', 'status', 'tri']
        for k in plain:
            assert one[k].dtype == plain[k].dtype and torch.equal(one[k], plain[k]), k


B, V, VOL = 2, 3, 24


@pytest.fixture(scope='module')
def scene(tdgp):
    """config_tiny, seeded weights, 2 samples x 3 cameras, volume_res 24 over the whole field; the level is the median of the density grids
    (the scene of tests/test_mesh_frames_gpu.py)."""
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
    return dict(G=G, ws=ws, cams=cams, level=float(grid.median()), grid=grid, box=box, res=G.synthesis.test_resolution)


def test_frames_grids_and_strips_take_samples(tdgp, scene):
    M, I, g = tdgp.mesh, tdgp.inference, tdgp.geometry
    sc = scene
    G, res = sc['G'], sc['res']
    kw = dict(level=sc['level'], volume_res=VOL, **SHADE)
    frames = M.render_mesh_frames(G, sc['ws'], sc['cams'], samples=4, **kw)
    assert set(frames.keys()) == {'rgb', 'depth', 'normal', 'status', 'tri', 'coverage'} and frames.coverage.shape == (B * V, res * res)
    cov = frames.coverage
    assert bool(((cov > 0) & (cov < 1)).any()) and bool((cov == 0).any()) and torch.equal(frames.status == 1, cov > 0)
    for b in range(B):
        verts, tris = g.marching_cubes(sc['grid'][b], sc['level'])
        world = g.grid_to_world(verts, VOL, (0.0, 0.0, 0.0), sc['box'], crop=None)
        views = M.render_mesh_views(world, tris, sc['cams'][b * V:(b + 1) * V], res, G=G, samples=4, **SHADE)
        for k in views:
            assert torch.equal(frames[k][b * V:(b + 1) * V], views[k]), (k, b)
    plain = M.render_mesh_frames(G, sc['ws'], sc['cams'], **kw)
    assert 'coverage' not in plain and not torch.equal(plain.rgb, frames.rgb)
    grid = M.render_mesh_video_grid(G, sc['ws'], sc['cams'], samples=4, **kw)
    assert grid.dtype == torch.uint8 and torch.equal(grid, I.frames_to_grid(frames.rgb, res, res, tiles=B, images=V, stride_image=1, stride_tile=V, nrow=2))
    assert not torch.equal(grid, M.render_mesh_video_grid(G, sc['ws'], sc['cams'], **kw))
    strips = M.render_mesh_strips(G, sc['ws'], sc['cams'], samples=16, normals='vertex', as_numpy=True, **kw)
    assert isinstance(strips, np.ndarray) and strips.dtype == np.uint8 and strips.shape == (B, res, V * res, 3)
    with pytest.raises(ValueError, match='samples'):
        M.render_mesh_frames(G, sc['ws'], sc['cams'], samples=4, normals='field', **kw)

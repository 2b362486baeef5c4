"""Mesh textures on the GPU: tdgp_atlas_points / tdgp_atlas_texels / tdgp_mesh_sample_texture bit for bit against the numpy restatement of their
contracts (tests/mesh_texture_reference.py) on a single triangle, closed, degenerate and marching-cubes meshes at the block edges of the
kernels; run-to-run and chunking identity; the linear-colour property end to end; what the feature is for (a checker finer than the
triangles); and the `texture=` options of mesh.render_mesh_views / render_mesh_frames, geometry.extract_geometry and the two command lines
on a seeded config_tiny scene."""
import functools
import importlib
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import mesh_components_reference as CR
import mesh_raster_reference as MR
import mesh_surface_reference as SR
import mesh_texture_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
D = np.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADE = dict(ambient=0.25, background=(1.0, 0.5, -1.0))


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


# ------------------------------------------------------------------------------------------------ the meshes (all inside the unit ball)
def _random_vertices(V, seed):
    return (np.random.RandomState(seed).randn(V, 3) * 0.15).astype(F)


def _mc_mesh():
    tdgp = importlib.import_module('3dgp_amd')
    v, t = tdgp.geometry.marching_cubes(T(CR.speck_volume(24)), 0.0)
    return ((H(v).astype(D) - 11.5) / 11.5 * 0.3).astype(F), H(t)


def _soup():
    """test_mesh_surface_gpu's soup: random triples over 40 of 42 vertices, then indices out of range, needles, points and duplicates."""
    t = CR.soup(40, 60, 7)
    extra = np.array([[0, 1, 42], [3, -1, 5], [2 ** 31 - 1, 0, 1], [7, 7, 9], [11, 11, 11], [4, 9, 4], t[5], t[5], [0, 1, 2], [2, 1, 0]], np.int32)
    return _random_vertices(42, 21), np.concatenate([t[:30], extra, t[30:]]).astype(np.int32)


MESHES = {
    'single triangle': lambda: (np.array([[-0.2, -0.15, 0.05], [0.25, -0.1, -0.05], [-0.05, 0.22, 0.1]], F), np.array([[0, 1, 2]], np.int32)),
    'tetrahedron': lambda: (SR.TETRA_V * F(0.15), SR.TETRA_T),
    'icosphere': lambda: MR.icosphere(1, 0.3),
    'soup': _soup,
    'marching cubes': _mc_mesh,
}
# texels = 2: 16 texels per tile.  P = 16 tiles: H * W = 256, exactly one block of lanes; P = 17: 20 x 16 = 320, one block and a partial one
for _T in (31, 32, 33, 34):
    MESHES[f'soup T={_T}'] = lambda n=_T: (_random_vertices(24, n), CR.soup(24, n, n))
TEXELS = {name: (2, 3, 8, 64) for name in ('single triangle', 'tetrahedron', 'icosphere')}
TEXELS.update({'soup': (2, 3, 8), 'marching cubes': (2, 3, 8), 'soup T=31': (2,), 'soup T=32': (2, 3), 'soup T=33': (2,), 'soup T=34': (2, 8)})


@functools.lru_cache(maxsize=None)
def named_mesh(name):
    v, t = MESHES[name]()
    v, t = np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def wavy(p):
    """A colour_fn on the device that leaves [-1, 1] and has a fourth column, as the field's rows do."""
    return torch.cat([torch.sin(p * 23.0) * 1.2, p[:, :1]], dim=1)


# ------------------------------------------------------------------------------------------------ the two bake kernels
@pytest.mark.parametrize('name', sorted(MESHES))
def test_atlas_points_and_texels_bit_for_bit(tdgp, name):
    Tx = tdgp.mesh_texture
    v, t = named_mesh(name)
    tv, tt = T(v), T(t)
    for n in TEXELS[name]:
        atlas = Tx.atlas_layout(len(t), n)
        assert tuple(atlas) == tuple(R.atlas_layout(len(t), n))
        points, owner = Tx.atlas_points(tv, tt, atlas)
        want_p, want_o = R.atlas_points(v, t, R.Atlas(*atlas))
        same_bytes(H(owner), want_o, f'owner ({name}, {n})')
        same_bytes(H(points), want_p, f'points ({name}, {n})')
        rgb = wavy(points)                                                   # [N,4]: read in place, stride 4
        fill = (7, 130, 255)
        tex = Tx.bake(tv, tt, wavy, texels=n, fill=fill)
        want_i = R.atlas_texels(H(rgb), want_o, fill).reshape(atlas.height, atlas.width, 3)
        same_bytes(H(tex.image), want_i, f'image ({name}, {n})')
        assert tex.atlas == atlas and tex.uvs.tobytes() == R.atlas_uvs(len(t), atlas).tobytes()
        assert (want_o >= 0).any() and ((want_o < 0).any() or len(t) % 2 == 0)
        # contiguous [N,3] rows and a run of texels in the middle of the atlas go the same way
        N = len(want_o)
        part = torch.zeros(N, 3, dtype=torch.uint8, device=DEV)
        Tx.atlas_texels(rgb[:, :3].contiguous(), owner, part, fill)
        assert torch.equal(part.view_as(tex.image), tex.image)
        i0, i1 = N // 3, N - N // 5
        part.zero_()
        Tx.atlas_texels(rgb[i0:i1], owner[i0:i1], part[i0:i1], fill)
        assert torch.equal(part[i0:i1], tex.image.view(N, 3)[i0:i1]) and int(part[:i0].sum()) == 0 and int(part[i1:].sum()) == 0
    if name == 'soup T=32':
        assert Tx.atlas_layout(32, 2).width * Tx.atlas_layout(32, 2).height == 256
    if name == 'soup T=33':
        assert Tx.atlas_layout(33, 2).width * Tx.atlas_layout(33, 2).height == 320


def test_empty_mesh_bakes_an_empty_image(tdgp):
    Tx = tdgp.mesh_texture
    calls = []
    tex = Tx.bake(T(np.zeros((3, 3), F)), torch.zeros(0, 3, dtype=torch.int32, device=DEV), lambda p: calls.append(p) or p)
    assert tuple(tex.image.shape) == (0, 0, 3) and tex.image.dtype == torch.uint8 and tex.uvs.shape == (0, 3, 2) and not calls
    with pytest.raises(ValueError, match='16384'):
        Tx.bake(T(np.zeros((3, 3), F)), torch.zeros(2 * 248 * 248 + 1, 3, dtype=torch.int32, device=DEV), wavy, texels=64)
    with pytest.raises(ValueError, match='colour_fn'):
        Tx.bake(T(named_mesh('tetrahedron')[0]), T(named_mesh('tetrahedron')[1]), lambda p: p[:, :2])


# ------------------------------------------------------------------------------------------------ the fetch
def cameras(tdgp, n=2):
    angles = np.array([[0.3, 1.3, 0.0], [-0.5, 1.8, 0.0]], F)[:n]
    return tdgp.generator.TensorGroup(angles=T(angles), fov=T(np.array([40.0, 50.0], F)[:n]), radius=T(np.array([1.0, 1.1], F)[:n]), look_at=T(np.zeros((n, 3), F)))


def resolved(tdgp, tv, tt, res, cams=None):
    """The device's own visibility + resolve of a mesh under the two cameras (tested bit for bit elsewhere) -> the inputs of the fetch."""
    M = tdgp.mesh
    cams = cameras(tdgp) if cams is None else cams
    c2w = tdgp.renderer.compute_cam2world_matrix(cams)
    C = int(c2w.shape[0])
    focal = M.focal_lengths(cams.fov, C, DEV)
    ray_o, ray_d = tdgp.renderer.sample_rays(c2w, fov=cams.fov, resolution=(res, res))
    o, d = ray_o.reshape(-1, 3).contiguous(), ray_d.reshape(-1, 3).contiguous()
    vis = M.mesh_visibility(tv, tt, c2w, focal, d, (res, res), near=0.1)
    t_hit, status, tri, normal, _, _ = M.mesh_resolve(vis.reshape(-1), tv, tt, o, d, 1.0 / 64, 2.5)
    return dict(tri=tri, status=status, t_hit=t_hit, o=o, d=d, normal=normal, c2w=c2w, focal=focal)


@pytest.mark.parametrize('name', ['single triangle', 'tetrahedron', 'icosphere', 'soup', 'marching cubes'])
def test_sample_texture_bit_for_bit_on_frames(tdgp, name):
    Tx = tdgp.mesh_texture
    v, t = named_mesh(name)
    tv, tt = T(v), T(t)
    hits = 0
    for n in (2, 5) if name != 'icosphere' else (2, 3, 8, 64):
        tex = Tx.bake(tv, tt, wavy, texels=n, fill=(255, 0, 255))
        image, atlas = H(tex.image), R.Atlas(*tex.atlas)
        for res in (32, 64):
            r = resolved(tdgp, tv, tt, res)
            host = [H(r[k]) for k in ('tri', 'status', 't_hit', 'o', 'd')]
            for filt in ('nearest', 'bilinear'):
                got = Tx.sample_texture(r['tri'], r['status'], r['t_hit'], r['o'], r['d'], tv, tt, tex, filt)
                same_bytes(H(got), R.sample_texture(*host, v, t, image, atlas, filt), f'colour ({name}, texels {n}, {res}^2, {filt})')
                again = Tx.sample_texture(r['tri'], r['status'], r['t_hit'], r['o'], r['d'], tv, tt, tex, filt)
                assert torch.equal(again, got)
            hits += int(host[1].sum())
            assert (H(got)[host[1] == 0] == 0).all() and H(got).min() >= 0.0 and H(got).max() <= 1.0
    assert hits > 50


def test_sample_texture_at_hand_placed_hits(tdgp):
    """Corners, edge midpoints, the hypotenuse and the centroid of lower and upper triangles, misses and invalid triangles in one launch."""
    Tx = tdgp.mesh_texture
    v, t = named_mesh('soup')
    tv, tt = T(v), T(t)
    bary = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5], [0, 0.25, 0.75], [0, 0.9, 0.1], [1 / 3, 1 / 3, 1 / 3],
                     [0.2, 0.3, 0.5], [-0.2, 0.6, 0.6], [0.5, 0.7, -0.2]], D)                   # the last two lie outside: clamped onto the triangle
    good = [k for k in range(len(t)) if (t[k] >= 0).all() and (t[k] < len(v)).all() and len(set(t[k].tolist())) == 3]
    ks = np.array(good[:6] + good[-6:] + [30, 31, 32, 33, 34, 35], np.int64)                       # lower and upper ones, and the bad, needle and point rows of the soup
    assert (ks % 2 == 0).any() and (ks % 2 == 1).any()
    k = np.repeat(ks, len(bary))
    b = np.tile(bary, (len(ks), 1))
    idx = np.clip(t[k], 0, len(v) - 1)
    P = v[idx].astype(D)
    x = ((b[:, :1] * P[:, 0] + b[:, 1:2] * P[:, 1]) + b[:, 2:] * P[:, 2]).astype(F)
    tri = np.concatenate([k, [len(t), -1, 2 ** 31 - 1, 0, 1]]).astype(np.int32)                    # out of range three ways, then two misses
    status = np.concatenate([np.ones(len(k) + 3), [0, 0]]).astype(np.int32)
    x = np.concatenate([x, np.tile(x[:1], (5, 1))])
    rays = len(tri)
    # the hit is o + d * t_hit: o = x / 2, d = x, t_hit = 1 / 2
    o, d, th = (x * F(0.5)).astype(F), x, np.full(rays, 0.5, F)
    for n in (2, 3, 8, 64):
        tex = Tx.bake(tv, tt, wavy, texels=n, fill=(255, 0, 255))
        for filt in ('nearest', 'bilinear'):
            got = H(Tx.sample_texture(T(tri), T(status), T(th), T(o), T(d), tv, tt, tex, filt))
            want = R.sample_texture(tri, status, th, o, d, v, t, H(tex.image), R.Atlas(*tex.atlas), filt)
            same_bytes(got, want, f'hand-placed hits (texels {n}, {filt})')
            assert (got[-5:] == 0).all() and (got[tri == 30] == 0).all() and np.isfinite(got).all()
            if filt == 'nearest':
                # at a corner (rows 0, 1, 2 of every proper triangle's block) the fetch is that corner's texel: the byte the bake stored
                image, uv = H(tex.image), tex.uvs.astype(D)
                for j, kk in enumerate(ks[:12]):
                    for c in range(3):
                        px, py = int(round(uv[kk, c, 0] * tex.atlas.width - 0.5)), int(round((1 - uv[kk, c, 1]) * tex.atlas.height - 0.5))
                        assert (got[j * len(bary) + c] == (image[py, px].astype(D) / 255).astype(F)).all(), (n, kk, c)


def test_bake_and_frames_are_the_same_bytes_on_every_run_and_under_chunking(tdgp):
    Tx, M = tdgp.mesh_texture, tdgp.mesh
    v, t = named_mesh('marching cubes')
    tv, tt = T(v), T(t)
    calls = []

    def counted(p):
        calls.append(int(p.shape[0]))
        return wavy(p)

    a = Tx.bake(tv, tt, counted, texels=8)
    whole = list(calls)
    calls.clear()
    b = Tx.bake(tv, tt, counted, texels=8, points_per_call=1000)
    N = a.atlas.width * a.atlas.height
    assert whole == [N] and calls == [1000] * (N // 1000) + ([N % 1000] if N % 1000 else []) and len(calls) > 3
    assert torch.equal(a.image, b.image) and torch.equal(Tx.bake(tv, tt, wavy, texels=8).image, a.image)
    cams = cameras(tdgp)
    kw = dict(mode='colour', texture=a, near=0.1, t_miss=2.5, **SHADE)
    for normals in ('face', 'vertex'):
        for filt in ('nearest', 'bilinear'):
            one = M.render_mesh_views(tv, tt, cams, 32, normals=normals, texture_filter=filt, **kw)
            two = M.render_mesh_views(tv, tt, cams, 32, normals=normals, texture_filter=filt, max_rays_per_call=32 * 32, **kw)
            three = M.render_mesh_views(tv, tt, cams, 32, normals=normals, texture_filter=filt, **kw)
            for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
                assert torch.equal(getattr(one, k), getattr(two, k)) and torch.equal(getattr(one, k), getattr(three, k)), (normals, filt, k)
    assert int(one.status.sum()) > 50


def test_textured_frames_are_resolve_sample_shade(tdgp):
    """render_mesh_views(mode='colour', texture=...) against the restatement's whole chain, face and vertex normals, and its refusals."""
    Tx, M = tdgp.mesh_texture, tdgp.mesh
    v, t = named_mesh('icosphere')
    tv, tt = T(v), T(t)
    cams = cameras(tdgp)
    res = 32
    tex = Tx.bake(tv, tt, wavy, texels=5)
    r = resolved(tdgp, tv, tt, res)
    start, corner, _ = SR.corner_table(t, len(v))
    vn = SR.vertex_normals(v, t, start, corner, 0)
    for normals, filt in (('face', 'bilinear'), ('vertex', 'nearest')):
        want = R.frames(v, t, H(r['c2w']), H(r['focal']), H(r['o']), H(r['d']), res, res, 0.1, 'none', 1.0 / 64, 2.5, H(tex.image), R.Atlas(*tex.atlas), filt,
                        vertex_normal=vn if normals == 'vertex' else None, **SHADE)
        got = M.render_mesh_views(tv, tt, cams, res, mode='colour', normals=normals, texture=tex, texture_filter=filt, near=0.1, t_miss=2.5, step=1.0 / 64, **SHADE)
        for k, wk in (('rgb', 'rgb'), ('normal', 'normal'), ('depth', 't_hit'), ('status', 'status'), ('tri', 'tri')):
            same_bytes(H(getattr(got, k)).reshape(want[wk].shape), want[wk], f'{k} ({normals}, {filt})')
        assert 0.05 < want['status'].mean() < 0.9
    other = Tx.bake(tv, tt[:-2].contiguous(), wavy, texels=5)
    with pytest.raises(ValueError, match='another mesh'):
        M.render_mesh_views(tv, tt, cams, res, mode='colour', texture=other)
    for kw in (dict(mode='shaded'), dict(mode='normals'), dict(mode='colour', texture_filter='trilinear')):
        with pytest.raises(ValueError):
            M.render_mesh_views(tv, tt, cams, res, texture=tex, **kw)
    # without a texture the colour mode is the vertex-colour path it was
    rgbv = T(np.random.RandomState(3).rand(len(v), 3).astype(F))
    a = M.render_mesh_views(tv, tt, cams, res, mode='colour', vertex_colours=rgbv, near=0.1)
    b = M.render_mesh_views(tv, tt, cams, res, mode='colour', vertex_colours=rgbv, near=0.1, texture=None, texture_filter='bilinear')
    assert torch.equal(a.rgb, b.rgb)


# ------------------------------------------------------------------------------------------------ properties
def test_linear_colour_comes_back_within_the_quantisation_on_the_device(tdgp):
    """The property the unclamped gutter exists for, end to end on the device.  colour(x) = A x + c, never clamped.  Every hit of the frame:
    |fetched - colour(true hit)| <= 0.5 / 255 + sum_c |A_jc| / 2 * |x32_c - x_c|, where x = o + d * t_hit in float64 from the fp32 o, d, t_hit
    and x32 the same in fp32 as the kernel forms it -- the quantisation of a texel (a bilinear fetch is a convex combination of four texels
    of one linear function, so it inherits the bound) plus the fp32 error of the hit point times the gradient, computed here per ray."""
    Tx = tdgp.mesh_texture
    v, t = named_mesh('icosphere')
    tv, tt = T(v), T(t)
    rs = np.random.RandomState(5)
    A, c0 = rs.uniform(-0.5, 0.5, (3, 3)), rs.uniform(-0.2, 0.2, 3)
    tA, tc = T(A.astype(F)), T(c0.astype(F))
    A32, c32 = A.astype(F).astype(D), c0.astype(F).astype(D)
    fn = lambda p: (p.double() @ tA.double().T + tc.double()).float()      # noqa: E731
    worst = 0.0
    for n in (2, 8):
        tex = Tx.bake(tv, tt, fn, texels=n)
        for res in (32, 64):
            r = resolved(tdgp, tv, tt, res)
            got = H(Tx.sample_texture(r['tri'], r['status'], r['t_hit'], r['o'], r['d'], tv, tt, tex, 'bilinear')).astype(D)
            o, d, th, hit = H(r['o']), H(r['d']), H(r['t_hit']), H(r['status']) == 1
            x = o.astype(D) + d.astype(D) * th.astype(D)[:, None]
            x32 = (o + d * th[:, None]).astype(D)
            want = (x @ A32.T + c32) * 0.5 + 0.5
            assert want[hit].min() > 0.02 and want[hit].max() < 0.98
            bound = 0.5 / 255 + (np.abs(x32 - x) @ np.abs(A32).T) * 0.5
            err = np.abs(got - want)
            print(f'texels {n} at {res}^2: {hit.sum()} hits, worst error {err[hit].max() * 255:.4f} / 255, worst error / bound {(err[hit] / bound[hit]).max():.4f}, '
                  f'fp32 term at most {(bound[hit].max() - 0.5 / 255) * 255:.2e} / 255')
            worst = max(worst, float((err[hit] / bound[hit]).max()))
            assert hit.sum() > 50 and (err[hit] <= bound[hit]).all()
    assert worst > 0.3                                                      # the quantisation is there: the bound is not vacuous


def test_a_texture_carries_what_vertex_colours_cannot(tdgp):
    """What the feature is for: icosphere(1), 80 triangles of edge ~0.16, under a checker of period 0.05.  Against colour_fn at every pixel's
    own hit point, the unlit textured frame at 16 texels has a strictly smaller mean absolute error than the vertex-colour frame, and the error
    does not grow from 4 to 16 texels.  No ratio is fixed."""
    Tx, M = tdgp.mesh_texture, tdgp.mesh
    v, t = named_mesh('icosphere')
    tv, tt = T(v), T(t)
    period = 0.05
    edge = np.linalg.norm(v[t[:, 0]] - v[t[:, 1]], axis=1).min()
    assert period < edge / 3

    def checker(p):
        s = torch.floor(p.double() / period).sum(dim=1) % 2
        return ((s * 2 - 1) * 0.8).float()[:, None].expand(-1, 3) * torch.tensor([1.0, -1.0, 0.5], device=p.device)

    cams = cameras(tdgp)
    res = 64
    kw = dict(mode='colour', ambient=1.0, near=0.1, t_miss=2.5)             # ambient 1: the unlit colour, rgb = k * 2 - 1
    vc = (checker(tv) * 0.5 + 0.5).clamp(0, 1)
    plain = M.render_mesh_views(tv, tt, cams, res, vertex_colours=vc, **kw)
    hit = plain.status.reshape(-1) == 1
    r = resolved(tdgp, tv, tt, res)
    o, d = r['o'], r['d']
    x = o + d * plain.depth.reshape(-1, 1)
    want = checker(x)[hit].double()
    mae = lambda frames: float((frames.rgb.reshape(-1, 3)[hit].double() - want).abs().mean())      # noqa: E731
    e_vertex = mae(plain)
    e = {n: mae(M.render_mesh_views(tv, tt, cams, res, texture=Tx.bake(tv, tt, checker, texels=n), **kw)) for n in (4, 16)}
    print(f'mean absolute error over {int(hit.sum())} hits: vertex colours {e_vertex:.4f}, texture at 4 texels {e[4]:.4f}, at 16 texels {e[16]:.4f}')
    assert int(hit.sum()) > 500 and e[16] < e_vertex and e[16] <= e[4]


# ------------------------------------------------------------------------------------------------ wiring
B, NV, VOL = 2, 3, 24
TEX = dict(texels=4, filter='nearest')


@pytest.fixture(scope='module')
def scene(tdgp):
    """config_tiny, seeded weights, 2 samples x 3 cameras, volume_res 24 over the whole field, the level at the median of the grid."""
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


def test_render_mesh_frames_with_a_texture(tdgp, scene):
    g, Me, Tx, S = tdgp.geometry, tdgp.mesh, tdgp.mesh_texture, tdgp.mesh_simplify
    sc = scene
    G, res = sc['G'], sc['res']
    kw = dict(level=sc['level'], volume_res=VOL, simplify=dict(cell=2.0))
    frames, counts = Me.render_mesh_frames(G, sc['ws'], sc['cams'], mode='colour', normals='vertex', texture=TEX, return_counts=True, **kw)
    planes = G.synthesis.tri_planes(sc['ws'], noise_mode='const')
    for b in range(B):
        pb = tdgp.renderer.HWCPlanes(planes.t[b:b + 1])
        sigma = g.density_grid_from_planes(G, pb, VOL, (0.0, 0.0, 0.0), sc['box'])[0]
        v, t = g.marching_cubes(sigma, sc['level'])
        sv, st = S.apply(v, t, dict(cell=2.0))[:2]
        world = g.grid_to_world(sv, VOL, (0.0, 0.0, 0.0), sc['box'], None)
        tex = Tx.bake_field(G, pb, world, st, texels=4)
        assert counts[b] == (sv.shape[0], st.shape[0]) and counts[b].atlas == tex.atlas == Tx.atlas_layout(st.shape[0], 4) and st.shape[0] > 0
        # the bake is the field's colour at the texels' points, quantised
        points, owner = Tx.atlas_points(world, st, tex.atlas)
        rgb = tdgp.shapes.field_functions(G.synthesis)[1](pb, points.unsqueeze(0))[0]
        same_bytes(H(tex.image).reshape(-1, 3), R.atlas_texels(H(rgb), H(owner)), f'bake_field (sample {b})')
        cams = Me._camera_slice(sc['cams'], DEV, b * NV, (b + 1) * NV)
        want = Me.render_mesh_views(world, st, cams, res, G=G, mode='colour', normals='vertex', texture=tex, texture_filter='nearest')
        for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
            assert torch.equal(getattr(frames, k)[b * NV:(b + 1) * NV], getattr(want, k)), (b, k)
    # the option off: byte-identical to a call that never mentions it, counts without an atlas
    for mode, normals in (('colour', 'vertex'), ('shaded', 'face')):
        off, off_counts = Me.render_mesh_frames(G, sc['ws'], sc['cams'], mode=mode, normals=normals, texture=None, return_counts=True, **kw)
        never = Me.render_mesh_frames(G, sc['ws'], sc['cams'], mode=mode, normals=normals, **kw)
        for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
            assert torch.equal(getattr(off, k), getattr(never, k)), (mode, k)
        assert all(c.atlas is None for c in off_counts)
    assert int(frames.status.sum()) > 0 and torch.equal(frames.status, off.status)
    for bad in (dict(mode='shaded'), dict(mode='colour', normals='field')):
        with pytest.raises(ValueError):
            Me.render_mesh_frames(G, sc['ws'], sc['cams'], texture=TEX, **bad, **kw)
    grid, gc = Me.render_mesh_video_grid(G, sc['ws'], sc['cams'], mode='colour', texture=TEX, return_counts=True, **kw)
    strips = Me.render_mesh_strips(G, sc['ws'], sc['cams'], mode='colour', texture=dict(texels=4), **kw)
    assert grid.dtype == torch.uint8 and grid.shape[0] == NV and strips.dtype == torch.uint8 and strips.shape[0] == B and [c.atlas for c in gc] == [c.atlas for c in counts]


def test_extract_geometry_with_a_texture(tdgp, scene):
    g, Tx = tdgp.geometry, tdgp.mesh_texture
    sc = scene
    G = sc['G']
    kw = dict(volume_res=VOL, cube_size=sc['box'], thresh_value=sc['level'], crop=None, simplify=dict(cell=2.0))
    plain = g.extract_geometry(G, sc['ws'], **kw)
    off = g.extract_geometry(G, sc['ws'], texture=None, **kw)
    world = g.extract_geometry(G, sc['ws'], units='world', **kw)
    tex_index, counts = g.extract_geometry(G, sc['ws'], texture=dict(texels=4), return_counts=True, **kw)
    tex_world = g.extract_geometry(G, sc['ws'], texture=dict(texels=4), units='world', **kw)
    syn = G.synthesis
    for b in range(B):
        # the planes as `density_grid` computes them for one sample
        pb = tdgp.renderer.planes_to_hwc(syn.tri_plane_decoder(sc['ws'][b:b + 1, :syn.tri_plane_decoder.num_ws], hwc=True, noise_mode='const'))
        assert type(plain[b]) is g.Shape and type(off[b]) is g.Shape and type(tex_index[b]) is g.TexturedShape
        for f in ('vertices', 'triangles', 'sigma'):
            assert torch.equal(getattr(plain[b], f), getattr(off[b], f)), f                         # the option off: the same bytes
            assert torch.equal(getattr(plain[b], f), getattr(tex_index[b], f)), f                   # and the mesh itself does not depend on it
            assert torch.equal(getattr(world[b], f), getattr(tex_world[b], f)), f
        want = Tx.bake_field(G, pb, world[b].vertices, world[b].triangles, texels=4)
        for got in (tex_index[b].texture, tex_world[b].texture):                                    # baked on the world vertices whatever `units` returns
            assert torch.equal(got.image, want.image) and got.atlas == want.atlas and got.uvs.tobytes() == want.uvs.tobytes()
        assert counts[b].atlas == want.atlas and want.image.numel() > 0 and int(want.image.max()) > 0


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_mt_gpu_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_take_the_texture_flags(tdgp, tmp_path, capsys):
    from PIL import Image
    cfg = tdgp.config.config_tiny()
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    ex = _tool('extract_geometry')
    common = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--volume-res', '24', '--cube-size', str(2.0 * cfg.cube_scale), '--thresh-value', '0.0', '--save-obj', '--no-save-mrc']
    ex.main(common + ['--output-dir', str(tmp_path / 'raw')])
    capsys.readouterr()
    ex.main(common + ['--output-dir', str(tmp_path / 'tex'), '--texture-texels', '3'])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
    assert [ln['name'] for ln in lines] == ['0000', '0001'] and all(ln['texture_texels'] == 3 for ln in lines)
    checked = 0
    for ln in lines:
        name = ln['name']
        raw, obj = open(tmp_path / 'raw' / f'{name}.obj').read(), open(tmp_path / 'tex' / f'{name}.obj').read()
        assert 'vt ' not in raw and not os.path.exists(tmp_path / 'raw' / f'{name}.mtl') and not os.path.exists(tmp_path / 'raw' / f'{name}.png')
        nt = raw.count('\nf ')
        assert ln['triangles'] == nt and ln['atlas'] == list(tdgp.mesh_texture.atlas_layout(nt, 3)[3:])
        if nt == 0:
            continue
        checked += 1
        assert [x for x in raw.splitlines() if x.startswith('v ')] == [x for x in obj.splitlines() if x.startswith('v ')]
        assert obj.startswith(f'mtllib {name}.mtl\n') and obj.count('\nvt ') == 3 * nt and re.search(r'\nusemtl baked\nf \d+/1 \d+/2 \d+/3\n', obj)
        assert open(tmp_path / 'tex' / f'{name}.mtl').read() == f'newmtl baked\nKd 1 1 1\nmap_Kd {name}.png\n'
        png = np.asarray(Image.open(tmp_path / 'tex' / f'{name}.png'))
        assert png.shape == (ln['atlas'][1], ln['atlas'][0], 3) and png.max() > 0
    assert checked >= 1
    rt = _tool('render_trajectory')
    base = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--trajectory', 'front_circle', '--num-frames', '2', '--level', '0.0', '--volume-res', '24', '--seed', '5']
    rt.main(base + ['--vis', 'mesh_grid', '--out', str(tmp_path / 'plain.npy')])
    rt.main(base + ['--vis', 'mesh_grid', '--out', str(tmp_path / 'tex.npy'), '--mesh-texture-texels', '3'])
    rt.main(base + ['--vis', 'mesh_strips', '--out', str(tmp_path / 'strips.npy'), '--mesh-texture-texels', '3', '--mesh-texture-filter', 'nearest', '--mesh-normals', 'vertex'])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 3 and 'mesh_texture_texels' not in lines[0] and lines[0]['shape_mode'] == 'shaded'
    assert lines[1]['mesh_texture_texels'] == 3 and lines[1]['mesh_texture_filter'] == 'bilinear' and lines[1]['shape_mode'] == 'colour' and lines[1]['triangles'] == lines[0]['triangles']
    assert lines[1]['atlas'] == [list(tdgp.mesh_texture.atlas_layout(nt, 3)[3:]) for nt in lines[1]['triangles']]
    assert lines[2]['mesh_texture_filter'] == 'nearest' and lines[2]['atlas'] == lines[1]['atlas']
    a, b = np.load(tmp_path / 'plain.npy'), np.load(tmp_path / 'tex.npy')
    assert a.shape == b.shape == tuple(lines[1]['shape']) and a.dtype == b.dtype == np.uint8

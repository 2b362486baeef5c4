"""Mesh textures without a GPU: the properties of the atlas layout and of the numpy restatement (tests/mesh_texture_reference.py) that make it
worth being the yardstick of the device tests -- every owned texel has one owner, corner UVs are texel centres, charts keep their
orientation, a colour that is linear in position comes back from a bilinear fetch with nothing but the 8-bit quantisation -- and the host
side of the feature: `atlas_layout` / `atlas_uvs` of 3dgp_amd/mesh_texture.py against the restatement, `save_obj` with uvs / texture, and
the option errors of the drivers and the two command lines."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import mesh_raster_reference as MR
import mesh_texture_reference as R

F = np.float32
D = np.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('tdgp_atlas_points', 'tdgp_atlas_texels', 'tdgp_mesh_sample_texture')


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_mt_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the layout
CASES = [(T, n) for T in (1, 2, 3, 4, 5, 7, 8, 9, 18, 19, 32, 33, 80) for n in (2, 3, 8)] + [(1, 64), (6, 64)]


def test_layout_is_the_formula_and_the_module_agrees(tdgp):
    Tx = tdgp.mesh_texture
    for T, n in CASES + [(0, 2), (0, 8)]:
        a = Tx.atlas_layout(T, n)
        assert tuple(a) == tuple(R.atlas_layout(T, n)) and a._fields == ('texels', 'tile', 'tiles_per_row', 'width', 'height')
        P, r = (T + 1) // 2, a.tiles_per_row
        assert a.texels == n and a.tile == n + 2 and r * r >= P and (r == 0 or (r - 1) ** 2 < P)
        assert a.width == r * (n + 2) and a.height == (0 if r == 0 else -(-P // r)) * (n + 2)
        uv = Tx.atlas_uvs(T, a)
        assert uv.dtype == np.float32 and uv.shape == (T, 3, 2) and uv.tobytes() == R.atlas_uvs(T, a).tobytes()
    assert tuple(Tx.atlas_layout(0, 8)) == (8, 10, 0, 0, 0)                          # T == 0: an empty image
    assert tuple(Tx.atlas_layout(1, 8)) == (8, 10, 1, 10, 10)                        # T == 1: one tile, its upper half unowned
    assert tuple(Tx.atlas_layout(18, 2)) == (2, 4, 3, 12, 12)                        # P = 9 = 3^2
    assert tuple(Tx.atlas_layout(19, 2)) == (2, 4, 4, 16, 12)                        # P = 10, one past a square: a new column, the last row short
    assert tuple(Tx.atlas_layout(32, 2)) == (2, 4, 4, 16, 16)                        # P = 16: 256 texels


def test_every_owned_texel_has_exactly_one_owner():
    for T, n in CASES:
        a = R.atlas_layout(T, n)
        t, qx, qy = R.texel_owner(T, a)
        S = n + 2
        P = (T + 1) // 2
        counts = np.bincount(t[t >= 0], minlength=T)
        lower, upper = (n + 1) * (n + 2) // 2, S * S - (n + 1) * (n + 2) // 2
        assert (counts[0::2] == lower).all() and (counts[1::2] == upper).all()      # a partition of each tile: no texel twice, none lost
        assert (t >= 0).sum() == (T // 2) * S * S + (T % 2) * lower
        # unowned: the tiles >= P and the upper half of the last tile when T is odd
        col, row = np.meshgrid(np.arange(a.width), np.arange(a.height))
        tile = (row // S) * a.tiles_per_row + col // S
        assert ((t < 0) == ((tile >= P) | ((T % 2 == 1) & (tile == P - 1) & ((col % S) + (row % S) > n)))).all()
        # every owner sees each of its texel coordinates once, and they cover the chart with its gutter
        for k in {0, T - 1, T // 2}:
            q = set(zip(qx[t == k].tolist(), qy[t == k].tolist()))
            assert len(q) == (t == k).sum() and q == {(x, y) for x in range(S) for y in range(S) if x + y <= (n if k % 2 == 0 else n + 1)}
        _, owner = R.atlas_points(np.zeros((3, 3), F), np.tile(np.array([[0, 1, 2]], np.int32), (T, 1)), a)
        assert (owner.reshape(a.height, a.width) == t).all()


def test_corner_uvs_land_on_texel_centres_and_keep_the_orientation():
    for T, n in CASES:
        a = R.atlas_layout(T, n)
        t, qx, qy = R.texel_owner(T, a)
        uv = R.atlas_uvs(T, a).astype(D)
        x, y = uv[..., 0] * a.width - 0.5, (1.0 - uv[..., 1]) * a.height - 0.5
        xi, yi = np.rint(x).astype(int), np.rint(y).astype(int)
        assert np.abs(x - xi).max() < 1e-3 and np.abs(y - yi).max() < 1e-3
        want_q = [(0, 0), (n - 1, 0), (0, n - 1)]
        for k in range(T):
            for i in range(3):
                assert t[yi[k, i], xi[k, i]] == k and (qx[yi[k, i], xi[k, i]], qy[yi[k, i], xi[k, i]]) == want_q[i]
        # orientation: the chart's signed area in image coordinates (x right, y down) is positive for lower and upper triangles alike (the
        # upper one is the lower one turned by a half turn, a rotation), so in (u, v) with v up every chart has the same negative sign
        ex, ey = x[:, 1:] - x[:, :1], y[:, 1:] - y[:, :1]
        area = ex[:, 0] * ey[:, 1] - ex[:, 1] * ey[:, 0]
        assert np.allclose(area, (n - 1) ** 2, atol=1e-2)
        du, dv = uv[:, 1:, 0] - uv[:, :1, 0], uv[:, 1:, 1] - uv[:, :1, 1]
        assert ((du[:, 0] * dv[:, 1] - du[:, 1] * dv[:, 0]) < 0).all()


def test_limits(tdgp):
    Tx = tdgp.mesh_texture
    for T, n in ((4, 1), (4, 65), (4, 0), (4, -3), (4, 2.5), (-1, 8)):
        with pytest.raises(ValueError):
            Tx.atlas_layout(T, n)
    # 16384 / 66 = 248.2: 248 tiles of 64 texels per row fit, 249 do not
    ok = Tx.atlas_layout(2 * 248 * 248, 64)
    assert ok.width == ok.height == 248 * 66 <= 16384
    with pytest.raises(ValueError, match='16384'):
        Tx.atlas_layout(2 * 248 * 248 + 1, 64)
    assert Tx.atlas_layout(2 * 4096 * 4096, 2).width == 16384
    with pytest.raises(ValueError, match='16384'):
        Tx.atlas_layout(2 * 4096 * 4096 + 1, 2)
    with pytest.raises(ValueError, match='not the atlas'):
        Tx.atlas_uvs(5, Tx.atlas_layout(9, 8))
    with pytest.raises(TypeError):
        Tx.atlas_uvs(5, (8, 10, 2, 20, 20))


def test_entry_points_are_declared_bound_and_check_their_arguments(tdgp):
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    for name in NEW:
        assert re.search(rf'\b{name}\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)) and name in tdgp._lib.EXPORTS
    assert 'mesh_texture.hip' in tdgp.build.SOURCES
    assert 'mesh_bary_weights' in open(os.path.join(REPO, '3dgp_amd', 'csrc', 'mesh_texture.hip')).read()       # the shared weights, not a restatement
    lib = tdgp._lib.load()
    # the argument checks of the C side come before any launch: they answer without a device
    import ctypes
    fill = (ctypes.c_uint8 * 3)(1, 2, 3)
    EINVAL, EUNSUPPORTED = -1, -2
    points = lambda T, n, r, W, H: lib.tdgp_atlas_points(None, 0, None, T, n, r, W, H, None, None, None)      # noqa: E731
    assert points(0, 8, 0, 0, 0) == 0                                                   # T == 0: nothing to launch
    assert points(4, 1, 2, 6, 3) == EINVAL and b'texels' in lib.tdgp_last_error()
    assert points(4, 65, 2, 134, 67) == EINVAL and b'[2, 64]' in lib.tdgp_last_error()
    assert points(4, 8, 2, 20, 20) == EINVAL and b'not the atlas' in lib.tdgp_last_error()          # P = 2: r = 2, but H = 10
    assert points(4, 8, 1, 10, 20) == EINVAL
    assert points(2 * 248 * 248 + 1, 64, 249, 249 * 66, 248 * 66) == EUNSUPPORTED and b'16384' in lib.tdgp_last_error()
    assert points(4, 8, 2, 20, 10) == EINVAL and b'null' in lib.tdgp_last_error()                   # the right atlas, no arrays
    assert lib.tdgp_atlas_texels(None, 2, None, 4, fill, None, None) == EINVAL and b'rgb_stride' in lib.tdgp_last_error()
    assert lib.tdgp_atlas_texels(None, 4, None, 4, None, None, None) == EINVAL and b'fill' in lib.tdgp_last_error()
    assert lib.tdgp_atlas_texels(None, 4, None, 0, fill, None, None) == 0
    assert lib.tdgp_atlas_texels(None, 4, None, 4, fill, None, None) == EINVAL
    sample = lambda rays, T, n, r, W, H, filt: lib.tdgp_mesh_sample_texture(None, None, None, None, None, rays, None, 0, None, T, None, n, r, W, H, filt, None, None)      # noqa: E731
    assert sample(0, 4, 8, 2, 20, 10, 1) == 0
    assert sample(5, 4, 8, 2, 20, 10, 2) == EINVAL and b'filter' in lib.tdgp_last_error()
    assert sample(5, 4, 8, 2, 20, 20, 1) == EINVAL and b'not the atlas' in lib.tdgp_last_error()
    assert sample(5, 4, 8, 2, 20, 10, 1) == EINVAL and b'null' in lib.tdgp_last_error()
    assert sample(-1, 4, 8, 2, 20, 10, 1) == EINVAL


# ------------------------------------------------------------------------------------------------ what the unclamped gutter is for
def _linear_colour(seed):
    rs = np.random.RandomState(seed)
    A, c = rs.uniform(-0.25, 0.25, (3, 3)), rs.uniform(-0.2, 0.2, 3)
    return (lambda p: (np.asarray(p, D) @ A.T + c).astype(F)), A, c


def test_bilinear_fetch_reproduces_a_linear_colour_up_to_quantisation():
    """A colour that is linear in position, c(x) = A x + c0 with |c| < 1 on the mesh: every owned texel -- gutter included, sampled on the
    triangle's plane beyond the hypotenuse -- holds round(255 * (c * 0.5 + 0.5)), off by at most 0.5 / 255 from the linear function, and a
    bilinear fetch is a convex combination of four texels of the SAME linear function whose weights reproduce a linear function exactly, so it
    is off by at most 0.5 / 255 too: quantisation is the only error (the fp32 roundings of the colour, of k and of the result, and the
    float64 ones of the weights, are four orders of magnitude below it and the data here are seeded).  Checked at random interior points, on
    the three edges -- the hypotenuse is the case the gutter exists for -- and at the corners, for lower and upper triangles and an odd T."""
    v, t = MR.icosphere(1)
    v, t = v[:], t[:21]                                                               # an odd count: the last tile's upper half is unowned
    fn, A, c0 = _linear_colour(5)
    bound = 0.5 / 255
    rs = np.random.RandomState(11)
    for n in (2, 3, 8, 16):
        image, _, atlas, _, owner = R.bake(v, t, fn, n)
        assert (image.reshape(-1, 3)[owner < 0] == 0).all()
        N = 40
        k = np.repeat(np.arange(len(t)), N)
        b = rs.dirichlet([1, 1, 1], len(k))
        b[0::N] = (1, 0, 0)
        b[1::N] = (0, 1, 0)
        b[2::N] = (0, 0, 1)                                                           # the corners
        s = rs.rand(len(k))
        for j, (i0, i1) in enumerate(((1, 2), (0, 1), (0, 2))):                       # the hypotenuse v1-v2 first, then the legs
            rows = np.arange(3 + j, len(k), N)
            b[rows] = 0
            b[rows, i0], b[rows, i1] = s[rows], 1 - s[rows]
        P = v[t[k]].astype(D)
        x = ((b[:, :1] * P[:, 0] + b[:, 1:2] * P[:, 1]) + b[:, 2:] * P[:, 2]).astype(F)
        # the hit as the kernel forms it: o + d * t_hit with o = 0, d = x, t_hit = 1
        args = (k.astype(np.int32), np.ones(len(k), np.int32), np.ones(len(k), F), np.zeros_like(x), x, v, t, image, atlas)
        want = (x.astype(D) @ A.T + c0) * 0.5 + 0.5
        assert want.min() > 0.05 and want.max() < 0.95                                # never clamped: the function stays linear
        got = R.sample_texture(*args, 'bilinear').astype(D)
        err = np.abs(got - want)
        print(f'texels {n}: worst bilinear error {err.max() * 255:.4f} / 255 (hypotenuse {err[3::N].max() * 255:.4f}, corners {err[0::N].max() * 255:.4f})')
        assert err.max() <= bound
        # nearest is off by the quantisation plus the colour's change over half a texel diagonal: not exact, and worse than bilinear on average
        near = np.abs(R.sample_texture(*args, 'nearest').astype(D) - want)
        assert near.mean() > err.mean()
    # and it is the gutter that does it: with the gutter's texels replaced by the fill, the hypotenuse is wrong
    image, _, atlas, _, _ = R.bake(v, t, fn, 8)
    tt, qx, qy = R.texel_owner(len(t), atlas)
    cut = image.copy()
    cut[(qx + qy > 7)] = 0
    k = np.arange(len(t), dtype=np.int32)
    P = v[t].astype(D)
    x = (0.37 * P[:, 1] + 0.63 * P[:, 2]).astype(F)
    args = (k, np.ones(len(k), np.int32), np.ones(len(k), F), np.zeros_like(x), x, v, t)
    want = (x.astype(D) @ A.T + c0) * 0.5 + 0.5
    assert np.abs(R.sample_texture(*args, image, atlas, 'bilinear') - want).max() <= bound
    assert np.abs(R.sample_texture(*args, cut, atlas, 'bilinear') - want).max() > 20 * bound


def test_restatement_edge_cases():
    """Misses, bad triangles and needles are defined; texels quantise as stated."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]], F)
    t = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 9], [1, 1, 1]], np.int32)              # a triangle, a needle, a bad index, a point
    fn = lambda p: np.concatenate([p[:, :2], p[:, :1] * 0 - 3.0, p[:, :1] * 0 + np.nan], axis=1).astype(F)      # noqa: E731
    image, uvs, atlas, points, owner = R.bake(v, t, fn, 4, fill=(9, 8, 7))
    assert tuple(atlas) == (4, 6, 2, 12, 6) and image.shape == (6, 12, 3) and np.isfinite(points).all()
    assert set(np.unique(owner)) == {-1, 0, 1, 3} and (image.reshape(-1, 3)[owner < 0] == (9, 8, 7)).all()     # triangle 2 names vertex 9: unowned
    assert (image[..., 2].reshape(-1)[owner >= 0] == 0).all()                         # -3 * 0.5 + 0.5 < 0 -> 0
    assert image[0, 0].tolist() == [128, 128, 0] and image[0, 3].tolist() == [255, 128, 0]          # v0 -> rint(127.5) = 128 (half to even), v1 -> 255
    assert R.atlas_texels(np.array([[np.nan, 7.0, -0.0]], F), [0]).tolist() == [[0, 255, 128]]
    tri = np.array([0, 1, 2, 3, 4, -1, 0], np.int32)
    status = np.array([1, 1, 1, 1, 1, 1, 0], np.int32)
    x = np.tile(np.array([[0.25, 0.25, 0.0]], F), (7, 1))
    for filt in ('nearest', 'bilinear'):
        got = R.sample_texture(tri, status, np.ones(7, F), np.zeros_like(x), x, v, t, image, atlas, filt)
        assert np.isfinite(got).all() and (got[[2, 4, 5, 6]] == 0).all() and (got[0, :2] > 0).all()
    assert R.bake(v, t[:0], fn, 4)[0].shape == (0, 0, 3)


# ------------------------------------------------------------------------------------------------ the .obj writer
def test_save_obj_with_uvs_and_texture_reads_back(tdgp, tmp_path):
    from PIL import Image
    g, Tx = tdgp.geometry, tdgp.mesh_texture
    v, t = MR.icosphere(1, 0.3)
    fn, _, _ = _linear_colour(2)
    image, uvs, atlas, _, _ = R.bake(v, t, fn, 5)
    vn = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    g.save_obj(str(tmp_path / 'plain.obj'), v, t)
    g.save_obj(str(tmp_path / 'none.obj'), v, t, uvs=None, texture=None)
    assert open(tmp_path / 'plain.obj', 'rb').read() == open(tmp_path / 'none.obj', 'rb').read()
    before = ''.join(f'v {np.format_float_positional(x, unique=True, trim="-")} {np.format_float_positional(y, unique=True, trim="-")} '
                     f'{np.format_float_positional(z, unique=True, trim="-")}\n' for x, y, z in v) + ''.join(f'f {a + 1} {b + 1} {c + 1}\n' for a, b, c in t.tolist())
    assert open(tmp_path / 'plain.obj').read() == before                               # the bytes this writer always wrote
    g.save_obj(str(tmp_path / 'n.obj'), v, t, normals=vn)
    assert '//' in open(tmp_path / 'n.obj').read() and 'vt ' not in open(tmp_path / 'n.obj').read()
    assert sorted(os.listdir(tmp_path)) == ['n.obj', 'none.obj', 'plain.obj']          # no .mtl / .png without a texture

    def read(path):
        out = dict(v=[], vn=[], vt=[], f=[], other=[])
        for ln in open(path).read().splitlines():
            key, rest = ln.split(' ', 1)
            if key == 'f':
                out['f'].append([[int(x) if x else None for x in c.split('/')] for c in rest.split()])
            elif key in out:
                out[key].append([F(x) for x in rest.split()])
            else:
                out['other'].append(ln)
        return out

    for normals in (None, vn):
        name = 'tex' if normals is None else 'texn'
        g.save_obj(str(tmp_path / f'{name}.obj'), v, t, normals=normals, uvs=uvs, texture=torch.as_tensor(image))
        o = read(tmp_path / f'{name}.obj')
        assert np.array(o['v'], F).tobytes() == v.tobytes() and np.array(o['vt'], F).reshape(-1, 3, 2).tobytes() == uvs.tobytes()
        assert o['other'] == [f'mtllib {name}.mtl', 'usemtl baked']
        f = np.array([[[x for x in c] for c in face] for face in o['f']], object)
        assert (f[:, :, 0].astype(int) - 1 == t).all() and (f[:, :, 1].astype(int) == 3 * np.arange(len(t))[:, None] + np.arange(3)[None, :] + 1).all()
        if normals is None:
            assert f.shape[2] == 2 and not o['vn']
        else:
            assert (f[:, :, 2].astype(int) == f[:, :, 0].astype(int)).all() and np.array(o['vn'], F).tobytes() == vn.tobytes()
        assert open(tmp_path / f'{name}.mtl').read().split('\n') == ['newmtl baked', 'Kd 1 1 1', f'map_Kd {name}.png', '']
        png = np.asarray(Image.open(tmp_path / f'{name}.png'))
        assert png.dtype == np.uint8 and png.shape == image.shape and (png == image).all()
    # uvs alone: vt lines and a/ta faces, no material; a Texture brings its own uvs
    g.save_obj(str(tmp_path / 'uv.obj'), v, t, uvs=uvs)
    o = read(tmp_path / 'uv.obj')
    assert o['other'] == [] and len(o['vt']) == 3 * len(t) and not os.path.exists(tmp_path / 'uv.mtl')
    g.save_obj(str(tmp_path / 'whole.obj'), v, t, texture=Tx.Texture(torch.as_tensor(image), uvs, Tx.Atlas(*atlas)))
    assert open(tmp_path / 'whole.obj').read() == open(tmp_path / 'tex.obj').read().replace('tex.mtl', 'whole.mtl')
    for call in (lambda: g.save_obj(str(tmp_path / 'bad.obj'), v, t, uvs=uvs[:-1]), lambda: g.save_obj(str(tmp_path / 'bad.obj'), v, t, texture=image),
                 lambda: g.save_obj(str(tmp_path / 'bad.obj'), v, t, uvs=uvs, texture=image[..., :2])):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------ options
def test_option_errors_of_the_drivers(tdgp):
    Tx, M, g = tdgp.mesh_texture, tdgp.mesh, tdgp.geometry
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    fn = lambda p: p              # noqa: E731
    tex = Tx.Texture(torch.zeros(10, 10, 3, dtype=torch.uint8), Tx.atlas_uvs(2, Tx.atlas_layout(2, 8)), Tx.atlas_layout(2, 8))
    cams = dict(angles=torch.zeros(1, 3), radius=torch.ones(1), look_at=torch.zeros(1, 3), fov=torch.full((1,), 40.0))
    bad = [lambda: Tx.bake(v, t, fn, texels=1), lambda: Tx.bake(v, t, fn, texels=65), lambda: Tx.bake(v, t, fn, fill=(0, 0)), lambda: Tx.bake(v, t, fn, fill=(0, 0, 256)),
           lambda: Tx.bake(v.double(), t, fn), lambda: Tx.bake(v, t.long(), fn),
           lambda: Tx.check_options(dict(texels=8, colour='red')), lambda: Tx.check_options(dict(texels=1)), lambda: Tx.check_options(dict(filter='cubic')),
           lambda: Tx.check_options(dict(points_per_call=0)), lambda: Tx.check_options(dict(fill=(1, 2))),
           lambda: M.render_mesh_views(v, t, cams, 8, mode='colour', normals='field', planes=object(), G=object(), texture=tex),
           lambda: M.render_mesh_views(v, t, cams, 8, mode='shaded', texture=tex), lambda: M.render_mesh_views(v, t, cams, 8, mode='normals', texture=tex),
           lambda: M.render_mesh_views(v, t, cams, 8, mode='colour', texture=tex, texture_filter='cubic'),
           lambda: g.extract_geometry(None, None, texture=dict(texels=100)), lambda: g.extract_geometry(None, None, texture=dict(texel=8))]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'call {k} did not raise')
    for call in (lambda: Tx.check_options(8), lambda: g.extract_geometry(None, None, texture=8)):
        with pytest.raises(TypeError):
            call()
    assert Tx.check_options(dict()) == (dict(texels=8), 'bilinear')
    assert Tx.check_options(dict(texels=6, filter='nearest', fill=(1, 2, 3), points_per_call=1000)) == (dict(texels=6, fill=(1, 2, 3), points_per_call=1000), 'nearest')
    with pytest.raises(RuntimeError, match='GPU'):                                     # well-formed, on the host: the kernels have no CPU path
        Tx.bake(v, t, fn)
    # a texture of another mesh: its uvs do not have T rows
    with pytest.raises(ValueError, match='another mesh'):
        Tx._check_texture(tex, 3)
    with pytest.raises(ValueError, match='uint8'):
        Tx._check_texture(Tx.Texture(tex.image[:5], tex.uvs, tex.atlas), 2)
    with pytest.raises(TypeError):
        Tx._check_texture((tex.image, tex.uvs, tex.atlas), 2)
    c = g.MeshCount(7, 9, 30)
    assert c == (7, 9) and c.atlas is None and g.TexturedShape._fields == ('vertices', 'triangles', 'sigma', 'texture') and g.Shape._fields == ('vertices', 'triangles', 'sigma')


def test_tools_usage_errors(capsys):
    ex, rt = _tool('extract_geometry'), _tool('render_trajectory')
    base = ['--seeds', '0']
    a = ex.parse_args(base)
    assert ex.texture_options(a) is None and not any(k.startswith('texture') for k in vars(a))
    assert ex.texture_options(ex.parse_args(base + ['--save-obj', '--texture-texels', '6'])) == dict(texels=6)
    assert ex.texture_options(ex.parse_args(base + ['--save-obj', '--save-ply', '--texture-texels', '64'])) == dict(texels=64)
    for extra in (['--texture-texels', '6'], ['--save-ply', '--texture-texels', '6'], ['--save-obj', '--texture-texels', '1'], ['--save-obj', '--texture-texels', '65'],
                  ['--save-obj', '--texture-texels', 'fine']):
        with pytest.raises(SystemExit):
            ex.parse_args(base + extra)
    p = rt.build_parser()
    base = ['--ckpt', 'x', '--out', 'y.npy']
    o = rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_grid', '--mesh-texture-texels', '4']))
    assert o['texture'] == dict(texels=4, filter='bilinear') and o['mode'] == 'colour'
    o = rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_strips', '--mesh-texture-texels', '4', '--mesh-texture-filter', 'nearest', '--mesh-normals', 'vertex']))
    assert o['texture'] == dict(texels=4, filter='nearest') and o['normals'] == 'vertex'
    o = rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_strips']))
    assert 'texture' not in o and o['mode'] == 'shaded'
    for extra in (['--mesh-texture-texels', '4'], ['--vis', 'shape_grid', '--mesh-texture-texels', '4'], ['--vis', 'mesh_grid', '--mesh-texture-filter', 'nearest'],
                  ['--vis', 'mesh_grid', '--mesh-texture-texels', '1'], ['--vis', 'mesh_grid', '--mesh-texture-texels', '65'],
                  ['--vis', 'mesh_grid', '--mesh-texture-texels', '4', '--mesh-texture-filter', 'cubic'],
                  ['--vis', 'mesh_grid', '--mesh-texture-texels', '4', '--mesh-normals', 'field'], ['--vis', 'video_grid', '--mesh-texture-filter', 'nearest']):
        with pytest.raises(SystemExit):
            p.parse_args(base + extra)
    capsys.readouterr()

"""Shape frames on the GPU: tdgp_iso_bracket / tdgp_iso_locate / tdgp_iso_shade bit for bit against the numpy restatement of their contracts
(tests/shapes_reference.py) at the sizes where the lane mapping can go wrong, their refusals with nothing launched, and `shapes.render_shape_views`
and the wrappers on a seeded config_tiny scene: bit for bit against the restated chain fed with the product's own field values, under every
chunking, through the image and grid layouts, for a two- and a three-layer decoder, and against the density grid of the mesh route."""
import ctypes

import numpy as np
import pytest
import torch

import shapes_reference as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.as_tensor(a).to(DEV)


def H(t):
    return t.detach().cpu().numpy()


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert not (got.dtype.kind == 'f' and np.isnan(got).any()), f'{what}: NaN in an output the contract keeps finite'
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32 if got.itemsize == 4 else np.uint8) != want.view(np.uint32 if want.itemsize == 4 else np.uint8))
        first = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}')


# ------------------------------------------------------------------------------------------------ rows
def make_rows(rays, n, level, seed):
    """[rays, n] densities around `level`, row r of kind r % 12: no crossing; a crossing at k = 0; one at k = n-1 only; several (the first
    wins); a value equal to the level as the first crossing; a NaN before the crossing; a NaN where the crossing would be; +inf as the crossing;
    -inf before it; a flat pair at the end under the level; all NaN; a ramp.  Short rows keep what fits."""
    rs = np.random.RandomState(seed)
    lv = np.float32(level)
    below = (lv - np.float32(0.25) - rs.rand(rays, n).astype(np.float32) * 3).astype(np.float32)
    above = (lv + np.float32(0.25) + rs.rand(rays, n).astype(np.float32) * 3).astype(np.float32)
    x = below.copy()
    k = rs.randint(0, n, size=rays)                              # where the row first reaches the level
    for r in range(rays):
        kind, c = r % 12, int(k[r])
        if kind == 0:
            pass
        elif kind == 1:
            x[r, 0] = above[r, 0]
        elif kind == 2:
            x[r, n - 1] = above[r, n - 1]
        elif kind == 3:
            x[r, c:] = np.where(rs.rand(n - c) < 0.5, above[r, c:], below[r, c:])
            x[r, c] = above[r, c]
        elif kind == 4:
            x[r, c] = lv
        elif kind == 5:
            x[r, c] = above[r, c]
            if c > 0:
                x[r, rs.randint(0, c)] = np.nan
        elif kind == 6:
            x[r, c] = np.nan
            if c + 1 < n:
                x[r, c + 1] = above[r, c + 1]
        elif kind == 7:
            x[r, c] = np.inf
        elif kind == 8:
            x[r, c] = above[r, c]
            if c > 0:
                x[r, c - 1] = -np.inf
        elif kind == 9:
            x[r, max(n - 2, 0):] = x[r, n - 1]
        elif kind == 10:
            x[r, :] = np.nan
        else:
            x[r] = np.sort(np.concatenate([below[r, :c], above[r, c:]]))
    return x


def make_depths(rays, n, seed):
    rs = np.random.RandomState(seed)
    return (np.float32(0.7) + np.cumsum(rs.rand(rays, n).astype(np.float32) * np.float32(0.01) + np.float32(1e-4), axis=1, dtype=np.float32)).astype(np.float32)


def strided(x, stride, seed):
    """A device view [rays, n] of the values x at an element stride of 1 (contiguous) or 4 (column 3 of rows [., 4], the other columns random)."""
    if stride == 1:
        return T(x)
    rows = np.random.RandomState(seed).randn(x.shape[0], x.shape[1], 4).astype(np.float32)
    rows[..., 3] = x
    return T(rows)[..., 3]


RAYS = (1, 63, 64, 65, 1000)
STEPS = (2, 5, 16, 64, 65, 512)
REFINE = (1, 2, 5, 16, 33, 64)        # 5 and 33: a lane group wider than N (the `l < N` guard) and fractions (j+1)/N that round


@pytest.mark.parametrize('S', STEPS)
@pytest.mark.parametrize('rays', RAYS)
def test_bracket_and_locate_bit_for_bit(tdgp, rays, S):
    """Every N of REFINE, sigma at strides 1 and 4, a positive and a negative level: idx, t_fine, t_hit, status and points are the restatement's
    bytes.  `locate` is fed fine densities of the same twelve kinds of row, so every branch of both kernels is met at every lane mapping."""
    Sh = tdgp.shapes
    seed = rays * 1000 + S
    t = make_depths(rays, S, seed)
    rs = np.random.RandomState(seed + 1)
    o = rs.randn(rays, 3).astype(np.float32)
    d = rs.randn(rays, 3).astype(np.float32)
    for level in (0.5, -3.0):
        sigma = make_rows(rays, S, level, seed + 2)
        for N in REFINE:
            idx_w, fine_w = SR.bracket(sigma, t, N, level)
            sig_f = np.roll(make_rows(rays, N, level, seed + 3 + N), 5, axis=0)       # the kinds of the fine rows are not aligned with the coarse ones
            th_w, st_w, pts_w = SR.locate(sigma, t, idx_w, sig_f, fine_w, o, d, level, 1.0 / 32, 1.25)
            for stride in (1, 4):
                what = f'rays={rays} S={S} N={N} level={level} stride={stride}'
                idx, fine = Sh.iso_bracket(strided(sigma, stride, seed), T(t), N, level)
                same_bytes(H(idx), idx_w, 'idx ' + what)
                same_bytes(H(fine), fine_w, 't_fine ' + what)
                th, st, pts = Sh.iso_locate(strided(sigma, stride, seed), T(t), idx, strided(sig_f, stride, seed + 9), fine, T(o), T(d), level, 1.0 / 32, 1.25)
                same_bytes(H(st), st_w, 'status ' + what)
                same_bytes(H(th), th_w, 't_hit ' + what)
                same_bytes(H(pts), pts_w, 'points ' + what)
        if rays >= 63:
            assert set(np.unique(st_w)) == {0, 1, 2}, np.unique(st_w)


@pytest.mark.parametrize('rays', RAYS)
def test_shade_bit_for_bit(tdgp, rays):
    """All three modes, headlight and fixed light, with and without the normal output; the stencil rows hold a zero gradient, a NaN, infinities and
    a gradient whose square overflows, and every status."""
    Sh = tdgp.shapes
    rs = np.random.RandomState(rays)
    stencil = (rs.randn(rays, 7, 4) * 2).astype(np.float32)
    for r in range(rays):
        kind = r % 8
        if kind == 1:
            stencil[r, 1:, 3] = stencil[r, 1, 3]                                  # zero gradient -> the ray's direction
        elif kind == 2:
            stencil[r, 1 + rs.randint(6), 3] = np.nan
        elif kind == 3:
            stencil[r, 1 + rs.randint(6), 3] = np.inf
        elif kind == 4:
            stencil[r, 1, 3], stencil[r, 2, 3] = 3e19, -3e19                      # g finite, g * g = inf
        elif kind == 5:
            stencil[r, 0, :3] = [np.nan, -7.0, 7.0]                               # colour mode: NaN -> 0, clamps on both sides
        elif kind == 6:
            stencil[r, 1, 3] = stencil[r, 2, 3] = np.inf                          # inf - inf
    status = (np.arange(rays) // 8 % 3).astype(np.int32)
    d = rs.randn(rays, 3).astype(np.float32)
    light = (0.36, 0.48, 0.8)
    for mode in ('shaded', 'normals', 'colour'):
        for lt in (None, light):
            kw = dict(light=lt, ambient=0.3, albedo=(0.9, 0.5, 0.7), background=(1.0, -0.5, 0.25))
            rgb_w, n_w = SR.shade(stencil, status, d, mode, **kw)
            rgb, n = Sh.iso_shade(T(stencil), T(status), T(d), mode=mode, **kw)
            same_bytes(H(rgb), rgb_w, f'rgb rays={rays} {mode} light={lt}')
            same_bytes(H(n), n_w, f'normal rays={rays} {mode} light={lt}')
            rgb2, n2 = Sh.iso_shade(T(stencil), T(status), T(d), mode=mode, return_normal=False, **kw)
            assert n2 is None
            same_bytes(H(rgb2), rgb_w, f'rgb without normal rays={rays} {mode} light={lt}')


def test_refusals_launch_nothing(tdgp):
    """S = 1 and 513, N = 0 and 65 are refused by both entry points, and the outputs keep the values they held."""
    L = tdgp._lib
    rays = 8
    buf = lambda n, dt=torch.float32: torch.full([n], 7, dtype=dt, device=DEV)       # noqa: E731
    sig, t, fine, sigf, o = buf(rays * 513), buf(rays * 513), buf(rays * 65), buf(rays * 65), buf(rays * 3)
    idx, st, th, pts = buf(rays, torch.int32), buf(rays, torch.int32), buf(rays), buf(rays * 21)
    s = L.stream_of(sig)
    for S, N, exc in ((1, 16, RuntimeError), (513, 16, L.Unsupported), (16, 0, RuntimeError), (16, 65, L.Unsupported)):
        with pytest.raises(RuntimeError, match='iso_bracket') as e:
            L.call('tdgp_iso_bracket', sig.data_ptr(), 1, t.data_ptr(), rays, S, N, 0.0, idx.data_ptr(), fine.data_ptr(), s)
        assert type(e.value) is exc
        with pytest.raises(RuntimeError, match='iso_locate') as e:
            L.call('tdgp_iso_locate', sig.data_ptr(), 1, t.data_ptr(), idx.data_ptr(), sigf.data_ptr(), 1, fine.data_ptr(), o.data_ptr(), o.data_ptr(), rays, S, N,
                   0.0, 0.1, 1.0, th.data_ptr(), st.data_ptr(), pts.data_ptr(), s)
        assert type(e.value) is exc
    with pytest.raises(RuntimeError, match='iso_shade'):
        L.call('tdgp_iso_shade', pts.data_ptr(), st.data_ptr(), o.data_ptr(), rays, 3, None, 0.2, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), th.data_ptr(), None, s)
    L.call('tdgp_iso_bracket', sig.data_ptr(), 1, t.data_ptr(), 0, 16, 16, 0.0, idx.data_ptr(), fine.data_ptr(), s)          # rays == 0: a no-op
    torch.cuda.synchronize()
    for x in (idx, st, th, pts, fine):
        assert bool((x == 7).all())


# ------------------------------------------------------------------------------------------------ the route on a scene
B, V = 2, 3
OPTS = dict(num_refine=4, ambient=0.25, albedo=(0.9, 0.6, 0.7), background=(1.0, 0.5, -1.0))


def assert_unjittered_depths(t, S, cfg):
    """The coarse depths are the stratified sampler's at u = 0.5 over cfg.ray_start .. cfg.ray_end, the same on every ray.  In float64, with
    lin(q) = q / (S-1): the classical marcher draws sample k between the mid-points of its neighbours (the end bins stop at 0 and 1), the mip
    marcher at lin(k) + u / (S-1); the kernel's fp32 chain is within a few ulp of that (depths are ~1: 1e-6)."""
    assert t.shape[1] == S and np.array_equal(t, np.broadcast_to(t[:1], t.shape))
    lin = np.arange(S, dtype=np.float64) / (S - 1)
    if cfg.ray_marcher_type == 'classical':
        mid = 0.5 * (lin[1:] + lin[:-1])
        lower, upper = np.concatenate([[lin[0]], mid]), np.concatenate([mid, [lin[-1]]])
        s = lower + (upper - lower) * 0.5
    else:
        s = lin + 0.5 / (S - 1)
    want = cfg.ray_start + (cfg.ray_end - cfg.ray_start) * s
    assert np.abs(t[0].astype(np.float64) - want).max() <= 1e-6, (t[0], want)
    assert np.all(np.diff(t[0]) > 0)


def build_scene(tdgp, n_layers):
    """config_tiny (16 x 16 rays, 8 coarse steps), seeded weights, 2 samples x 3 cameras; the level is the median over rays of the largest coarse
    density, and the yardstick is the restated chain fed with the product's own field values, computed once and left unchanged."""
    Sh = tdgp.shapes
    cfg = tdgp.config.config_tiny()
    cfg.mlp_n_layers = n_layers
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=31 + n_layers, exercise_all=True))
    G = G.to(DEV).eval()
    inp = tdgp.weights.synthetic_inputs(cfg, batch=B, seed=12)
    ws = G.mapping(T(inp['z']), T(inp['c']))
    cam_np = tdgp.weights.synthetic_inputs(cfg, batch=B * V, seed=13)['camera']
    cams = tdgp.generator.TensorGroup(**{k: T(v) for k, v in cam_np.items()})
    syn = G.synthesis
    planes = syn.tri_planes(ws, noise_mode='const')
    res = syn.test_resolution
    R, S, N = res * res, cfg.num_ray_steps, OPTS['num_refine']
    ray_o, ray_d = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cams), fov=cams.fov, resolution=(res, res), device=DEV)
    ray_o, ray_d = ray_o.reshape(B, V * R, 3), ray_d.reshape(B, V * R, 3)
    ray_field, point_field = Sh.field_functions(syn)
    rays = B * V * R
    t = Sh.coarse_depths(syn, rays, S, DEV)
    assert_unjittered_depths(H(t), S, cfg)
    per_ray = lambda x: H(x).reshape(rays, -1, 4)                                                     # noqa: E731
    on_rays = lambda tt: per_ray(ray_field(planes, ray_o, ray_d, T(tt).reshape(B, V * R, -1), res))   # noqa: E731
    at_points = lambda p: per_ray(point_field(planes, T(p).reshape(B, V * R * 7, 3)))                 # noqa: E731
    level = float(np.median(on_rays(H(t))[..., 3].max(axis=1)))
    step = 2.0 * cfg.cube_scale / cfg.tri_plane_res
    o_np, d_np = H(ray_o).reshape(rays, 3), H(ray_d).reshape(rays, 3)
    want = {mode: SR.chain(on_rays, at_points, H(t), o_np, d_np, N, level, step, cfg.ray_end, mode=mode,
                           **{k: OPTS[k] for k in ('ambient', 'albedo', 'background')}) for mode in ('shaded', 'normals', 'colour')}
    return dict(G=G, ws=ws, cams=cams, planes=planes, level=level, R=R, res=res, want=want, o=o_np, d=d_np)


@pytest.fixture(scope='module')
def scene2(tdgp):
    return build_scene(tdgp, 2)


@pytest.fixture(scope='module')
def scene3(tdgp):
    return build_scene(tdgp, 3)


def check_views(tdgp, sc, what, single_rays=False):
    Sh = tdgp.shapes
    R = sc['R']
    hit_share = float((sc['want']['shaded']['status'] != 0).mean())
    assert 0.2 <= hit_share <= 0.8, f'{what}: {hit_share:.3f} of the rays hit at level {sc["level"]}'
    assert (sc['want']['shaded']['status'] == 1).sum() > 50
    base = None
    for mode in ('shaded', 'normals', 'colour'):
        w = sc['want'][mode]
        # unlimited; one image; a third of an image (whole rows); 11 rays per call: runs that are no whole rows (ray_w = 0) with a ragged last
        # one; and, once, one ray per call: fewer rays than samples, so the samples are taken one at a time
        for chunk in (None, R, R // 3, 11) + ((1,) if single_rays and mode == 'shaded' else ()):
            out = Sh.render_shape_views(sc['G'], sc['planes'], sc['cams'], level=sc['level'], mode=mode, max_rays_per_call=chunk, **OPTS)
            assert out.rgb.shape == (B * V, R, 3) and out.depth.shape == (B * V, R, 1) and out.normal.shape == (B * V, R, 3) and out.status.shape == (B * V, R)
            tag = f'{what} {mode} chunk={chunk}'
            same_bytes(H(out.status).reshape(-1), w['status'], 'status ' + tag)
            same_bytes(H(out.depth).reshape(-1), w['depth'], 'depth ' + tag)
            same_bytes(H(out.normal).reshape(-1, 3), w['normal'], 'normal ' + tag)
            same_bytes(H(out.rgb).reshape(-1, 3), w['rgb'], 'rgb ' + tag)
            if mode == 'shaded' and chunk is None:
                base = out
    return base


def test_views_equal_the_restated_chain_two_layers(tdgp, scene2):
    check_views(tdgp, scene2, 'two-layer decoder', single_rays=True)


def test_views_equal_the_restated_chain_three_layers(tdgp, scene3):
    assert tdgp.renderer.deep_form(scene3['G'].synthesis.tri_plane_mlp)
    check_views(tdgp, scene3, 'three-layer decoder')


def test_render_shapes_images_and_grids(tdgp, scene2):
    """render_shapes == rays_to_image of the ray-major frames (one sample per plane batch and all at once); the video grid and the strips ==
    frames_to_grid of the same frames, colours and normalised depths."""
    Sh, I = tdgp.shapes, tdgp.inference
    sc = scene2
    G, res, R = sc['G'], sc['res'], sc['R']
    w = sc['want']['shaded']
    kw = dict(level=sc['level'], mode='shaded', **OPTS)
    for plane_batch in (1, 4):
        out = Sh.render_shapes(G, sc['ws'], sc['cams'], plane_batch=plane_batch, return_all=True, **kw)
        same_bytes(H(out.img), w['rgb'].reshape(B * V, res, res, 3).transpose(0, 3, 1, 2), f'img plane_batch={plane_batch}')
        same_bytes(H(out.normal), w['normal'].reshape(B * V, res, res, 3).transpose(0, 3, 1, 2), 'normal image')
        same_bytes(H(out.depth), w['depth'].reshape(B * V, 1, res, res), 'depth image')
        same_bytes(H(out.status), w['status'].reshape(B * V, res, res), 'status image')
    img = Sh.render_shapes(G, sc['ws'], sc['cams'], **kw)
    assert torch.equal(img, out.img)
    rgb, depth = T(w['rgb'].reshape(B * V, R, 3)), T(w['depth'].reshape(B * V, R, 1))
    norm = I._depth_normalisation(G)
    assert torch.equal(Sh.render_shape_video_grid(G, sc['ws'], sc['cams'], **kw),
                       I.frames_to_grid(rgb, res, res, tiles=B, images=V, stride_image=1, stride_tile=V, nrow=2))
    assert torch.equal(Sh.render_shape_video_grid(G, sc['ws'], sc['cams'], show='depth', nrow=1, plane_batch=1, **kw),
                       I.frames_to_grid(depth, res, res, tiles=B, images=V, stride_image=1, stride_tile=V, nrow=1, normalise=norm))
    assert torch.equal(Sh.render_shape_strips(G, sc['ws'], sc['cams'], **kw),
                       I.frames_to_grid(rgb, res, res, tiles=V, images=B, stride_image=V, stride_tile=1, nrow=V, padding=0))
    strips = Sh.render_shape_strips(G, sc['ws'], sc['cams'], show='depth', as_numpy=True, **kw)
    assert isinstance(strips, np.ndarray) and strips.dtype == np.uint8 and strips.shape == (B, res, V * res, 3)
    assert np.array_equal(strips, H(I.frames_to_grid(depth, res, res, tiles=V, images=B, stride_image=V, stride_tile=1, nrow=V, padding=0, normalise=norm)))


def test_hits_agree_with_the_density_grid(tdgp, scene2):
    """The mesh route's grid at volume_res = 64 over the tri-plane box, interpolated trilinearly at every status-1 hit point, is within the
    grid's own discretisation of the level: the largest difference between adjacent grid values of the cell the point lies in (computed from
    the grid; nothing is chosen in advance).  density_grid's lattice is the reference's sheared one, point (i, j, k) at
    ((i + j / res + k / res^2), (j + k / res), k) * voxel + origin, so the cell coordinates come from inverting that map."""
    sc = scene2
    G = sc['G']
    res, box = 64, 2.0 * G.cfg.cube_scale
    w = sc['want']['shaded']
    hit = w['status'] == 1
    p = w['points'][hit, 0, :].astype(np.float64)
    sample = np.repeat(np.arange(B), V * sc['R'])[hit]
    grid = H(tdgp.geometry.density_grid(G, sc['ws'], volume_res=res, cube_size=box)).astype(np.float64)
    voxel, origin = box / (res - 1), -box / 2
    k = (p[:, 2] - origin) / voxel
    j = (p[:, 1] - origin) / voxel - k / res
    i = (p[:, 0] - origin) / voxel - j / res - k / res ** 2
    u = np.stack([i, j, k], axis=1)
    inside = ((u >= 0) & (u <= res - 1)).all(axis=1)
    # the lattice is sheared by up to one cell (i by j / res, j by k / res), so it misses a strip of the box at the low x and low y rims: a hit
    # can fall outside the lattice only there (unsheared cell index below 1 + 1 / res), or outside the box itself
    cell = (p - origin) / voxel
    rim = (cell[:, :2].min(axis=1) < 1 + 1.0 / res) | (cell.min(axis=1) < 0) | (cell.max(axis=1) > res - 1)
    assert np.all(inside | rim), f'{int((~inside & ~rim).sum())} hits inside the lattice were left out'
    print(f'status-1 hits {len(u)}, outside the sheared lattice (not compared) {int((~inside).sum())}')
    u, sample = u[inside], sample[inside]
    c = np.minimum(np.floor(u).astype(np.int64), res - 2)
    f = u - c
    corner = np.empty([len(u), 2, 2, 2])
    for a in (0, 1):
        for b in (0, 1):
            for e in (0, 1):
                corner[:, a, b, e] = grid[sample, c[:, 0] + a, c[:, 1] + b, c[:, 2] + e]
    wts = np.stack([1 - f, f], axis=-1)                              # [n, axis, 2]
    interp = np.einsum('nabe,na,nb,ne->n', corner, wts[:, 0], wts[:, 1], wts[:, 2])
    bound = np.max([np.abs(np.diff(corner, axis=ax)).max(axis=(1, 2, 3)) for ax in (1, 2, 3)], axis=0)
    err = np.abs(interp - sc['level'])
    print(f'hits {len(u)}, |interp - level| max {err.max():.4g}, median {np.median(err):.4g}; bound min {bound.min():.4g}, median {np.median(bound):.4g}; '
          f'worst err / bound {np.max(err / np.maximum(bound, 1e-30)):.4g}')
    assert len(u) > 50 and np.all(err <= bound), f'{int((err > bound).sum())} of {len(u)} hits beyond the cell bound, worst ratio {np.max(err / bound):.3f}'


def test_cli_writes_a_shape_grid(tdgp, tmp_path, capsys):
    """tools/render_trajectory.py --vis shape_grid / shape_strips on a directory laid out as tools/export_reference_checkpoint.py writes it, run in
    this process: the file exists, one JSON line describes it, and the block equals `render_shape_video_grid` called with the same seeds."""
    import importlib.util
    import json
    import os
    spec = importlib.util.spec_from_file_location('render_trajectory_cli', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools',
                                                                                       'render_trajectory.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = tdgp.config.config_tiny()
    sd = tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True)
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **sd)
    common = ['--ckpt', str(tmp_path), '--seeds', '0-3', '--trajectory', 'front_circle', '--num-frames', '8', '--level', '0.0', '--num-refine', '4', '--seed', '5']
    out = str(tmp_path / 'shapes.npy')
    cli.main(common + ['--vis', 'shape_grid', '--out', out])
    cli.main(common + ['--vis', 'shape_grid', '--out', str(tmp_path / 'shapes.gif')])
    cli.main(common + ['--vis', 'shape_strips', '--shape-mode', 'normals', '--depth', '--out', str(tmp_path / 'strips.png')])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 3 and os.path.getsize(tmp_path / 'shapes.gif') > 0 and os.path.getsize(tmp_path / 'strips.png') > 0
    res = cfg.img_resolution
    assert lines[0]['vis'] == 'shape_grid' and lines[0]['shape'] == [8, 2 * (res + 2) + 2, 2 * (res + 2) + 2, 3] and lines[0]['level'] == 0.0
    assert lines[0]['samples'] == 4 and lines[0]['frames'] == 8 and lines[0]['shape_mode'] == 'shaded' and lines[0]['num_refine'] == 4
    assert lines[2]['vis'] == 'shape_strips' and lines[2]['shape'] == [1, 4 * res, 8 * res, 3] and lines[2]['depth'] is True
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(sd)
    G = G.to(DEV).eval()
    torch.manual_seed(5)
    np.random.seed(5)
    with torch.no_grad():
        ws, z, c = tdgp.inference.sample_ws_from_seeds(G, [0, 1, 2, 3], device='cuda')
        cams = tdgp.inference.generate_camera_params(G, z, c, dict(name='front_circle', num_frames=8, use_mean_camera=True, fov_offset=0.0, yaw_diff=0.5,
                                                                   pitch_diff=0.3, fov_diff=1.0))
        want = tdgp.shapes.render_shape_video_grid(G, ws, cams, level=0.0, num_refine=4, as_numpy=True)
    got = np.load(out)
    assert got.dtype == np.uint8 and np.array_equal(got, want)

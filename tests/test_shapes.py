"""Shape frames, the parts that need no GPU: the numpy restatement of the iso-surface contracts (tests/shapes_reference.py) against an analytic
sphere -- before the GPU tests trust it --, the Python layer's refusals before any device call, the CLI's new arguments, and the three new
entry points in header, binding and library."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import shapes_reference as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ('tdgp_iso_bracket', 'tdgp_iso_locate', 'tdgp_iso_shade')


def _cli():
    spec = importlib.util.spec_from_file_location('render_trajectory_cli', os.path.join(REPO, 'tools', 'render_trajectory.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _G(tdgp):
    return tdgp.generator.Generator(tdgp.config.config_tiny())


def _cams(tdgp, n):
    return tdgp.generator.TensorGroup(angles=torch.zeros(n, 3), fov=torch.full([n], 20.0), radius=torch.ones(n), look_at=torch.zeros(n, 3))


# ------------------------------------------------------------------------------------------------ the restatement against an analytic sphere
SPHERE = dict(radius=0.3, gain=200.0, res=32, fov=40.0, near=0.5, far=1.5, S=64, N=16, level=0.0)


def _sphere_chain(mode='shaded'):
    p = SPHERE
    o, d = SR.pinhole_rays(p['res'], p['fov'])
    rays = len(o)

    def sigma_at(x):                                       # sigma(x) = 200 * (0.3 - |x|), evaluated in float64 and rounded once
        x = np.asarray(x, np.float64)
        out = np.zeros(x.shape[:-1] + (4,), np.float32)
        out[..., 3] = p['gain'] * (p['radius'] - np.linalg.norm(x, axis=-1))
        return out

    ray_field = lambda t: sigma_at(o[:, None, :].astype(np.float64) + np.asarray(t, np.float64)[..., None] * d[:, None, :].astype(np.float64))   # noqa: E731
    k = (np.arange(p['S'], dtype=np.float64) + 0.5) / p['S']
    t = np.broadcast_to((p['near'] + (p['far'] - p['near']) * k).astype(np.float32), (rays, p['S']))
    h = 1.0 / 64
    out = SR.chain(ray_field, sigma_at, t, o, d, p['N'], p['level'], h, p['far'], mode=mode)
    return o, d, out


def test_restatement_finds_the_analytic_sphere():
    """Status equals the analytic hit mask and |t_hit - t_analytic| <= (far - near) / (S * N), the bracket width, on every ray whose chord inside
    the sphere is at least two coarse steps long; the grazing rays left out are at most 10 %, and the field of view keeps the sphere's
    silhouette inside the frame with both hits and misses well represented."""
    p = SPHERE
    o, d, out = _sphere_chain()
    hit, t_true, chord = SR.ray_sphere(o, d, p['radius'])
    coarse = (p['far'] - p['near']) / p['S']
    graze = hit & (chord < 2 * coarse)
    keep = ~graze
    assert graze.mean() <= 0.10, f'{graze.mean():.3f} of the rays graze the sphere'
    assert 0.2 <= hit.mean() <= 0.8, hit.mean()                        # the field of view: neither an empty nor a full frame
    edge = np.abs(np.arange(len(o)) % p['res'] - (p['res'] - 1) / 2) == (p['res'] - 1) / 2
    assert not hit[edge].any()                                         # the silhouette stays inside the frame
    assert np.array_equal(out['status'][keep] == SR.STATUS_HIT, hit[keep]) and not (out['status'] == SR.STATUS_NEAR).any()
    err = np.abs(out['depth'].astype(np.float64) - t_true)[keep & hit]
    assert err.size > 200 and err.max() <= (p['far'] - p['near']) / (p['S'] * p['N']), err.max()
    assert np.all(out['depth'][out['status'] == SR.STATUS_MISS] == np.float32(p['far']))


def test_restatement_shades_the_analytic_sphere():
    """The sphere's normal is x / |x|: the central-difference normal of the restatement agrees to the stencil's second-order error, hits are lit by
    the headlight (n . l > 0, so v > ambient), misses carry the background and a zero normal."""
    p = SPHERE
    o, d, out = _sphere_chain(mode='normals')
    hit = out['status'] == SR.STATUS_HIT
    x = out['points'][:, 0, :].astype(np.float64)
    n_true = x / np.linalg.norm(x, axis=-1, keepdims=True)
    # |x| has second derivatives <= 1 / |x| ~ 3.4 and third ones <= 3 / |x|^2: the central difference is off by <= h^2 / 6 * 3 / |x|^2 per axis
    h = 1.0 / 64
    bound = 3 * (h * h / 6 * 3 / 0.29 ** 2) + 1e-5
    assert np.abs(out['normal'][hit] - n_true[hit]).max() <= bound
    assert np.array_equal(out['rgb'][hit], out['normal'][hit])
    assert np.all(out['normal'][~hit] == 0) and np.all(out['rgb'][~hit] == 1)
    _, _, shaded = _sphere_chain(mode='shaded')
    v = (shaded['rgb'][hit, 0].astype(np.float64) + 1) / 2 / 0.8
    assert v.min() > 0.2 and v.max() <= 1.0 + 1e-6


def test_restatement_edge_rows():
    """The cases the contract spells out, on hand-written rows."""
    t = np.array([[1, 2, 3, 4]] * 6, np.float32)
    nan, inf = np.nan, np.inf
    sigma = np.array([[0, 0, 0, 0], [5, 0, 0, 0], [0, 0, 0, 5], [0, nan, 5, 9], [0, 1, inf, 0], [-inf, 1, 1, 7]], np.float32)
    idx, fine = SR.bracket(sigma, t, 4, 1.0)
    assert idx.tolist() == [4, 0, 3, 2, 1, 1]                          # none; k = 0; k = S-1; NaN is not a crossing; a value equal to the level is
    assert fine[0].tolist() == [4, 4, 4, 4] and fine[1].tolist() == [1, 1, 1, 1] and fine[2].tolist() == [3.25, 3.5, 3.75, 4]
    sig_f = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 2, 9, 9], [nan, nan, nan, 5], [1, 1, 1, 1], [0.5, 0.5, 0.5, 0.5]], np.float32)
    o, d = np.zeros([6, 3], np.float32), np.tile(np.array([[0, 0, 1]], np.float32), (6, 1))
    th, st, pts = SR.locate(sigma, t, idx, sig_f, fine, o, d, 1.0, 0.5, 99.0)
    assert st.tolist() == [0, 2, 1, 1, 1, 1]
    assert th[0] == 99 and th[1] == 1 and th[2] == np.float32(3.25) + np.float32(0.25) * np.float32(0.5)
    assert th[3] == fine[3, 3]                                         # NaN on the low side: a = 1, the high side
    assert th[4] == np.float32(1.0) + (fine[4, 0] - np.float32(1.0)) * np.float32(1.0)          # j == 0: the low side is the coarse sample idx-1
    assert th[5] == fine[5, 3]                                         # no fine sample reaches the level and the last pair is flat: a = 1
    assert pts.shape == (6, 7, 3) and pts[2, 5, 2] == th[2] + np.float32(0.5) and pts[2, 6, 2] == th[2] - np.float32(0.5) and pts[2, 1, 0] == 0.5


# ------------------------------------------------------------------------------------------------ refusals of the Python layer, before any device call
def test_render_shape_views_refusals(tdgp):
    S = tdgp.shapes
    G = _G(tdgp).eval()
    res = G.cfg.tri_plane_res
    planes = tdgp.renderer.HWCPlanes(torch.zeros(2, 3, res, res, G.cfg.feat_dim))
    with pytest.raises(ValueError, match='mode must be one of'):
        S.render_shape_views(G, planes, _cams(tdgp, 4), mode='wireframe')
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match=r'num_refine must be an integer in 1\.\.64'):
            S.render_shape_views(G, planes, _cams(tdgp, 4), num_refine=bad)
    for bad in (1, 513):
        with pytest.raises(ValueError, match=r'num_steps must be an integer in 2\.\.512'):
            S.render_shape_views(G, planes, _cams(tdgp, 4), num_steps=bad)
    with pytest.raises(ValueError, match='not a multiple of the plane batch'):
        S.render_shape_views(G, planes, _cams(tdgp, 3))
    with pytest.raises(TypeError, match='HWCPlanes'):
        S.render_shape_views(G, planes.t, _cams(tdgp, 4))
    with pytest.raises(ValueError, match='max_rays_per_call must be positive'):
        S.render_shape_views(G, planes, _cams(tdgp, 4), max_rays_per_call=0)
    with pytest.raises(RuntimeError, match='GPU'):                       # everything above was refused before this: the kernels have no CPU path
        S.render_shape_views(G, planes, _cams(tdgp, 4))
    G.train()
    with pytest.raises(RuntimeError, match=r'inference route: call \.eval\(\) first'):
        S.render_shape_views(G, planes, _cams(tdgp, 4))


def test_render_shapes_refusals(tdgp):
    S = tdgp.shapes
    G = _G(tdgp).eval()
    ws = torch.zeros(2, G.num_ws, G.w_dim)
    for fn in (S.render_shapes, S.render_shape_video_grid, S.render_shape_strips):
        with pytest.raises(ValueError, match='cameras are not a multiple of the 2 samples'):
            fn(G, ws, _cams(tdgp, 3))
        with pytest.raises(ValueError, match='mode must be one of'):
            fn(G, ws, _cams(tdgp, 4), mode='x')
        with pytest.raises(ValueError, match='num_refine'):
            fn(G, ws, _cams(tdgp, 4), num_refine=0)
    for fn in (S.render_shape_video_grid, S.render_shape_strips):
        with pytest.raises(ValueError, match="show must be 'rgb' or 'depth'"):
            fn(G, ws, _cams(tdgp, 4), show='normal')
    G.train()
    with pytest.raises(RuntimeError, match=r'call \.eval\(\) first'):
        S.render_shapes(G, ws, _cams(tdgp, 4))
    with pytest.raises(ValueError, match='mode must be one of'):
        S.iso_shade(torch.zeros(1, 7, 4), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3), mode='x')
    with pytest.raises(RuntimeError, match='GPU'):
        S.iso_bracket(torch.zeros(3, 4), torch.zeros(3, 4), 2, 0.0)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_shape_arguments():
    cli = _cli()
    p = cli.build_parser()
    a = p.parse_args(['--ckpt', 'd', '--out', 'o.gif', '--vis', 'shape_grid'])
    assert a.vis == 'shape_grid' and a.level == 25.0 and a.shape_mode == 'shaded' and a.num_refine == 16 and a.ambient == 0.2 and a.background == 1.0
    a = p.parse_args(['--ckpt', 'd', '--out', 'o.png', '--vis', 'shape_strips', '--level', '-3.5', '--shape-mode', 'normals', '--num-refine', '8',
                      '--ambient', '0.4', '--background', '0'])
    assert (a.vis, a.level, a.shape_mode, a.num_refine, a.ambient, a.background) == ('shape_strips', -3.5, 'normals', 8, 0.4, 0.0)
    assert cli.shape_options(a) == dict(level=-3.5, mode='normals', num_refine=8, ambient=0.4, background=(0.0, 0.0, 0.0))
    a = p.parse_args(['--ckpt', 'd', '--out', 'o.gif'])                  # the existing choices and defaults are untouched
    assert a.vis == 'video_grid' and not a.depth
    assert p.parse_args(['--ckpt', 'd', '--out', 'o.png', '--vis', 'image_grid']).vis == 'image_grid'
    for bad in (['--vis', 'shape'], ['--shape-mode', 'wire']):
        with pytest.raises(SystemExit):
            p.parse_args(['--ckpt', 'd', '--out', 'o.gif'] + bad)


# ------------------------------------------------------------------------------------------------ ABI
def test_entry_points_in_header_binding_and_library(tdgp):
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib_path = tdgp._lib.LIB_PATH
    exported = subprocess.run(['nm', '-D', '--defined-only', lib_path], capture_output=True, text=True).stdout
    lib = tdgp._lib.load()
    for name in NAMES:
        assert re.search(rf'\bint\s+{name}\s*\(', code), f'{name} is not declared in include/tdgp.h'
        assert name in tdgp._lib.EXPORTS and hasattr(lib, name)
        assert re.search(rf' T {name}\b', exported), f'{name} is not exported by the library'
    assert 'iso_surface.hip' in tdgp.build.SOURCES

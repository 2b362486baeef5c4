"""Multisampled mesh frames without a GPU: the properties of the numpy restatement (tests/mesh_msaa_reference.py) that make it worth being the
yardstick of the device tests -- the sample patterns are the constants of the contract, more samples estimate the covered area of a pixel
better, triangles that share edges cover every sample exactly once -- and the host side of the feature: the `samples` option of the drivers
and `--mesh-samples` of the command line."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_msaa_reference as R
import mesh_raster_reference as MR

F = np.float32
D = np.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('tdgp_mesh_visibility_ms', 'tdgp_mesh_resolve_ms')
# the issue's triangle, snapped vertices in 1/256 pixel, on a 16 x 16 frame
TRI_X, TRI_Y = (808, 3528, 1613), (522, 1410, 3427)


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_ms_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ patterns
def test_patterns_are_the_constants_of_the_contract(tdgp):
    four = ((-32, -96), (96, -32), (-96, 32), (32, 96))
    sixteen = tuple((ox, oy) for oy in (-96, -32, 32, 96) for ox in (-96, -32, 32, 96))
    assert R.PATTERNS == {4: four, 16: sixteen}
    assert tdgp.mesh.SAMPLE_PATTERNS == {4: four, 16: sixteen} and tdgp.mesh.SAMPLES == (1, 4, 16)
    assert sixteen[0] == (-96, -96) and sixteen[1] == (-32, -96) and sixteen[4] == (-96, -32) and sixteen[15] == (96, 96)      # row-major, oy outer
    for S, p in R.PATTERNS.items():
        p = np.array(p)
        assert len(p) == S and len({tuple(q) for q in p}) == S and np.abs(p).max() == R.PAD == 96
        assert p.sum(axis=0).tolist() == [0, 0]                                      # centred on the pixel centre
        assert len(set(p[:, 0])) == 4 and len(set(p[:, 1])) == 4                     # every column and row of the 4 x 4 sub-grid is used
    # the rotated grid: one sample in every row and column of the sub-grid
    assert sorted(q[0] for q in four) == [-96, -32, 32, 96] and [q[1] for q in four] == [-96, -32, 32, 96]
    # the entry points stand in the header, the export table and the source
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    source = open(os.path.join(REPO, '3dgp_amd', 'csrc', 'mesh_raster.hip')).read()
    for name in NEW:
        assert name in header and name in tdgp._lib.EXPORTS and name in source
    # the per-hit bodies are one text: the one-sample kernels and the fused resolve call the same functions
    texture, surface = (open(os.path.join(REPO, '3dgp_amd', 'csrc', f)).read() for f in ('mesh_texture.hip', 'mesh_surface.hip'))
    assert 'mesh_hit.h' in tdgp.build.HEADERS
    for fn, files in (('mesh_face_normal', (source,)), ('mesh_vertex_colour', (source,)), ('mesh_vertex_normal', (source, surface)),
                      ('mesh_texture_fetch', (source, texture)), ('mesh_bary_weights', (source, surface, texture))):
        for text in files:
            assert fn + '(' in text, fn
    assert source.count('mesh_face_normal(') == 2 and source.count('mesh_vertex_colour(') == 2             # mesh_resolve_kernel and mesh_resolve_ms_kernel


# ------------------------------------------------------------------------------------------------ coverage
def test_more_samples_estimate_the_area_better():
    """The triangle of the issue: the exact area of every pixel's unit square inside it, by clipping in float64, against hits / S.
    Mean absolute error per touched pixel: 0.0941 at the pixel centre alone, 0.0381 at four samples, 0.0101 at sixteen."""
    exact = R.exact_coverage(TRI_X, TRI_Y, 16, 16)
    area2 = abs((TRI_X[1] - TRI_X[0]) * (TRI_Y[2] - TRI_Y[0]) - (TRI_Y[1] - TRI_Y[0]) * (TRI_X[2] - TRI_X[0]))
    assert abs(exact.sum() - area2 / 2.0 / 65536.0) < 1e-9                           # the triangle lies inside the frame: the pieces add up to it
    assert exact.min() >= 0.0 and exact.max() <= 1.0 + 1e-12 and (exact == 0).any() and (exact > 1.0 - 1e-12).any()
    e1, e4, e16 = (R.coverage_error(TRI_X, TRI_Y, 16, 16, S) for S in (1, 4, 16))
    print(f'coverage error per touched pixel: e1 = {e1:.4f}, e4 = {e4:.4f}, e16 = {e16:.4f}')
    assert e16 < e4 < e1
    # a pixel no sample of which is covered has no area to speak of, and a fully covered one has every sample
    for S in (4, 16):
        hits = R.hit_counts(TRI_X, TRI_Y, 16, 16, S)
        assert (hits[exact == 0] == 0).all() and (hits[exact > 1.0 - 1e-12] == S).all() and 0 < hits.sum() < 256 * S
    # S = 1 is the one-sample rasteriser's coverage
    one = R.hit_counts(TRI_X, TRI_Y, 16, 16, 1)
    inside, _, _, _ = R.cover(TRI_X, TRI_Y, 0, 15, 0, 15, 1)
    assert np.array_equal(one, inside[:, :, 0].astype(np.int64)) and one.max() == 1


def _partition(tris, h, w):
    """tris: [(X, Y)] in 1/256 pixel -> for both patterns, (the per-pixel hit counts added over the triangles, the samples covered more than once)."""
    out = {}
    for S in (4, 16):
        total, twice = np.zeros((h, w), np.int64), 0
        seen = np.zeros((h, w, S), np.int64)
        for X, Y in tris:
            total += R.hit_counts(X, Y, h, w, S)
            seen += R.cover(X, Y, 0, w - 1, 0, h - 1, S)[0]
        twice = int((seen > 1).sum())
        assert np.array_equal(seen.sum(axis=2), total)                               # the padded box loses no sample
        out[S] = (total, twice)
    return out


def test_partition_two_triangles_sharing_an_edge():
    """A quad split along a diagonal that passes through sample positions: every sample of the quad belongs to exactly one half."""
    # corners on sample positions of both patterns (multiples of 32 that are odd multiples of 32 from the centres), the diagonal through many
    A, B, Cc, Dd = (2 * 256 - 96, 1 * 256 - 96), (9 * 256 + 96, 1 * 256 - 96), (9 * 256 + 96, 8 * 256 + 96), (2 * 256 - 96, 8 * 256 + 96)
    halves = [((A[0], B[0], Cc[0]), (A[1], B[1], Cc[1])), ((A[0], Cc[0], Dd[0]), (A[1], Cc[1], Dd[1]))]
    for h2 in (halves, [(X[::-1], Y[::-1]) for X, Y in halves]):                     # either winding
        for S, (total, twice) in _partition(h2, 12, 12).items():
            assert twice == 0
            # the union: an axis-aligned rectangle [x0, x1) x [y0, y1) under the top-left rule, counted directly
            ox, oy = R.offsets(S)
            sx = (np.arange(12) << 8)[None, :, None] + ox[None, None, :]
            sy = (np.arange(12) << 8)[:, None, None] + oy[None, None, :]
            want = ((sx >= A[0]) & (sx < B[0]) & (sy >= A[1]) & (sy < Cc[1])).sum(axis=2)
            assert np.array_equal(total, want), S
            assert total.max() == S and (total == S).sum() >= 36


def test_partition_fan_around_a_vertex():
    """Seven triangles around a vertex that is itself a sample position: the fan covers what its outline covers, every sample once."""
    centre = (6 * 256 + 32, 6 * 256 - 32)
    rim = [(11 * 256 + 17, 6 * 256 + 5), (9 * 256 + 96, 10 * 256 - 96), (5 * 256 - 3, 11 * 256 + 64), (1 * 256 + 32, 8 * 256 + 32), (1 * 256 - 96, 3 * 256 + 1),
           (5 * 256 + 96, 1 * 256 - 32), (10 * 256 - 32, 2 * 256 + 96)]
    fan = [((centre[0], rim[i][0], rim[(i + 1) % 7][0]), (centre[1], rim[i][1], rim[(i + 1) % 7][1])) for i in range(7)]
    for S, (total, twice) in _partition(fan, 13, 13).items():
        assert twice == 0 and total.max() == S
        # the outline is convex: a sample strictly inside it is covered exactly once, so the fan has no cracks along its spokes
        ox, oy = R.offsets(S)
        sx = (np.arange(13) << 8)[None, :, None] + ox[None, None, :]
        sy = (np.arange(13) << 8)[:, None, None] + oy[None, None, :]
        strictly = np.ones((13, 13, S), bool)
        for i in range(7):
            (x0, y0), (x1, y1) = rim[i], rim[(i + 1) % 7]
            strictly &= (x1 - x0) * (sy - y0) - (y1 - y0) * (sx - x0) > 0
        assert strictly.sum() > 20 * S
        seen = sum(R.cover(X, Y, 0, 12, 0, 12, S)[0].astype(np.int64) for X, Y in fan)
        assert (seen[strictly] == 1).all()
        if S == 16:                                                                  # the hub itself is sample (32, -32) of pixel (6, 6): one spoke's triangle owns it
            assert R.PATTERNS[16][6] == (32, -32) and strictly[6, 6, 6] and seen[6, 6, 6] == 1


def test_restatement_end_to_end_on_the_host():
    """visibility_ms -> resolve_ms on an icosphere: coverage is hits / S, interior pixels equal the one-sample frame's status, rgb of a fully
    missed pixel is the background, and one sample per pixel through the same functions would see the one-sample keys' triangles."""
    v, t = MR.icosphere(1, 0.3)
    c2w, focal = MR.pinhole_camera(50.0)
    bg = (1.0, 0.5, -1.0)
    for S in (4, 16):
        out = R.frames_ms(v, t, c2w, focal, 12, 12, S, 0.1, 'back', 2.5, ambient=0.25, background=bg)
        cov, st = out['coverage'], out['status']
        assert cov.dtype == F and set(np.unique(cov * S)) <= set(range(S + 1)) and 0 < (cov == 1).sum() and 0 < (cov == 0).sum() and ((cov > 0) & (cov < 1)).any()
        assert np.array_equal(st, (cov > 0).astype(np.int32)) and np.array_equal(out['tri'] >= 0, st == 1)
        assert (out['rgb'][cov == 0] == np.asarray(bg, F)).all() and (out['depth'][cov == 0] == F(2.5)).all()
        hit = st == 1
        assert np.all(np.abs(np.linalg.norm(out['normal'][hit].astype(D), axis=1) - 1) < 1e-6) and np.all(out['normal'][~hit] == 0)
        # the depth of a pixel is the smallest of its samples' depths
        th = (out['vis'].reshape(-1, S) >> np.uint64(32)).astype(np.uint32).view(F)
        th = np.where(out['sample_status'], th, np.inf)
        assert np.array_equal(out['depth'][hit], th.min(axis=1)[hit])


# ------------------------------------------------------------------------------------------------ options
def test_samples_option_errors(tdgp):
    M = tdgp.mesh
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    cams = dict(angles=torch.zeros(1, 3), radius=torch.ones(1), look_at=torch.zeros(1, 3), fov=torch.full((1,), 40.0))
    for s in (0, 2, 3, 8, 32, -4, True, None, '4'):
        with pytest.raises(ValueError, match='samples'):
            M.render_mesh_views(v, t, cams, 8, samples=s)
    with pytest.raises(ValueError, match='samples'):
        M.render_mesh_views(v, t, cams, 8, samples=4, normals='field', planes=object(), G=object())
    with pytest.raises(ValueError, match='samples'):
        M.render_mesh_views(v, t, cams, 8, samples=16, normals='field', planes=object(), G=object())
    for s in (1, 4, 16):                                                            # well-formed, on the host: the kernels have no CPU path
        with pytest.raises(RuntimeError, match='GPU'):
            M.render_mesh_views(v, t, cams, 8, samples=s)
    for s in (0, 1, 2, 8):
        with pytest.raises(ValueError, match='samples'):
            M.mesh_visibility_ms(v, t, torch.zeros(1, 4, 4), torch.ones(1), 8, s)
    with pytest.raises(ValueError, match='cull'):
        M.mesh_visibility_ms(v, t, torch.zeros(1, 4, 4), torch.ones(1), 8, 4, cull='both')
    with pytest.raises(ValueError, match='mode'):
        M.mesh_resolve_ms(torch.zeros(1, 64, 4, dtype=torch.int64), v, t, torch.zeros(1, 4, 4), torch.ones(1), 8, 0.0, mode='wire')
    with pytest.raises(RuntimeError, match='GPU'):
        M.mesh_visibility_ms(v, t, torch.zeros(1, 4, 4), torch.ones(1), 8, 4)
    # the frame drivers refuse a bad value before any work
    class _G:                                                                        # noqa: E306
        synthesis, cfg = None, None
    for kw in (dict(samples=2), dict(samples=4, normals='field')):
        with pytest.raises(ValueError, match='samples'):
            M.render_mesh_frames(_G(), [0], cams, **kw)


def test_mesh_samples_on_the_command_line(capsys):
    rt = _tool('render_trajectory')
    p = rt.build_parser()
    base = ['--ckpt', 'x', '--out', 'y.npy']
    assert 'samples' not in rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_grid']))
    assert 'samples' not in rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_grid', '--mesh-samples', '1']))
    assert rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_grid', '--mesh-samples', '4']))['samples'] == 4
    o = rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_strips', '--mesh-samples', '16', '--mesh-normals', 'vertex', '--mesh-texture-texels', '4']))
    assert o['samples'] == 16 and o['normals'] == 'vertex' and o['texture'] == dict(texels=4, filter='bilinear')
    for extra in (['--mesh-samples', '4'], ['--vis', 'video_grid', '--mesh-samples', '4'], ['--vis', 'shape_grid', '--mesh-samples', '16'],
                  ['--vis', 'image_grid', '--mesh-samples', '1'], ['--vis', 'shape_strips', '--mesh-samples', '4'], ['--vis', 'mesh_grid', '--mesh-samples', '2'],
                  ['--vis', 'mesh_grid', '--mesh-samples', '8'], ['--vis', 'mesh_grid', '--mesh-samples', '0'], ['--vis', 'mesh_grid', '--mesh-samples', 'many'],
                  ['--vis', 'mesh_grid', '--mesh-samples', '4', '--mesh-normals', 'field'], ['--vis', 'mesh_strips', '--mesh-samples', '16', '--mesh-normals', 'field']):
        with pytest.raises(SystemExit):
            p.parse_args(base + extra)
    assert '--mesh-samples' in capsys.readouterr().err

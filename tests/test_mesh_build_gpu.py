"""mesh_build on the GPU: the one per-sample build against its stages called by hand with all four of them on, and the two drivers
(geometry.extract_geometry, mesh.render_mesh_frames) against `build_mesh` on the planes each of them computes, bit for bit, on the seeded
config_tiny scene of the other driver tests."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, NV, VOL = 2, 3, 24
ORIGIN = (0.0, 0.0, 0.0)
STAGES = dict(components=dict(keep=1), smooth=dict(iterations=2), simplify=dict(cell=2.0), texture=dict(texels=4))
FRAME_FIELDS = ('rgb', 'depth', 'normal', 'status', 'tri')


def T(a):
    return torch.as_tensor(a).to(DEV)


def same_texture(got, want):
    return torch.equal(got.image, want.image) and torch.equal(torch.as_tensor(np.asarray(got.uvs)), torch.as_tensor(np.asarray(want.uvs))) and got.atlas == want.atlas


@pytest.fixture(scope='module')
def scene(tdgp):
    """config_tiny, seeded weights, 2 samples x 3 cameras, volume_res 24 over the whole field, the level at the median of the grid; the planes
    of both drivers and the record `build_mesh` makes of each sample's, computed once."""
    cfg = tdgp.config.config_tiny()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    G = G.to(DEV).eval()
    inp = tdgp.weights.synthetic_inputs(cfg, batch=B, seed=12)
    ws = G.mapping(T(inp['z']), T(inp['c']))
    cam_np = tdgp.weights.synthetic_inputs(cfg, batch=B * NV, seed=13)['camera']
    cams = tdgp.generator.TensorGroup(**{k: T(v) for k, v in cam_np.items()})
    box = 2.0 * cfg.cube_scale
    syn, HWC = G.synthesis, tdgp.renderer.HWCPlanes
    with torch.no_grad():
        level = float(tdgp.geometry.density_grid(G, ws, volume_res=VOL, cube_size=box).median())
        batch = syn.tri_planes(ws, noise_mode='const')                                           # as render_mesh_frames: one plane batch
        frame_planes = [HWC(batch.t[b:b + 1]) for b in range(B)]
        decoder = syn.tri_plane_decoder                                                          # as extract_geometry: the decoder, batch of one
        shape_planes = [tdgp.renderer.planes_to_hwc(decoder(ws[b:b + 1, :decoder.num_ws], hwc=True, noise_mode='const')) for b in range(B)]
    sc = dict(G=G, ws=ws, cams=cams, level=level, box=box, res=syn.test_resolution, frame_planes=frame_planes, shape_planes=shape_planes)
    sc['grid'] = dict(volume_res=VOL, voxel_origin=ORIGIN, cube_size=box, level=level, crop_slices=None, sheared=True)
    stages = tdgp.mesh_build.check_stages(**STAGES)
    sc['frame_meshes'] = [tdgp.mesh_build.build_mesh(G, p, stages, keep_grid=True, **sc['grid']) for p in frame_planes]
    sc['shape_meshes'] = [tdgp.mesh_build.build_mesh(G, p, stages, keep_grid=True, **sc['grid']) for p in shape_planes]
    return sc


def test_all_four_stages_are_the_stages_called_by_hand(tdgp, scene):
    g, sc, G = tdgp.geometry, scene, scene['G']
    for b, (planes, m) in enumerate(zip(sc['frame_planes'], sc['frame_meshes'])):
        sigma = g.density_grid_from_planes(G, planes, VOL, ORIGIN, sc['box'])[0]
        v, t = g.marching_cubes(sigma, sc['level'])
        v, t = tdgp.mesh_components.clean_mesh(v, t, keep=1)[:2]
        v = tdgp.mesh_surface.smooth(v, t, iterations=2)
        before = int(t.shape[0])
        v, t = tdgp.mesh_simplify.simplify(v, t, cell=2.0)[:2]
        world = g.grid_to_world(v, VOL, ORIGIN, sc['box'], None, True)
        tex = tdgp.mesh_texture.bake_field(G, planes, world, t, texels=4)
        print(f'sample {b}: {before} triangles before the simplification, {t.shape[0]} after, {v.shape[0]} vertices, atlas {tex.atlas}')
        assert 0 < t.shape[0] < before, (b, t.shape[0], before)
        assert torch.equal(m.vertices, v) and torch.equal(m.triangles, t) and torch.equal(m.world, world) and torch.equal(m.sigma, sigma), b
        assert same_texture(m.texture, tex) and int(tex.image.max()) > 0, b
        assert m.count == (v.shape[0], t.shape[0]) and m.count.triangles_before == before and m.count.atlas == tex.atlas, b


def test_extract_geometry_is_build_mesh_on_the_decoder_planes(tdgp, scene):
    g, sc = tdgp.geometry, scene
    kw = dict(volume_res=VOL, cube_size=sc['box'], thresh_value=sc['level'], crop=None, **STAGES)
    shapes, counts = g.extract_geometry(sc['G'], sc['ws'], units='world', return_counts=True, **kw)
    index = g.extract_geometry(sc['G'], sc['ws'], units='index', normalize=False, **kw)
    for b, m in enumerate(sc['shape_meshes']):
        assert type(shapes[b]) is g.TexturedShape and m.triangles.shape[0] > 0
        assert torch.equal(shapes[b].vertices, m.world) and torch.equal(shapes[b].triangles, m.triangles) and torch.equal(shapes[b].sigma, m.sigma), b
        assert same_texture(shapes[b].texture, m.texture) and same_texture(index[b].texture, m.texture), b
        assert torch.equal(index[b].vertices, m.vertices) and torch.equal(index[b].triangles, m.triangles), b
        assert counts[b] == m.count and counts[b].triangles_before == m.count.triangles_before and counts[b].atlas == m.count.atlas, b


@pytest.mark.parametrize('samples', [1, 4])
def test_render_mesh_frames_is_build_mesh_then_render_mesh_views(tdgp, scene, samples):
    Me, sc, G = tdgp.mesh, scene, scene['G']
    frames, counts = Me.render_mesh_frames(G, sc['ws'], sc['cams'], level=sc['level'], volume_res=VOL, mode='colour', normals='vertex', plane_batch=2,
                                           samples=samples, return_counts=True, **STAGES)
    fields = FRAME_FIELDS + (('coverage',) if samples > 1 else ())
    assert int(frames.status.sum()) > 0
    for b, m in enumerate(sc['frame_meshes']):
        cams = Me._camera_slice(sc['cams'], DEV, b * NV, (b + 1) * NV)
        want = Me.render_mesh_views(m.world, m.triangles, cams, sc['res'], G=G, mode='colour', normals='vertex', texture=m.texture, samples=samples)
        for k in fields:
            assert torch.equal(getattr(frames, k)[b * NV:(b + 1) * NV], getattr(want, k)), (b, k)
        assert counts[b] == m.count and counts[b].triangles_before == m.count.triangles_before and counts[b].atlas == m.count.atlas, b


def test_world_vertices_are_computed_once_and_the_texture_is_baked_on_them(tdgp, scene, monkeypatch):
    g, sc, G = tdgp.geometry, scene, scene['G']
    calls, grid_to_world = [], g.grid_to_world
    monkeypatch.setattr(g, 'grid_to_world', lambda *a, **k: calls.append(1) or grid_to_world(*a, **k))
    kw = dict(volume_res=VOL, cube_size=sc['box'], thresh_value=sc['level'], crop='reference', texture=dict(texels=4))
    shapes = g.extract_geometry(G, sc['ws'], units='world', **kw)
    assert len(calls) == B                                                              # one world array per sample
    index = g.extract_geometry(G, sc['ws'], units='index', normalize=False, **kw)
    for b in range(B):
        assert shapes[b].triangles.shape[0] > 0
        assert torch.equal(shapes[b].vertices, grid_to_world(index[b].vertices, VOL, ORIGIN, sc['box'], 'reference', True)), b
        assert same_texture(tdgp.mesh_texture.bake_field(G, sc['shape_planes'][b], shapes[b].vertices, shapes[b].triangles, texels=4), shapes[b].texture), b
        assert same_texture(index[b].texture, shapes[b].texture), b


def test_keep_grid_false_drops_the_grid_and_nothing_else(tdgp, scene):
    sc = scene
    stages = tdgp.mesh_build.check_stages(**STAGES)
    for b, (planes, m) in enumerate(zip(sc['frame_planes'], sc['frame_meshes'])):
        lean = tdgp.mesh_build.build_mesh(sc['G'], planes, stages, keep_grid=False, **sc['grid'])
        assert lean.sigma is None and m.sigma is not None
        assert torch.equal(lean.vertices, m.vertices) and torch.equal(lean.triangles, m.triangles) and torch.equal(lean.world, m.world), b
        assert same_texture(lean.texture, m.texture) and lean.count == m.count and lean.count.triangles_before == m.count.triangles_before, b
        assert lean.count.atlas == m.count.atlas, b

"""The mesh of one sample, from its planes to the finished mesh: density grid -> crop -> marching cubes -> components -> smoothing ->
simplification -> decimation -> world units -> texture -> ambient occlusion.  `geometry.extract_geometry` and `mesh.render_mesh_frames` obtain the planes, each its own way,
and call `build_mesh` once per sample: a stage is added here, once."""
import collections

from . import geometry as _geometry
from . import mesh_components as _mesh_components
from . import mesh_decimate as _mesh_decimate
from . import mesh_simplify as _mesh_simplify
from . import mesh_surface as _mesh_surface
from . import mesh_texture as _mesh_texture

Mesh = collections.namedtuple('Mesh', ['vertices', 'triangles', 'world', 'count', 'texture', 'sigma', 'occlusion'], defaults=(None,))
AO_KEYS = ('rays', 'radius', 'bias')


class Stages(collections.namedtuple('Stages', ['components', 'smooth', 'simplify', 'bake_kw', 'texture_filter', 'decimate'], defaults=(None,))):
    """The checked stage options: six fields, a plain tuple to whoever unpacks or compares them, and `.ao`, the options of the occlusion
    stage (None without it), carried beside them as `geometry.MeshCount` carries its extras."""
    ao = None


def check_stages(components, smooth, simplify, texture, decimate=None, ao=None):
    """The stage options of both drivers, in the order they run: each None (the stage is skipped) or a dict, checked before any device work
    -> Stages (bake_kw is None without a texture).  components and smooth are checked by their stages, not here.
    components: `mesh_components.select` keyword arguments (dict(keep=1)): `mesh_components.clean_mesh` drops the floaters on the device.
    smooth: `mesh_surface.smooth` keyword arguments (dict(iterations=10)).
    simplify: `mesh_simplify.simplify` keyword arguments with either `cell` (in voxels: dict(cell=2.0)) or `max_triangles`
    (dict(max_triangles=100000): the first cell of `mesh_simplify.cell_for_triangles`' ladder that leaves no more): vertex clustering with
    quadric placement; a count's `.triangles_before` holds what the mesh had before.
    decimate: `mesh_decimate.decimate` keyword arguments with `target_triangles`, `max_error` (in voxels) or both (dict(target_triangles=100000)):
    quadric edge collapse that keeps the surface closed, oriented and of the same topology; it runs after `simplify`, and a count's
    `.decimate` is then dict(rounds, stopped, triangles_before): what the stage was given and how it ended.
    texture: dict(texels=8, filter='bilinear') (also fill, points_per_call of `mesh_texture.bake`): baked from the sample's planes on the
    FINAL mesh in world units, where the field lives; a count's `.atlas` is then its `mesh_texture.Atlas`.
    ao: dict(rays=32, radius=None, bias=None) of `mesh_rays.vertex_occlusion` (radius and bias in world units): ambient occlusion per vertex of
    the finished world-space mesh, after every other stage; `Mesh.occlusion` is then fp32 [V] in [0, 1]."""
    if simplify is not None:
        _mesh_simplify.check_options(simplify)
    if decimate is not None:
        _mesh_decimate.check_options(decimate)
    bake_kw, texture_filter = (None, 'bilinear') if texture is None else _mesh_texture.check_options(texture)
    stages = Stages(components, smooth, simplify, bake_kw, texture_filter, decimate)
    if ao is not None:
        stages.ao = check_ao(ao)
    return stages


def check_ao(ao):
    """dict(rays=32, radius=None, bias=None) -> the dict with every key present, checked as `mesh_rays.ambient_occlusion` checks them."""
    from . import mesh_rays as _mesh_rays
    if not isinstance(ao, dict) or set(ao) - set(AO_KEYS):
        raise ValueError(f'ao must be a dict with keys among {AO_KEYS}, got {ao!r}')
    out = dict(rays=_mesh_rays._check_count(ao.get('rays', 32)), radius=ao.get('radius'), bias=ao.get('bias'))
    if out['radius'] is not None:
        out['radius'] = _mesh_rays._fp32(out['radius'], 'radius', True)
    if out['bias'] is not None:
        out['bias'] = _mesh_rays._fp32(out['bias'], 'bias', False)
    return out


def build_mesh(G, planes, stages, *, volume_res, voxel_origin, cube_size, level, crop_slices, sheared, slab_points=2 ** 22, keep_grid, world=True):
    """planes: the HWCPlanes of ONE sample; crop_slices: `geometry._crop_slices` -> Mesh(vertices in index units of the cropped grid, triangles,
    world: `grid_to_world` of the vertices, computed once and only for world=True, the bake or the occlusion (else None), count: a `geometry.MeshCount`,
    texture: a `mesh_texture.Texture` or None, sigma: the cropped grid, occlusion: fp32 [V] or None).  The stages run in index units.  keep_grid=False releases the grid
    right after marching cubes (sigma is None): nothing O(res^3) lives through the later stages."""
    sigma = _geometry.density_grid_from_planes(G, planes, volume_res, voxel_origin, cube_size, slab_points)[0]
    if crop_slices is not None:
        sigma = sigma[crop_slices]
    verts, tris = _geometry.marching_cubes(sigma, level)
    if not keep_grid:
        sigma = None
    if stages.components is not None:
        verts, tris = _mesh_components.clean_mesh(verts, tris, **dict(stages.components))[:2]
    if stages.smooth is not None:
        verts = _mesh_surface.smooth(verts, tris, **dict(stages.smooth))
    before = int(tris.shape[0])
    if stages.simplify is not None:
        verts, tris = _mesh_simplify.apply(verts, tris, stages.simplify)[:2]
    decimated = None
    if stages.decimate is not None:
        given = int(tris.shape[0])
        d = _mesh_decimate.apply(verts, tris, stages.decimate)
        verts, tris, decimated = d.vertices, d.triangles, dict(rounds=d.rounds, stopped=d.stopped, triangles_before=given)
    count = _geometry.MeshCount(verts.shape[0], tris.shape[0], before)
    if decimated is not None:
        count.decimate = decimated
    wv = tex = None
    if world or stages.bake_kw is not None or stages.ao is not None:
        wv = _geometry.grid_to_world(verts, volume_res, voxel_origin, cube_size, crop_slices, sheared)
    if stages.bake_kw is not None:
        tex = _mesh_texture.bake_field(G, planes, wv, tris, **stages.bake_kw)
        count.atlas = tex.atlas
    occlusion = None
    if stages.ao is not None:
        from . import mesh_rays as _mesh_rays
        occlusion = _mesh_rays.vertex_occlusion(wv, tris, **stages.ao)
    return Mesh(verts, tris, wv, count, tex, sigma, occlusion)

"""Mesh frames: the indexed mesh `geometry.marching_cubes` leaves on the device, rasterised from the cameras.

`shapes.render_shape_views` finds the surface of a density level on the rays, S + N + 7 field points per ray per frame.  The surface does not
change between the frames of a turn-table, so here it is extracted once per sample (`density_grid` -> `marching_cubes` -> `grid_to_world`)
and every frame is a visibility buffer of that mesh: tdgp_mesh_visibility (one triangle per lane, a 64-bit atomic minimum of (depth bits,
triangle) per covered pixel) -> tdgp_mesh_resolve (depth, face normal, colour, the 7 stencil points) -> tdgp_mesh_shade.  Smooth normals come either
from the mesh itself (normals='vertex': tdgp_mesh_interp_normals between the two, the vertex normals of mesh_surface.py interpolated at the
hit -- any mesh, no generator) or from the field (normals='field': the field at the 7 points and tdgp_iso_shade: 7 field points per pixel
instead of 87).  The colour of mode 'colour' is interpolated from one value per vertex by resolve, or, with a `mesh_texture.Texture`, fetched
from the per-triangle atlas baked from the field (tdgp_mesh_sample_texture between resolve and shade; mesh_texture.py).

The arithmetic of the three kernels is fixed operation by operation (include/tdgp.h); the minimum does not depend on the order of its
operands, so frames are the same bytes on every run, under every permutation of the triangles and every chunking of the cameras.  Limits:
no clipping at the near plane (a triangle with a vertex nearer than `near` is dropped whole: the cameras sit outside the cube), one mesh per
call.  GPU only: the kernels have no CPU path.

Anti-aliasing: `samples=4 | 16` decides coverage at 4 or 16 fixed sub-pixel positions per pixel in one pass --
tdgp_mesh_visibility_ms (one 8-byte key per sample, no ray table) -> tdgp_mesh_resolve_ms (every sample resolved and shaded with the
per-hit bodies of the one-sample kernels, averaged per pixel) -- and returns the covered fraction of every pixel.  The 16-sample pattern is
an ordered grid; normals from the field are not supersampled.
"""
import numpy as np
import torch

from . import _lib
from . import geometry as _geometry
from . import inference as _inference
from . import mesh_build as _mesh_build
from . import mesh_surface as _mesh_surface
from . import mesh_texture as _mesh_texture
from . import renderer as _renderer
from . import shapes as _shapes
from .generator import TensorGroup
from .geometry import FIELD_POINTS_MAX

MODES = _shapes.MODES
CULL = {'none': 0, 'back': 1, 'front': 2}
NORMALS = ('face', 'field', 'vertex')
STENCIL = _shapes.STENCIL


# ----------------------------------------------------------------------------------------------------------------------
# the three kernels on tensors
# ----------------------------------------------------------------------------------------------------------------------
def _check_mesh(vertices, triangles):
    for t, what in ((vertices, 'vertices'), (triangles, 'triangles')):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{what} must be a tensor, got {type(t).__name__}')
    if vertices.dtype != torch.float32 or vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f'vertices must be fp32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}')
    if triangles.dtype != torch.int32 or triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f'triangles must be int32 [T,3], got {triangles.dtype} {tuple(triangles.shape)}')
    _lib.require_cuda(vertices, 'vertices')
    _lib.require_cuda(triangles, 'triangles')
    return vertices.contiguous(), triangles.contiguous()


def focal_lengths(fov, C, device):
    """[C] fp32 1 / tan(fov / 2) of fields of view in degrees (a number, or a tensor of C): the angle as tdgp_sample_rays forms it in fp32, its
    tangent in float64 rounded once, so that the pixel grid of the rasteriser is the one the rays were shot through."""
    f = fov.to(device=device, dtype=torch.float32).reshape(-1) if isinstance(fov, torch.Tensor) else torch.full([1], float(fov), dtype=torch.float32, device=device)
    if f.numel() == 1:
        f = f.expand(C)
    if f.numel() != C:
        raise ValueError(f'fov must be a number or have {C} elements, got {f.numel()}')
    half = (f / 360.0 * 2.0 * float(np.float32(np.pi))) * 0.5
    return (1.0 / torch.tan(half.double()).float()).contiguous()


def mesh_visibility(vertices, triangles, c2w, focal, ray_d, resolution, near=1e-3, cull='none'):
    """tdgp_mesh_visibility: vertices [V,3] fp32 (world), triangles [T,3] int32, c2w [C,4,4], focal [C], ray_d [C,h*w,3] -> vis int64 [C,h*w]
    (the kernel's uint64 keys: -1 is an empty pixel, otherwise (bits(t) << 32) | triangle).  resolution: (w, h) as `sample_rays` takes it."""
    if cull not in CULL:
        raise ValueError(f'cull must be one of {sorted(CULL)}, got {cull!r}')
    vertices, triangles = _check_mesh(vertices, triangles)
    w, h = (int(resolution), int(resolution)) if np.isscalar(resolution) else (int(r) for r in resolution)
    _lib.require_cuda(ray_d, 'ray_d')
    c2w, focal, ray_d = _lib.f32c(c2w), _lib.f32c(focal), _lib.f32c(ray_d)
    C = int(c2w.shape[0]) if c2w.ndim == 3 else -1
    if tuple(c2w.shape) != (C, 4, 4) or focal.numel() != C or ray_d.numel() != C * h * w * 3:
        raise ValueError(f'mesh_visibility: c2w [C,4,4], focal [C], ray_d [C,{h * w},3] expected, got {tuple(c2w.shape)}, {tuple(focal.shape)}, {tuple(ray_d.shape)}')
    if not float(near) > 0.0:
        raise ValueError(f'near must be positive, got {near!r}')
    vis = torch.empty([C, h * w], dtype=torch.int64, device=vertices.device)
    with torch.cuda.device(vertices.device):
        _lib.call('tdgp_mesh_visibility', vertices.data_ptr(), vertices.shape[0], triangles.data_ptr(), triangles.shape[0], c2w.data_ptr(), focal.data_ptr(),
                  ray_d.data_ptr(), C, h, w, float(near), CULL[cull], vis.data_ptr(), _lib.stream_of(vertices))
    return vis


def mesh_resolve(vis, vertices, triangles, ray_o, ray_d, step, t_miss, vertex_rgb=None):
    """tdgp_mesh_resolve -> (t_hit [rays], status int32 [rays], tri int32 [rays], normal [rays,3], colour [rays,3] or None, points [rays,7,3])."""
    vertices, triangles = _check_mesh(vertices, triangles)
    _lib.require_cuda(vis, 'vis')
    if vis.dtype != torch.int64:
        raise ValueError(f'vis must be the int64 tensor mesh_visibility returns, got {vis.dtype}')
    vis, ray_o, ray_d = vis.contiguous(), _lib.f32c(ray_o), _lib.f32c(ray_d)
    rays = vis.numel()
    if ray_o.numel() != rays * 3 or ray_d.numel() != rays * 3:
        raise ValueError(f'mesh_resolve: ray_o / ray_d [{rays}, 3] expected')
    if vertex_rgb is not None:
        if vertex_rgb.dtype != torch.float32 or tuple(vertex_rgb.shape) != tuple(vertices.shape):
            raise ValueError(f'vertex_rgb must be fp32 {tuple(vertices.shape)}, got {vertex_rgb.dtype} {tuple(vertex_rgb.shape)}')
        _lib.require_cuda(vertex_rgb, 'vertex_rgb')
        vertex_rgb = vertex_rgb.contiguous()
    dev = vertices.device
    t_hit = torch.empty([rays], dtype=torch.float32, device=dev)
    status = torch.empty([rays], dtype=torch.int32, device=dev)
    tri = torch.empty([rays], dtype=torch.int32, device=dev)
    normal = torch.empty([rays, 3], dtype=torch.float32, device=dev)
    colour = None if vertex_rgb is None else torch.empty([rays, 3], dtype=torch.float32, device=dev)
    points = torch.empty([rays, STENCIL, 3], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_resolve', vis.data_ptr(), vertices.data_ptr(), vertices.shape[0], triangles.data_ptr(), triangles.shape[0], ray_o.data_ptr(),
                  ray_d.data_ptr(), rays, float(step), float(t_miss), _lib.ptr(vertex_rgb), t_hit.data_ptr(), status.data_ptr(), tri.data_ptr(),
                  normal.data_ptr(), _lib.ptr(colour), points.data_ptr(), _lib.stream_of(vertices))
    return t_hit, status, tri, normal, colour, points


def mesh_shade(normal, status, ray_d, colour=None, mode='shaded', light=None, ambient=0.2, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0)):
    """tdgp_mesh_shade: normal [rays,3], status int32 [rays], ray_d [rays,3], colour [rays,3] in [0, 1] (mode 'colour') -> rgb [rays,3]."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if mode == 'colour' and colour is None:
        raise ValueError("mode 'colour' needs the colour mesh_resolve interpolated (give it vertex_rgb)")
    _lib.require_cuda(normal, 'normal')
    normal, ray_d = _lib.f32c(normal), _lib.f32c(ray_d)
    rays = status.numel()
    if normal.numel() != rays * 3 or ray_d.numel() != rays * 3 or status.dtype != torch.int32 or (colour is not None and (colour.dtype != torch.float32 or colour.numel() != rays * 3)):
        raise ValueError(f'mesh_shade: normal [{rays}, 3], status int32 [{rays}], ray_d [{rays}, 3], colour fp32 [{rays}, 3] expected')
    status = status.contiguous()
    colour = None if colour is None else colour.contiguous()
    rgb = torch.empty([rays, 3], dtype=torch.float32, device=normal.device)
    with torch.cuda.device(normal.device):
        _lib.call('tdgp_mesh_shade', normal.data_ptr(), status.data_ptr(), ray_d.data_ptr(), _lib.ptr(colour), rays, MODES[mode],
                  None if light is None else _shapes._vec3(light, 'light'), float(ambient), _shapes._vec3(albedo, 'albedo'), _shapes._vec3(background, 'background'),
                  rgb.data_ptr(), _lib.stream_of(normal))
    return rgb


# ----------------------------------------------------------------------------------------------------------------------
# the two multisample kernels on tensors
# ----------------------------------------------------------------------------------------------------------------------
# offsets (ox, oy) of the samples from the pixel centre in 1/256 pixel, x to the right and y down, in sample order (include/tdgp.h)
SAMPLE_PATTERNS = {4: ((-32, -96), (96, -32), (-96, 32), (32, 96)),
                   16: tuple((ox, oy) for oy in (-96, -32, 32, 96) for ox in (-96, -32, 32, 96))}
SAMPLES = (1,) + tuple(SAMPLE_PATTERNS)


def _check_samples_ms(samples):
    if samples not in SAMPLE_PATTERNS:
        raise ValueError(f'samples must be one of {sorted(SAMPLE_PATTERNS)} here (one sample per pixel is mesh_visibility / mesh_resolve), got {samples!r}')
    return int(samples)


def _check_cameras_ms(what, c2w, focal, resolution):
    w, h = (int(resolution), int(resolution)) if np.isscalar(resolution) else (int(r) for r in resolution)
    _lib.require_cuda(c2w, 'c2w')
    c2w, focal = _lib.f32c(c2w), _lib.f32c(focal)
    C = int(c2w.shape[0]) if c2w.ndim == 3 else -1
    if tuple(c2w.shape) != (C, 4, 4) or focal.numel() != C:
        raise ValueError(f'{what}: c2w [C,4,4] and focal [C] expected, got {tuple(c2w.shape)}, {tuple(focal.shape)}')
    return c2w, focal, C, h, w


def mesh_visibility_ms(vertices, triangles, c2w, focal, resolution, samples, near=1e-3, cull='none'):
    """tdgp_mesh_visibility_ms: vertices [V,3] fp32 (world), triangles [T,3] int32, c2w [C,4,4], focal [C] -> vis int64 [C,h*w,samples] (the
    kernel's uint64 keys, one per sample of SAMPLE_PATTERNS[samples]: -1 is an empty sample, otherwise (bits(t) << 32) | triangle).  No ray
    table is read: the ray of a sample follows from its position.  resolution: (w, h) as `sample_rays` takes it."""
    if cull not in CULL:
        raise ValueError(f'cull must be one of {sorted(CULL)}, got {cull!r}')
    S = _check_samples_ms(samples)
    vertices, triangles = _check_mesh(vertices, triangles)
    c2w, focal, C, h, w = _check_cameras_ms('mesh_visibility_ms', c2w, focal, resolution)
    if not float(near) > 0.0:
        raise ValueError(f'near must be positive, got {near!r}')
    vis = torch.empty([C, h * w, S], dtype=torch.int64, device=vertices.device)
    with torch.cuda.device(vertices.device):
        _lib.call('tdgp_mesh_visibility_ms', vertices.data_ptr(), vertices.shape[0], triangles.data_ptr(), triangles.shape[0], c2w.data_ptr(), focal.data_ptr(),
                  C, h, w, S, float(near), CULL[cull], vis.data_ptr(), _lib.stream_of(vertices))
    return vis


def mesh_resolve_ms(vis, vertices, triangles, c2w, focal, resolution, t_miss, vertex_normals=None, vertex_rgb=None, texture=None, texture_filter='bilinear',
                    mode='shaded', light=None, ambient=0.2, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0)):
    """tdgp_mesh_resolve_ms: vis int64 [C,h*w,S] of `mesh_visibility_ms` -> (rgb [C*h*w,3], coverage [C*h*w], status int32 [C*h*w], depth
    [C*h*w], tri int32 [C*h*w], normal [C*h*w,3]).  Every sample is resolved and shaded as a ray of `mesh_resolve` (+ `interp_normals` with
    vertex_normals [V,3], + `sample_texture` with a texture) -> `mesh_shade` would be; rgb is the mean of the S colours, a miss counting as
    `background`; coverage the fraction of samples that hit; depth, tri and normal those of the nearest hit sample (t_miss, -1, 0 without one).
    mode 'colour' takes vertex_rgb [V,3] in [0, 1] or a `mesh_texture.Texture`, not both."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if texture_filter not in _mesh_texture.FILTERS:
        raise ValueError(f'texture_filter must be one of {sorted(_mesh_texture.FILTERS)}, got {texture_filter!r}')
    vertices, triangles = _check_mesh(vertices, triangles)
    c2w, focal, C, h, w = _check_cameras_ms('mesh_resolve_ms', c2w, focal, resolution)
    _lib.require_cuda(vis, 'vis')
    if vis.dtype != torch.int64 or vis.ndim != 3 or tuple(vis.shape[:2]) != (C, h * w) or vis.shape[2] not in SAMPLE_PATTERNS:
        raise ValueError(f'vis must be the int64 [{C}, {h * w}, 4 or 16] tensor mesh_visibility_ms returns, got {vis.dtype} {tuple(vis.shape)}')
    vis, S = vis.contiguous(), int(vis.shape[2])
    if vertex_rgb is not None and texture is not None:
        raise ValueError('the colour comes from vertex_rgb or from the texture, not both')
    if mode == 'colour' and vertex_rgb is None and texture is None:
        raise ValueError("mode 'colour' needs vertex_rgb [V,3] or a texture")
    for t, what in ((vertex_normals, 'vertex_normals'), (vertex_rgb, 'vertex_rgb')):
        if t is not None:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(vertices.shape):
                raise ValueError(f'{what} must be fp32 {tuple(vertices.shape)}, got {getattr(t, "dtype", type(t).__name__)} {tuple(getattr(t, "shape", ()))}')
            _lib.require_cuda(t, what)
    vertex_normals = None if vertex_normals is None else vertex_normals.contiguous()
    vertex_rgb = None if vertex_rgb is None else vertex_rgb.contiguous()
    image, atlas = None, _mesh_texture.Atlas(0, 0, 0, 0, 0)
    if texture is not None:
        atlas = _mesh_texture._check_texture(texture, int(triangles.shape[0]))
        _lib.require_cuda(texture.image, 'texture.image')
        image = texture.image.contiguous()
    dev, P = vertices.device, C * h * w
    rgb = torch.empty([P, 3], dtype=torch.float32, device=dev)
    coverage = torch.empty([P], dtype=torch.float32, device=dev)
    status = torch.empty([P], dtype=torch.int32, device=dev)
    depth = torch.empty([P], dtype=torch.float32, device=dev)
    tri = torch.empty([P], dtype=torch.int32, device=dev)
    normal = torch.empty([P, 3], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_mesh_resolve_ms', vis.data_ptr(), vertices.data_ptr(), vertices.shape[0], triangles.data_ptr(), triangles.shape[0], c2w.data_ptr(),
                  focal.data_ptr(), C, h, w, S, float(t_miss), _lib.ptr(vertex_normals), _lib.ptr(vertex_rgb), _lib.ptr(image), atlas.texels, atlas.tiles_per_row,
                  atlas.width, atlas.height, _mesh_texture.FILTERS[texture_filter], MODES[mode], None if light is None else _shapes._vec3(light, 'light'),
                  float(ambient), _shapes._vec3(albedo, 'albedo'), _shapes._vec3(background, 'background'), rgb.data_ptr(), coverage.data_ptr(),
                  status.data_ptr(), depth.data_ptr(), tri.data_ptr(), normal.data_ptr(), _lib.stream_of(vertices))
    return rgb, coverage, status, depth, tri, normal


# ----------------------------------------------------------------------------------------------------------------------
# frames
# ----------------------------------------------------------------------------------------------------------------------
def _check_options(mode, normals, cull, max_rays_per_call, texture=None, texture_filter='bilinear', samples=1):
    """The options of a frame that do not depend on the mesh (texture: only whether there is one)."""
    if isinstance(samples, bool) or samples not in SAMPLES:
        raise ValueError(f'samples must be one of {SAMPLES}, got {samples!r}')
    if samples > 1 and normals == 'field':
        raise ValueError("samples > 1 renders with normals='face' or 'vertex': normals='field' evaluates the field once per pixel and is not supersampled")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if normals not in NORMALS:
        raise ValueError(f'normals must be one of {NORMALS}, got {normals!r}')
    if cull not in CULL:
        raise ValueError(f'cull must be one of {sorted(CULL)}, got {cull!r}')
    if texture is not None:
        if normals == 'field':
            raise ValueError("texture is fetched with face or vertex normals; normals='field' takes its colour from the field at the hit")
        if mode != 'colour':
            raise ValueError(f"texture is the colour of mode='colour', got mode={mode!r}")
        if texture_filter not in _mesh_texture.FILTERS:
            raise ValueError(f'texture_filter must be one of {sorted(_mesh_texture.FILTERS)}, got {texture_filter!r}')
    if max_rays_per_call is not None and int(max_rays_per_call) < 1:
        raise ValueError(f'max_rays_per_call must be positive, got {max_rays_per_call!r}')


@torch.no_grad()
def vertex_colours(G, planes, vertices, points_per_call=2 ** 22):
    """The field's colour at the vertices of one sample's mesh (coords mode), `* 0.5 + 0.5`, clamped to [0, 1] -> [V,3] fp32."""
    _lib.require_cuda(vertices, 'vertices')
    point_field = _shapes.field_functions(G.synthesis)[1]
    out = torch.empty([vertices.shape[0], 3], dtype=torch.float32, device=vertices.device)
    step = int(min(max(int(points_per_call), 1), FIELD_POINTS_MAX))
    for i0 in range(0, vertices.shape[0], step):
        v = _lib.f32c(vertices[i0:i0 + step]).unsqueeze(0)
        out[i0:i0 + step] = (point_field(planes, v)[0, :, :3] * 0.5 + 0.5).clamp_(0.0, 1.0)
    return out


# the pieces of a frame: name, trailing shape, dtype; `coverage` with samples > 1 only
FIELDS = (('rgb', (3,), torch.float32), ('depth', (1,), torch.float32), ('normal', (3,), torch.float32), ('status', (), torch.int32),
          ('tri', (), torch.int32), ('coverage', (), torch.float32))


@torch.no_grad()
def render_mesh_views(vertices, triangles, camera_params, resolution, mode='shaded', normals='face', cull='none', near=None, planes=None, G=None,
                      vertex_colours=None, light=None, ambient=0.2, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0), max_rays_per_call=None,
                      t_miss=None, step=None, vertex_normals=None, texture=None, texture_filter='bilinear', samples=1, vertex_occlusion=None):
    """C frames of ONE mesh (vertices [V,3] fp32 in world units, triangles [T,3] int32, on the device) under C cameras (`camera_params`: angles,
    radius, look_at, fov as the renderer takes them) at `resolution` (a side, or (w, h)).

    -> TensorGroup(rgb [C,R,3], depth [C,R,1], normal [C,R,3], status int32 [C,R], tri int32 [C,R]), ray-major, on the device: the layout and
    meanings of `shapes.render_shape_views`.  status 1: a hit, 0: a miss (rgb = background, normal = 0, tri = -1, depth = t_miss: default
    cfg.ray_end with a generator, 0 without).  depth is the ray parameter of the hit.
    normals='face': the flat normal of the hit triangle (its stored winding; marching cubes: toward lower density) -- no generator is needed, any
    mesh renders.  normals='field': `planes` (this sample's, batch 1) and `G`: the field at the 7 stencil points of every pixel and
    tdgp_iso_shade -- smooth normals, and mode='colour' takes the field's colour at the hit; `step` is the stencil step (default one
    tri-plane texel).  normals='vertex': smooth normals from the mesh alone -- `vertex_normals` [V,3] fp32 (default: `mesh_surface.vertex_normals`
    of this mesh, area weight, computed once per call) interpolated at every hit with the weights of the colour interpolation and normalised
    (tdgp_mesh_interp_normals); no generator is needed.  A mesh on the CPU is refused as a bad option (ValueError): the mode exists on the device only.  mode='colour' with face or vertex normals interpolates `vertex_colours` [V,3] in [0, 1].
    texture: None, or the `mesh_texture.Texture` baked for THIS mesh (its uvs have T rows, else ValueError): mode='colour' with face or vertex
    normals then takes the colour of every hit from the texture (tdgp_mesh_sample_texture between resolve and shade; texture_filter
    'bilinear' | 'nearest') instead of `vertex_colours`, which is not needed.  The colour is still lit: ambient=1.0 gives the unlit texture.
    texture with normals='field', or with another mode, is a ValueError.
    cull: 'none' | 'back' | 'front'.  near (default cfg.ray_start with a generator, else 1e-3): a triangle with a vertex nearer is dropped whole.
    Cameras are taken in chunks of whole frames, max_rays_per_call rays at most (default 16 frames; never less than one frame): they are
    independent, so the chunking does not change a byte.
    samples: 1 (one point sample at the pixel centre: the route above), 4 (a rotated grid) or 16 (the 4 x 4 grid) coverage samples per pixel
    (SAMPLE_PATTERNS), with face or vertex normals.  Every sample is visible, resolved and shaded on its own ray, in two launches per chunk
    (tdgp_mesh_visibility_ms -> tdgp_mesh_resolve_ms, 8 bytes per sample between them): rgb is the mean of the sample colours over
    `background`, and the group gains coverage [C,R], the fraction of the pixel's samples the mesh covers (composite another background B as
    rgb + (1 - coverage) * (B - background)).  status is 1 where any sample hit; depth, tri and normal are those of the nearest hit sample.  The
    frame stays on the pixel grid of the one-sample frame and of the renderer's frames of the same cameras.  The chunks shrink by `samples`.
    vertex_occlusion: None, or fp32 [V] in [0, 1] (`mesh_rays.vertex_occlusion`: 1 = open) that darkens the surface colour before it is lit.
    mode='colour' with `vertex_colours`: the colours times it, one fp32 multiply; mode='shaded': the frame goes through the colour path with
    albedo * occlusion as vertex colours.  With a texture, normals='field' or mode='normals' it is a ValueError."""
    _check_options(mode, normals, cull, max_rays_per_call, texture, texture_filter, samples)
    if vertex_occlusion is not None and (texture is not None or normals == 'field' or mode == 'normals'):
        raise ValueError(f"vertex_occlusion darkens vertex colours: it takes mode 'shaded' or 'colour' with face or vertex normals and no texture (got mode={mode!r}, "
                         f"normals={normals!r}{', a texture' if texture is not None else ''})")
    # what those options need of this mesh: the field behind it, its colours, its normals
    if normals == 'field' and (planes is None or G is None):
        raise ValueError("normals='field' evaluates the field at the hits: it needs the generator G and the sample's planes (G.synthesis.tri_planes)")
    if normals != 'field' and mode == 'colour' and vertex_colours is None and texture is None:
        raise ValueError(f"mode='colour' with normals={normals!r} needs vertex_colours [V,3] (mesh.vertex_colours)")
    if vertex_normals is not None:
        if normals != 'vertex':
            raise ValueError(f"vertex_normals are read by normals='vertex' only, got normals={normals!r}")
        if not isinstance(vertex_normals, torch.Tensor) or vertex_normals.dtype != torch.float32 or vertex_normals.ndim != 2 or vertex_normals.shape[1] != 3:
            raise ValueError(f'vertex_normals must be an fp32 [V,3] tensor (mesh_surface.vertex_normals), got {getattr(vertex_normals, "dtype", type(vertex_normals).__name__)} '
                             f'{tuple(getattr(vertex_normals, "shape", ()))}')
    if normals == 'vertex' and isinstance(vertices, torch.Tensor) and isinstance(triangles, torch.Tensor) and not (vertices.is_cuda and triangles.is_cuda):
        # this mode is an option of a device mesh only (its corner table is built there): asking for it on a host mesh is a bad option value
        raise ValueError(f"normals='vertex' takes a mesh on the GPU (got {vertices.device}, {triangles.device}); the vertex normals have no CPU path")
    vertices, triangles = _check_mesh(vertices, triangles)
    if vertex_occlusion is not None:
        if not isinstance(vertex_occlusion, torch.Tensor) or vertex_occlusion.dtype != torch.float32 or tuple(vertex_occlusion.shape) != (int(vertices.shape[0]),) \
                or vertex_occlusion.device != vertices.device:
            raise ValueError(f'vertex_occlusion must be an fp32 [{int(vertices.shape[0])}] tensor on {vertices.device} (mesh_rays.vertex_occlusion), got '
                             f'{getattr(vertex_occlusion, "dtype", type(vertex_occlusion).__name__)} {tuple(getattr(vertex_occlusion, "shape", ()))}')
    w, h = (int(resolution), int(resolution)) if np.isscalar(resolution) else (int(r) for r in resolution)
    if h < 2 or w < 2:
        raise ValueError(f'resolution must be at least 2 x 2, got {resolution!r}')
    cfg = None if G is None else G.cfg
    near = (float(cfg.ray_start) if cfg is not None else 1e-3) if near is None else float(near)
    t_miss = (float(cfg.ray_end) if cfg is not None else 0.0) if t_miss is None else float(t_miss)
    if step is None:
        step = 2.0 * float(cfg.cube_scale) / int(cfg.tri_plane_res) if cfg is not None else 0.0
    dev = vertices.device
    R = h * w
    get = _renderer.cam_get(camera_params)
    c2w = _renderer.compute_cam2world_matrix(camera_params)
    C = int(c2w.shape[0])
    focal = focal_lengths(get('fov'), C, dev)
    if samples == 1:
        ray_o, ray_d = _renderer.sample_rays(c2w, fov=get('fov'), resolution=(w, h))
    point_field = None
    if normals == 'field':
        if G.synthesis.training:
            raise RuntimeError('render_mesh_views is the inference route: call .eval() first')
        if not isinstance(planes, _renderer.HWCPlanes) or int(planes.t.shape[0]) != 1:
            raise TypeError("normals='field' takes the HWCPlanes of ONE sample (tri_planes of a batch of one, or HWCPlanes(planes.t[b:b + 1]))")
        point_field = _shapes.field_functions(G.synthesis)[1]
    vnorm = None
    if normals == 'vertex':
        if vertex_normals is not None and tuple(vertex_normals.shape) != tuple(vertices.shape):
            raise ValueError(f'vertex_normals must be fp32 {tuple(vertices.shape)}, got {tuple(vertex_normals.shape)}')
        vnorm = _mesh_surface.vertex_normals(vertices, triangles) if vertex_normals is None else vertex_normals
    if texture is not None:
        _mesh_texture._check_texture(texture, int(triangles.shape[0]))
    vrgb = None
    if point_field is None and mode == 'colour' and texture is None:
        vrgb = vertex_colours if vertex_colours.dtype == torch.float32 else vertex_colours.float() / (255.0 if vertex_colours.dtype == torch.uint8 else 1.0)
    if vertex_occlusion is not None:                # plumbing: the surface colour times the occlusion, then the colour path as it is
        base = vrgb if mode == 'colour' else torch.tensor([float(a) for a in albedo], dtype=torch.float32, device=dev)[None, :]
        vrgb = base * vertex_occlusion[:, None]
        mode = 'colour'
    max_rays = 16 * R if max_rays_per_call is None else int(max_rays_per_call)
    cstep = max(1, min(max_rays, FIELD_POINTS_MAX // STENCIL) // (R * samples))
    shade = dict(mode=mode, light=light, ambient=ambient, albedo=albedo, background=background)
    fields = FIELDS if samples > 1 else FIELDS[:-1]

    def one_sample(cs):                         # a chunk of cameras -> its pieces by name, ray-flat
        o, d = ray_o[cs].reshape(-1, 3), ray_d[cs].reshape(-1, 3)
        n = o.shape[0]
        vis = mesh_visibility(vertices, triangles, c2w[cs], focal[cs], d, (w, h), near=near, cull=cull)
        t_hit, status, tri, normal, colour, points = mesh_resolve(vis.reshape(n), vertices, triangles, o, d, step, t_miss, vertex_rgb=vrgb)
        if point_field is not None:
            rgb, normal = _shapes.iso_shade(point_field(planes, points.reshape(1, n * STENCIL, 3)), status, d, **shade)
        else:
            if vnorm is not None:
                _mesh_surface.interp_normals(tri, status, t_hit, _lib.f32c(o), _lib.f32c(d), vertices, triangles, vnorm, normal)
            if texture is not None:
                colour = _mesh_texture.sample_texture(tri, status, t_hit, _lib.f32c(o), _lib.f32c(d), vertices, triangles, texture, texture_filter)
            rgb = mesh_shade(normal, status, d, colour=colour, **shade)
        return dict(rgb=rgb, depth=t_hit, normal=normal, status=status, tri=tri)

    def multisample(cs):                        # the same, with `coverage`
        vis = mesh_visibility_ms(vertices, triangles, c2w[cs], focal[cs], (w, h), samples, near=near, cull=cull)
        rgb, coverage, status, depth, tri, normal = mesh_resolve_ms(vis, vertices, triangles, c2w[cs], focal[cs], (w, h), t_miss, vertex_normals=vnorm,
                                                                    vertex_rgb=vrgb, texture=texture, texture_filter=texture_filter, **shade)
        return dict(rgb=rgb, depth=depth, normal=normal, status=status, tri=tri, coverage=coverage)
    out = _renderer.Gather(C, R)
    for c0 in range(0, C, cstep):
        cs = slice(c0, min(c0 + cstep, C))
        pieces = multisample(cs) if samples > 1 else one_sample(cs)
        out.put(cs, slice(0, R), **{name: pieces[name].reshape(cs.stop - cs.start, R, *shape) for name, shape, _ in fields})
    values = out.result() if C else [torch.empty([0, R, *shape], dtype=dtype, device=dev) for _, shape, dtype in fields]
    return TensorGroup(**{name: value for (name, _, _), value in zip(fields, values)})


def _camera_slice(camera_params, device, c0, c1):
    """Cameras c0 .. c1 of an attribute bag or dict, fp32 on `device`."""
    get = _renderer.cam_get(camera_params)
    cam = {k: get(k).to(dtype=torch.float32, device=device)[c0:c1] for k in ('angles', 'radius', 'look_at')}
    fov = get('fov')
    cam['fov'] = fov.to(dtype=torch.float32, device=device).reshape(-1)[c0:c1] if isinstance(fov, torch.Tensor) and fov.numel() > 1 else fov
    return cam


@torch.no_grad()
def render_mesh_frames(G, ws, camera_params, level=25.0, volume_res=256, voxel_origin=(0.0, 0.0, 0.0), cube_size=None, crop=None, sheared=True,
                       mode='shaded', normals='face', plane_batch=4, return_counts=False, components=None, smooth=None, simplify=None, texture=None, decimate=None,
                       ao=None, **kw):
    """Mesh frames of every `ws` under its cameras (sample-major: camera n * V + v is view v of sample n).  Per sample: `mesh_build.build_mesh`
    -- the density grid at volume_res^3 over a cube of `cube_size` (default the whole field, 2 * cfg.cube_scale), marching cubes at `level`, the
    stages, `grid_to_world` -- then its V cameras through `render_mesh_views`.  The backbone runs once per plane batch; its planes feed the
    build and, with normals='field' (or face normals in mode 'colour'), the field lookups of the frames.
    -> TensorGroup(rgb [B*V,R,3], depth, normal, status, tri) as `render_mesh_views`; return_counts=True: also a `geometry.MeshCount` per sample.
    components, smooth, simplify, decimate, texture: the stages of `mesh_build.check_stages`.  Normals, vertex colours (mode 'colour') and counts are
    those of the finished mesh in world units; with a texture the frames take their colour from it (mode='colour', face or vertex normals).
    ao: dict(rays=32, radius=None, bias=None): ambient occlusion per vertex of the finished mesh (`mesh_rays.vertex_occlusion`), handed to
    `render_mesh_views(vertex_occlusion=)` -- mode 'shaded' or 'colour', face or vertex normals, no texture.
    kw: cull, near, light, ambient, albedo, background, max_rays_per_call, t_miss, step, samples of `render_mesh_views` (samples=4 | 16: multisampled
    frames, and the group gains `coverage`; the grids and strips below take it the same way)."""
    syn, cfg = G.synthesis, G.cfg
    num_samples = len(ws)
    get = _renderer.cam_get(camera_params)
    V = _renderer.views_per_sample(int(get('angles').shape[0]), num_samples, f'{num_samples} samples')
    if int(plane_batch) < 1:
        raise ValueError(f'plane_batch must be positive, got {plane_batch!r}')
    stages = _mesh_build.check_stages(components, smooth, simplify, texture, decimate, ao)
    if stages.ao is not None and (texture is not None or normals == 'field' or mode == 'normals'):
        raise ValueError(f"ao darkens vertex colours: it takes mode 'shaded' or 'colour' with face or vertex normals and no texture (got mode={mode!r}, normals={normals!r})")
    _check_options(mode, normals, kw.get('cull', 'none'), kw.get('max_rays_per_call'), texture, stages.texture_filter, kw.get('samples', 1))
    if syn.training:
        raise RuntimeError('render_mesh_frames is the inference route: call .eval() first (training mode renders patches with density noise)')
    _lib.require_cuda(ws, 'ws')
    cube_size = 2.0 * float(cfg.cube_scale) if cube_size is None else float(cube_size)
    slices = _geometry._crop_slices(crop, volume_res)
    res = syn.test_resolution
    parts, counts = [], []
    for n0 in range(0, num_samples, int(plane_batch)):
        n1 = min(n0 + int(plane_batch), num_samples)
        planes = syn.tri_planes(ws[n0:n1], noise_mode='const')
        for b in range(n1 - n0):
            pb = _renderer.HWCPlanes(planes.t[b:b + 1])
            m = _mesh_build.build_mesh(G, pb, stages, volume_res=volume_res, voxel_origin=voxel_origin, cube_size=cube_size, level=level, crop_slices=slices,
                                       sheared=sheared, keep_grid=False)
            counts.append(m.count)
            vc = vertex_colours(G, pb, m.world) if (mode == 'colour' and normals != 'field' and m.texture is None) else None
            cams = _camera_slice(camera_params, ws.device, (n0 + b) * V, (n0 + b + 1) * V)
            parts.append(render_mesh_views(m.world, m.triangles, cams, res, mode=mode, normals=normals, planes=pb if normals == 'field' else None, G=G,
                                           vertex_colours=vc, **({} if m.texture is None else dict(texture=m.texture, texture_filter=stages.texture_filter)),
                                           **({} if m.occlusion is None else dict(vertex_occlusion=m.occlusion)), **kw))
    frames = parts[0] if len(parts) == 1 else TensorGroup.cat(parts, dim=0)
    return (frames, counts) if return_counts else frames


def _mesh_frames_tail(tail, G, ws, camera_params, show, return_counts, kw):
    """tail(num_samples, V, the `show` buffer of `render_mesh_frames` as a callable) -> what it returns, with the per-sample counts when asked."""
    num_samples, counts = len(ws), []
    V = int(_renderer.cam_get(camera_params)('angles').shape[0]) // max(num_samples, 1)

    def all_frames():
        frames, counts[:] = render_mesh_frames(G, ws, camera_params, return_counts=True, **kw)
        return frames
    out = tail(num_samples, V, lambda: _inference.shown(show, all_frames))
    return (out, counts) if return_counts else out


def render_mesh_video_grid(G, ws, camera_params, nrow='auto', show='rgb', num_videos=None, padding=2, as_numpy=False, return_counts=False, **kw):
    """`shapes.render_shape_video_grid` of mesh frames: frame t of the video is the make_grid of every sample's mesh view t -> uint8
    [T, GH, GW, 3] on the device (as_numpy=True: one copy to the host).  kw: the options of `render_mesh_frames`."""
    return _mesh_frames_tail(lambda n, V, frames: _inference.video_grid_of(G, n, V, frames, nrow, num_videos, padding, show == 'depth', as_numpy),
                             G, ws, camera_params, show, return_counts, kw)


def render_mesh_strips(G, ws, camera_params, show='rgb', as_numpy=False, return_counts=False, **kw):
    """`shapes.render_shape_strips` of mesh frames: per sample, its mesh views side by side -> uint8 [num_samples, h, V * w, 3] on the device."""
    return _mesh_frames_tail(lambda n, V, frames: _inference.strips_of(G, n, V, frames, show == 'depth', as_numpy), G, ws, camera_params, show, return_counts, kw)

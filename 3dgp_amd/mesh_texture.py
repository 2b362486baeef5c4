"""Mesh textures: a per-triangle atlas of the extracted mesh baked from the field, and its fetch at the hits of a mesh frame (DESIGN.md 5.23;
csrc/mesh_texture.hip, contract in include/tdgp.h).

A mesh carries one RGB value per vertex (`mesh.vertex_colours`); after `mesh_simplify.simplify` that is a tenth of the colour samples the
level set had, while the field still holds the colour at full resolution.  `bake` gives every triangle its own right-angled chart of
`texels` x `texels` / 2 texels -- two triangles per square tile, the second one turned by a half turn -- evaluates `colour_fn` at the point
every texel stands for and stores the colours as an 8-bit image.  The layout (`atlas_layout`, `atlas_uvs`) is a pure function of the
triangle count: no unwrapping, no packing heuristics, the same bytes on every run.  `mesh.render_mesh_views(texture=...)` fetches the image
at every hit (tdgp_mesh_sample_texture, nearest or bilinear), and `geometry.save_obj(uvs=, texture=)` writes it for other programs.

Limits, named plainly: per-triangle charts waste about half of each tile's diagonal band and no chart spans triangles, so the atlas is
about (n + 2)^2 / n^2 larger than its payload and a viewer's bilinear filter sees the gutter, not the neighbouring triangle, across an
edge; there are no mip levels (a viewer that builds its own will bleed across tiles); 8 bits per channel; a texel of a simplified triangle
lies up to the simplification error off the iso-surface and takes the field's colour THERE; nothing here is differentiable.  GPU only.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from . import mesh_surface as _mesh_surface
from . import shapes as _shapes
from .geometry import FIELD_POINTS_MAX

Atlas = collections.namedtuple('Atlas', ['texels', 'tile', 'tiles_per_row', 'width', 'height'])
Texture = collections.namedtuple('Texture', ['image', 'uvs', 'atlas'])
FILTERS = {'nearest': 0, 'bilinear': 1}
TEXELS_MIN, TEXELS_MAX, SIDE_MAX = 2, 64, 16384


# ----------------------------------------------------------------------------------------------------------------------
# the layout: host side, integers only
# ----------------------------------------------------------------------------------------------------------------------
def atlas_layout(T, texels):
    """The atlas of T triangles at `texels` = n texels along a leg -> Atlas(texels=n, tile=S, tiles_per_row=r, width=W, height=H):
    S = n + 2, P = ceil(T / 2) tiles, r the smallest integer with r * r >= P, W = r * S, H = ceil(P / r) * S.  Tile k has its origin at
    ((k % r) * S, (k // r) * S) and holds triangles 2k (texels with px + py <= n) and 2k + 1 (the others, turned by a half turn).
    2 <= texels <= 64 and W, H <= 16384, else ValueError."""
    T, n = int(T), int(texels)
    if n != texels or not TEXELS_MIN <= n <= TEXELS_MAX:
        raise ValueError(f'texels must be an integer in [{TEXELS_MIN}, {TEXELS_MAX}], got {texels!r}')
    if T < 0 or T > 2 ** 31 - 1:
        raise ValueError(f'the triangle count must lie in [0, 2^31 - 1], got {T}')
    S, P = n + 2, (T + 1) // 2
    r = int(np.ceil(np.sqrt(P)))
    while r * r < P:
        r += 1
    while r > 0 and (r - 1) * (r - 1) >= P:
        r -= 1
    W, H = r * S, (-(-P // r) if r else 0) * S
    if W > SIDE_MAX or H > SIDE_MAX:
        raise ValueError(f'an atlas of {W} x {H} texels ({T} triangles at {n} texels) exceeds the limit of {SIDE_MAX} x {SIDE_MAX}: take fewer texels, or simplify the mesh')
    return Atlas(texels=n, tile=S, tiles_per_row=r, width=W, height=H)


def _check_atlas(atlas, T):
    if not isinstance(atlas, Atlas):
        raise TypeError(f'atlas must be the Atlas `atlas_layout` returns, got {type(atlas).__name__}')
    want = atlas_layout(T, atlas.texels)
    if tuple(atlas) != tuple(want):
        raise ValueError(f'{atlas} is not the atlas of {T} triangles at {atlas.texels} texels ({want})')
    return want


def atlas_uvs(T, atlas):
    """-> [T,3,2] fp32 (a numpy array), one (u, v) per corner: the texel CENTRES of the corners, v0 at the right angle of the chart.  Lower
    triangle of the tile at (X0, Y0): (X0, Y0), (X0 + n - 1, Y0), (X0, Y0 + n - 1); upper: (X0 + S - 1, Y0 + S - 1), (X0 + S - n, Y0 + S - 1),
    (X0 + S - 1, Y0 + S - n).  u = (x + 0.5) / W, v = 1 - (y + 0.5) / H in float64, rounded once: image row 0 is the top row of the file."""
    T = int(T)
    atlas = _check_atlas(atlas, T)
    n, S, r = atlas.texels, atlas.tile, atlas.tiles_per_row
    if T == 0:
        return np.empty((0, 3, 2), np.float32)
    # u depends on a tile's column and v on its row alone: the six corners of one column of tiles and of one row are computed once and
    # broadcast over the grid of tiles (this runs on the host inside every bake, and a mesh has far more corners than its atlas has columns)
    rows = atlas.height // S
    qx, qy = np.array([0, n - 1, 0, S - 1, S - n, S - 1], np.int64), np.array([0, 0, n - 1, S - 1, S - 1, S - n], np.int64)
    x = (np.arange(r, dtype=np.int64) * S)[:, None] + qx[None, :]
    y = (np.arange(rows, dtype=np.int64) * S)[:, None] + qy[None, :]
    u = ((x.astype(np.float64) + 0.5) / float(atlas.width)).astype(np.float32)
    v = (1.0 - (y.astype(np.float64) + 0.5) / float(atlas.height)).astype(np.float32)
    out = np.empty((rows, r, 6, 2), np.float32)
    out[..., 0] = u[None, :, :]
    out[..., 1] = v[:, None, :]
    return out.reshape(rows * r * 2, 3, 2)[:T]


# ----------------------------------------------------------------------------------------------------------------------
# the three kernels on tensors
# ----------------------------------------------------------------------------------------------------------------------
def atlas_points(vertices, triangles, atlas):
    """tdgp_atlas_points -> (points fp32 [H*W,3], owner int32 [H*W]): per texel the point of its triangle's plane it stands for (unowned:
    0) and the triangle's index (-1: unowned, or a triangle naming a vertex that does not exist)."""
    vertices, triangles = _mesh_surface._check_mesh(vertices, triangles)
    T = int(triangles.shape[0])
    atlas = _check_atlas(atlas, T)
    dev = vertices.device
    texels = atlas.width * atlas.height
    points = torch.empty([texels, 3], dtype=torch.float32, device=dev)
    owner = torch.empty([texels], dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('tdgp_atlas_points', vertices.data_ptr(), vertices.shape[0], triangles.data_ptr(), T, atlas.texels, atlas.tiles_per_row, atlas.width,
                  atlas.height, points.data_ptr(), owner.data_ptr(), _lib.stream_of(vertices))
    return points, owner


def _fill_bytes(fill):
    f = np.asarray(fill)
    if f.shape != (3,) or not np.all((f >= 0) & (f <= 255) & (f == np.floor(f))):
        raise ValueError(f'fill must be three integers in [0, 255], got {fill!r}')
    return (ctypes.c_uint8 * 3)(*(int(x) for x in f))


def atlas_texels(rgb, owner, image, fill=(0, 0, 0)):
    """tdgp_atlas_texels: rgb fp32 [N, >=3] in [-1, 1] (rows may be strided: the field's [N,4] is read in place), owner int32 [N] -> image, a
    contiguous uint8 [N,3] (a run of the atlas' texels) written IN PLACE: (uint8)rint(clamp(c * 0.5 + 0.5, 0, 1) * 255), `fill` where owner < 0."""
    for t, what in ((rgb, 'rgb'), (owner, 'owner'), (image, 'image')):
        _lib.require_cuda(t, what)
    N = int(owner.numel())
    if rgb.dtype != torch.float32 or rgb.ndim != 2 or rgb.shape[0] != N or rgb.shape[1] < 3:
        raise ValueError(f'atlas_texels: rgb must be fp32 [{N}, >=3], got {rgb.dtype} {tuple(rgb.shape)}')
    if owner.dtype != torch.int32 or not owner.is_contiguous() or image.dtype != torch.uint8 or image.numel() != N * 3 or not image.is_contiguous():
        raise ValueError(f'atlas_texels: owner must be contiguous int32 [{N}] and image contiguous uint8 [{N}, 3], got {owner.dtype} {tuple(owner.shape)}, '
                         f'{image.dtype} {tuple(image.shape)}')
    if N <= 1 or rgb.stride(1) != 1 or not 3 <= rgb.stride(0) <= 1024:
        rgb = rgb[:, :3].contiguous()
    stride = int(rgb.stride(0)) if N > 1 else 3
    fill = _fill_bytes(fill)
    with torch.cuda.device(owner.device):
        _lib.call('tdgp_atlas_texels', rgb.data_ptr(), stride, owner.data_ptr(), N, fill, image.data_ptr(), _lib.stream_of(owner))
    return image


def _check_texture(texture, T):
    if not isinstance(texture, Texture):
        raise TypeError(f'texture must be the Texture `mesh_texture.bake` returns, got {type(texture).__name__}')
    if tuple(np.shape(texture.uvs)) != (T, 3, 2):
        raise ValueError(f'texture.uvs must be [{T}, 3, 2] for this mesh of {T} triangles, got {tuple(np.shape(texture.uvs))}: the texture was baked for another mesh')
    atlas = _check_atlas(texture.atlas, T)
    image = texture.image
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or tuple(image.shape) != (atlas.height, atlas.width, 3):
        raise ValueError(f'texture.image must be a uint8 [{atlas.height}, {atlas.width}, 3] tensor, got {getattr(image, "dtype", type(image).__name__)} '
                         f'{tuple(getattr(image, "shape", ()))}')
    return atlas


def sample_texture(tri, status, t_hit, ray_o, ray_d, vertices, triangles, texture, filter='bilinear'):
    """tdgp_mesh_sample_texture: tri / status / t_hit as `mesh.mesh_resolve` returned them, ray_o / ray_d [rays,3] -> colour fp32 [rays,3] in
    [0, 1], the texture fetched inside the hit triangle's chart at the barycentric weights of the hit ('nearest' | 'bilinear'); 0 on a miss."""
    if filter not in FILTERS:
        raise ValueError(f'texture_filter must be one of {sorted(FILTERS)}, got {filter!r}')
    vertices, triangles = _mesh_surface._check_mesh(vertices, triangles)
    atlas = _check_texture(texture, int(triangles.shape[0]))
    rays = int(status.numel())
    for t, what, dt, n in ((tri, 'tri', torch.int32, rays), (status, 'status', torch.int32, rays), (t_hit, 't_hit', torch.float32, rays),
                           (ray_o, 'ray_o', torch.float32, rays * 3), (ray_d, 'ray_d', torch.float32, rays * 3)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError(f'sample_texture: {what} must be contiguous {dt} with {n} elements, got {t.dtype} {tuple(t.shape)}')
        _lib.require_cuda(t, what)
    _lib.require_cuda(texture.image, 'texture.image')
    image = texture.image.contiguous()
    colour = torch.empty([rays, 3], dtype=torch.float32, device=vertices.device)
    with torch.cuda.device(vertices.device):
        _lib.call('tdgp_mesh_sample_texture', tri.data_ptr(), status.data_ptr(), t_hit.data_ptr(), ray_o.data_ptr(), ray_d.data_ptr(), rays, vertices.data_ptr(),
                  vertices.shape[0], triangles.data_ptr(), triangles.shape[0], image.data_ptr(), atlas.texels, atlas.tiles_per_row, atlas.width, atlas.height,
                  FILTERS[filter], colour.data_ptr(), _lib.stream_of(vertices))
    return colour


# ----------------------------------------------------------------------------------------------------------------------
# the bake
# ----------------------------------------------------------------------------------------------------------------------
OPTION_KEYS = ('texels', 'filter', 'fill', 'points_per_call')


def check_options(options):
    """The `texture=` dict of the drivers: dict(texels=8, filter='bilinear', fill=(0, 0, 0), points_per_call=...) -> (bake keywords, filter).
    Raises before anything is computed."""
    if not isinstance(options, dict):
        raise TypeError(f'texture must be None or a dict of mesh_texture.bake arguments (texels, fill, points_per_call) and `filter`, got {type(options).__name__}')
    unknown = sorted(set(options) - set(OPTION_KEYS))
    if unknown:
        raise ValueError(f'texture: unknown keys {unknown}; known: {list(OPTION_KEYS)}')
    kw = {k: v for k, v in options.items() if k != 'filter'}
    kw.setdefault('texels', 8)
    atlas_layout(0, kw['texels'])
    if 'fill' in kw:
        _fill_bytes(kw['fill'])
    if 'points_per_call' in kw and int(kw['points_per_call']) < 1:
        raise ValueError(f'texture: points_per_call must be positive, got {kw["points_per_call"]!r}')
    filt = options.get('filter', 'bilinear')
    if filt not in FILTERS:
        raise ValueError(f'texture: filter must be one of {sorted(FILTERS)}, got {filt!r}')
    return kw, filt


@torch.no_grad()
def bake(vertices, triangles, colour_fn, texels=8, fill=(0, 0, 0), points_per_call=2 ** 22):
    """Bake the texture of one mesh (vertices [V,3] fp32, triangles [T,3] int32, on the device) -> Texture(image uint8 [H,W,3] on the device,
    uvs fp32 [T,3,2] (numpy, `atlas_uvs`), atlas).  `colour_fn(points [N,3])` -> fp32 [N, >=3] on the device in the renderer's range [-1, 1]
    (columns beyond the third are ignored); it is called on runs of at most min(points_per_call, FIELD_POINTS_MAX) texels, unowned ones
    (at the point 0) included, and must treat every point on its own: then the chunking does not change a byte.  `fill`: the three bytes of
    an unowned texel.  T == 0: a [0,0,3] image, nothing launched."""
    atlas_layout(0, texels)
    _fill_bytes(fill)
    if int(points_per_call) < 1:
        raise ValueError(f'points_per_call must be positive, got {points_per_call!r}')
    vertices, triangles = _mesh_surface._check_mesh(vertices, triangles)
    T = int(triangles.shape[0])
    atlas = atlas_layout(T, texels)
    image = torch.empty([atlas.height, atlas.width, 3], dtype=torch.uint8, device=vertices.device)
    N = atlas.width * atlas.height
    if N == 0:
        return Texture(image, atlas_uvs(T, atlas), atlas)
    points, owner = atlas_points(vertices, triangles, atlas)
    flat = image.view(N, 3)
    step = int(min(int(points_per_call), FIELD_POINTS_MAX))
    for i0 in range(0, N, step):
        p = points[i0:i0 + step]
        rgb = colour_fn(p)
        if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.float32 or rgb.ndim != 2 or rgb.shape[0] != p.shape[0] or rgb.shape[1] < 3:
            raise ValueError(f'colour_fn must return an fp32 [{p.shape[0]}, >=3] tensor, got {getattr(rgb, "dtype", type(rgb).__name__)} {tuple(getattr(rgb, "shape", ()))}')
        atlas_texels(rgb, owner[i0:i0 + step], flat[i0:i0 + step], fill)
    return Texture(image, atlas_uvs(T, atlas), atlas)          # on the host, while the device works through the launches above


def field_colour_fn(G, planes):
    """The field of one sample in coords mode as a `colour_fn`: points [N,3] in world units -> [N,4] (rgb in [-1, 1], sigma)."""
    point_field = _shapes.field_functions(G.synthesis)[1]
    return lambda p: point_field(planes, p.unsqueeze(0))[0]


@torch.no_grad()
def bake_field(G, planes, vertices, triangles, **kw):
    """`bake` with the field in coords mode: `planes` are the HWCPlanes of ONE sample, as `mesh.vertex_colours` takes them, and the vertices
    are in world units (`geometry.grid_to_world`).  kw: texels, fill, points_per_call."""
    return bake(vertices, triangles, field_colour_fn(G, planes), **kw)

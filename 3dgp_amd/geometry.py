"""Shape extraction (scripts/extract_geometry.py): the reference's voxel grid built on the device, densities evaluated in bounded slabs
through the field kernel, marching cubes as HIP kernels that leave an indexed mesh on the device, and the three file writers.

The reference materialises res^3 x 3 coordinates on the host, gets a [1, res^3, 4]-backed tensor back, copies the grid to the host and
hands it to `mcubes` / `trimesh` / `mrcfile`.  Here only the mesh (and, for .mrc, the cropped grid) crosses to the host.

Conventions of `marching_cubes` (csrc/geometry.hip, csrc/mc_table.inc): a corner is inside when its value is >= the threshold; vertices
are in index units of the volume, axis order (d, h, w) as `mcubes` returns them; every sign-changing grid edge carries ONE vertex, ordered by
the edge's lower grid point then axis; triangles are ordered by cell then table order and wound so that their normals point toward lower
density (read (d, h, w) as a right-handed (x, y, z): a blob of high density has positive signed volume).  PyMCubes' own vertex / triangle
ORDER is not reproduced.
"""
import collections
import struct

import numpy as np
import torch

from . import _lib
from . import renderer as _renderer

Shape = collections.namedtuple('Shape', ['vertices', 'triangles', 'sigma'])
TexturedShape = collections.namedtuple('TexturedShape', ['vertices', 'triangles', 'sigma', 'texture'])
OccludedShape = collections.namedtuple('OccludedShape', ['vertices', 'triangles', 'sigma', 'texture', 'occlusion'])


class MeshCount(tuple):
    """(vertices, triangles) of a finished mesh -- a plain pair to whoever unpacks or compares it -- with `.triangles_before`, the triangles it
    had before `simplify=` / `decimate=` (the same number without them), `.atlas`, the `mesh_texture.Atlas` of its texture (None without
    `texture=`), and `.decimate`, dict(rounds, stopped, triangles_before) of the `decimate=` stage (None without it)."""
    def __new__(cls, vertices, triangles, triangles_before=None):
        self = super().__new__(cls, (int(vertices), int(triangles)))
        self.atlas = None
        self.decimate = None
        self.triangles_before = int(triangles if triangles_before is None else triangles_before)
        return self
FIELD_POINTS_MAX = (2 ** 31 - 1) // 4          # points one tdgp_triplane_field call takes (csrc/field.hip)


def _grid_constants(resolution, voxel_origin, cube_size):
    """extract_geometry.py:58-59,72-74 in double, each rounded to fp32 once (a Python scalar meeting an fp32 tensor): voxel_size and
    the offsets of output columns (x, y, z) = voxel_origin[(2, 1, 0)] - cube_size / 2."""
    origin = np.array(voxel_origin, dtype=np.float64) - cube_size / 2.0
    voxel_size = cube_size / (resolution - 1)
    return float(voxel_size), float(origin[2]), float(origin[1]), float(origin[0])


def _voxel_coords_into(out, i0, resolution, consts):
    with torch.cuda.device(out.device):
        _lib.call('tdgp_voxel_coords', out.data_ptr(), int(i0), out.shape[0], int(resolution), *consts, _lib.stream_of(out))
    return out


def create_voxel_coords(resolution=256, voxel_origin=(0.0, 0.0, 0.0), cube_size=2.0, batch_size=1, device='cuda'):
    """extract_geometry.py:55-76 on the device, bit for bit (sheared grid and inexact index conversion included): [batch_size, resolution^3, 3]."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'create_voxel_coords builds the grid on the GPU (got device {device}); the HIP ops have no CPU path')
    out = torch.empty([int(resolution) ** 3, 3], dtype=torch.float32, device=device)
    _voxel_coords_into(out, 0, resolution, _grid_constants(resolution, voxel_origin, cube_size))
    return out.unsqueeze(0) if batch_size == 1 else out.repeat(batch_size, 1, 1)


@torch.no_grad()
def density_grid(G, ws, volume_res=256, voxel_origin=(0.0, 0.0, 0.0), cube_size=0.3, slab_points=2 ** 22, noise_mode='const'):
    """Raw sigma of `G.synthesis.compute_densities(ws, create_voxel_coords(volume_res, voxel_origin, cube_size))` as [B, res, res, res] fp32:
    the backbone runs once, then slabs of `slab_points` grid indices go through tdgp_voxel_coords and the field kernel (coords mode), and
    their sigma column is copied into the grid.  Temporaries are O(slab_points); the grid itself is the only O(res^3) tensor."""
    syn = G.synthesis
    _lib.require_cuda(ws, 'ws')
    planes = _renderer.planes_to_hwc(syn.tri_plane_decoder(ws[:, :syn.tri_plane_decoder.num_ws], hwc=True, noise_mode=noise_mode))
    return density_grid_from_planes(G, planes, volume_res, voxel_origin, cube_size, slab_points)


@torch.no_grad()
def density_grid_from_planes(G, planes, volume_res=256, voxel_origin=(0.0, 0.0, 0.0), cube_size=0.3, slab_points=2 ** 22):
    """`density_grid` behind the backbone: the same grid from the HWCPlanes the backbone returned, for callers that use those planes again
    (mesh.py renders field normals from them)."""
    syn = G.synthesis
    _lib.require_cuda(planes.t, 'planes')
    dev = planes.t.device
    res = int(volume_res)
    total = res ** 3
    slab = int(min(max(int(slab_points), 1), total, FIELD_POINTS_MAX))
    mlp, scale = syn.tri_plane_mlp, syn.cfg.cube_scale
    fused = _renderer.fused_form(mlp) or _renderer.deep_form(mlp)          # a field kernel evaluates it: two layers, or the deep form (3 / 4)
    params = (_renderer._mlp_params_deep(mlp) if _renderer.deep_form(mlp) else _renderer._mlp_params(mlp)) if fused else None
    consts = _grid_constants(res, voxel_origin, cube_size)
    B = planes.t.shape[0]
    grid = torch.empty([B, total], dtype=torch.float32, device=dev)
    coords = torch.empty([slab, 3], dtype=torch.float32, device=dev)
    for i0 in range(0, total, slab):
        n = min(slab, total - i0)
        c = _voxel_coords_into(coords[:n], i0, res, consts).unsqueeze(0)
        for b in range(B):
            pb = _renderer.HWCPlanes(planes.t[b:b + 1])
            rgbs = _renderer._field(pb, params, scale, coords=c) if fused else _renderer._field_eager(pb, mlp, scale, coords=c)
            grid[b, i0:i0 + n] = rgbs[0, :, -1]
    return grid.reshape(B, res, res, res)


def crop_reference(res):
    """The three slices of extract_geometry.py:33, `sigma[res//8:-res//8, res//2:, :-res//3]`, with Python's floor semantics for the
    negative bounds (`-res//8` is floor(-res / 8), not -(res // 8))."""
    res = int(res)
    return slice(res // 8, -res // 8), slice(res // 2, None), slice(None, -res // 3)


def marching_cubes(volume, thresh):
    """Marching cubes of a [D,H,W] volume at `thresh` on the device -> (vertices [V,3] fp32, triangles [T,3] int32), device tensors (module
    docstring for the conventions).  The only host read-back is the pair (V, T) that sizes the outputs."""
    _lib.require_cuda(volume, 'volume')
    if volume.ndim != 3:
        raise ValueError(f'marching_cubes takes a [D,H,W] volume, got {tuple(volume.shape)}')
    vol = _lib.f32c(volume)
    D, H, W = (int(s) for s in vol.shape)
    dev = vol.device
    empty = lambda: (torch.empty([0, 3], dtype=torch.float32, device=dev), torch.empty([0, 3], dtype=torch.int32, device=dev))   # noqa: E731
    if min(D, H, W) < 2:
        return empty()
    ws, need = _lib.byte_workspace('tdgp_mcubes_workspace_bytes', (D, H, W), dev, _lib.Unsupported(
        f'marching_cubes: a volume of {D}x{H}x{W} points exceeds the 2^31 - 1 this build indexes; extract it in parts'))
    with torch.cuda.device(dev):
        stream = _lib.stream_of(vol)
        _lib.call('tdgp_mcubes_count', vol.data_ptr(), D, H, W, float(thresh), ws.data_ptr(), need, stream)
        V, T = (int(x) for x in ws[:16].view(torch.int64).cpu())
        if V == 0 or T == 0:
            return empty()
        verts = torch.empty([V, 3], dtype=torch.float32, device=dev)
        tris = torch.empty([T, 3], dtype=torch.int32, device=dev)
        _lib.call('tdgp_mcubes_emit', vol.data_ptr(), D, H, W, float(thresh), ws.data_ptr(), need, verts.data_ptr(), V, tris.data_ptr(), T, stream)
    return verts, tris


def _crop_slices(crop, volume_res):
    """'reference' | None | three slices -> three slices or None."""
    if isinstance(crop, str):
        if crop != 'reference':
            raise ValueError("crop must be 'reference', None or three slices")
        return crop_reference(volume_res)
    if crop is None:
        return None
    crop = tuple(crop)
    if len(crop) != 3 or not all(isinstance(s, slice) for s in crop):
        raise ValueError("crop must be 'reference', None or three slices")
    return crop


@torch.no_grad()
def grid_to_world(vertices, volume_res, voxel_origin=(0.0, 0.0, 0.0), cube_size=0.3, crop='reference', sheared=True):
    """Mesh vertices in index units (d, h, w) of a CROPPED grid (`marching_cubes` of `sigma[crop]`) -> [V,3] fp32 world coordinates (x, y, z),
    the space `create_voxel_coords` samples and the cameras live in.  The start of each crop slice is added (`slice.indices`: Python's floor
    semantics for negative bounds), then the affine map whose values at integer grid indices are the points `create_voxel_coords` generates.
    That grid is sheared (extract_geometry.py:64-65: `(idx.float() / res) % res` keeps its fraction):
        x = (d + h / res + w / res^2) * voxel_size + origin_x,   y = (h + w / res) * voxel_size + origin_y,   z = w * voxel_size + origin_z
    with voxel_size and the origins as `_grid_constants` returns them, each rounded to fp32 as tdgp_voxel_coords takes them.  sheared=False
    drops the fractional terms: the plain lattice the reference's authors meant.  Computed in float64 on the vertices' device, rounded once."""
    res = int(volume_res)
    if res < 2:
        raise ValueError(f'volume_res must be at least 2, got {volume_res!r}')
    v = torch.as_tensor(vertices)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f'grid_to_world takes [V,3] vertices, got {tuple(v.shape)}')
    crop = _crop_slices(crop, res)
    starts = [0, 0, 0] if crop is None else [s.indices(res)[0] for s in crop]
    vs, ox, oy, oz = (float(np.float32(c)) for c in _grid_constants(res, voxel_origin, cube_size))
    v = v.to(torch.float64)
    d, h, w = (v[:, i] + float(starts[i]) for i in range(3))
    if sheared:
        x, y = d + h / res + w / (res * res), h + w / res
    else:
        x, y = d, h
    return torch.stack([x * vs + ox, y * vs + oy, w * vs + oz], dim=1).to(torch.float32)


@torch.no_grad()
def extract_geometry(G, ws, volume_res=256, voxel_origin=(0.0, 0.0, 0.0), cube_size=0.3, thresh_value=25.0, crop='reference', normalize=True,
                     slab_points=2 ** 22, noise_mode='const', units='index', sheared=True, components=None, smooth=None, simplify=None,
                     return_counts=False, texture=None, decimate=None, ao=None):
    """scripts/extract_geometry.py:26-42 per sample of `ws`: density grid -> crop -> marching cubes -> (optionally) scale.  Returns a list of
    Shape(vertices [V,3] fp32, triangles [T,3] int32, sigma [D,H,W] fp32 -- the cropped grid), all on the device.
    crop: 'reference' (extract_geometry.py:33), None, or three slices.  normalize: divide the vertices by the length of their bounding-box
    diagonal (`mesh.apply_scale(1.0 / mesh.scale)`, extract_geometry.py:42 -- trimesh's `scale`; no translation).
    units='world': the vertices go through `grid_to_world` with this call's volume_res / voxel_origin / cube_size / crop (and `sheared`)
    instead of `normalize` -- the mesh `mesh.render_mesh_views` takes.
    components, smooth, simplify, decimate, texture: the stages of `mesh_build.check_stages`, run on the marching-cubes output BEFORE it is scaled
    (`normalize` divides by the diagonal of the finished mesh; vertex normals are the caller's: `mesh_surface.vertex_normals` of the final
    vertices).  With texture= every item is a TexturedShape(vertices, triangles, sigma, texture) whose `texture` is a `mesh_texture.Texture`,
    baked on the `grid_to_world` vertices WHATEVER `units` returns.  return_counts=True: also a list of `MeshCount` per sample.
    ao: dict(rays=32, radius=None, bias=None): every item is an OccludedShape(vertices, triangles, sigma, texture or None, occlusion) whose
    `occlusion` is `mesh_rays.vertex_occlusion` of the finished mesh in world units (fp32 [V] in [0, 1]; `save_ply(colours=)` takes it as grey)."""
    if units not in ('index', 'world'):
        raise ValueError(f"units must be 'index' or 'world', got {units!r}")
    from . import mesh_build as _mesh_build          # the mesh modules behind it import this one
    stages = _mesh_build.check_stages(components, smooth, simplify, texture, decimate, ao)
    crop = _crop_slices(crop, volume_res)
    out, counts = [], []
    for b in range(ws.shape[0]):               # one sample's grid alive at a time, as the reference loops
        _lib.require_cuda(ws, 'ws')
        decoder = G.synthesis.tri_plane_decoder
        planes = _renderer.planes_to_hwc(decoder(ws[b:b + 1, :decoder.num_ws], hwc=True, noise_mode=noise_mode))
        m = _mesh_build.build_mesh(G, planes, stages, volume_res=volume_res, voxel_origin=voxel_origin, cube_size=cube_size, level=thresh_value,
                                   crop_slices=crop, sheared=sheared, slab_points=slab_points, keep_grid=True, world=units == 'world')
        verts = m.vertices
        if units == 'world':
            verts = m.world
        elif normalize and verts.shape[0] > 0:
            diag = (verts.max(dim=0).values - verts.min(dim=0).values).norm()
            if float(diag) > 0:
                verts = verts / diag
        counts.append(m.count)
        if m.occlusion is not None:
            out.append(OccludedShape(verts, m.triangles, m.sigma, m.texture, m.occlusion))
            continue
        out.append(Shape(verts, m.triangles, m.sigma) if m.texture is None else TexturedShape(verts, m.triangles, m.sigma, m.texture))
    return (out, counts) if return_counts else out


# ---- writers: host side, numpy only --------------------------------------------------------------------------------------------------

def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _check_normals(normals, v):
    n = _host(normals, '<f4')
    if n.shape != v.shape:
        raise ValueError(f'normals must be [V,3] like the vertices {v.shape}, got {n.shape}')
    return n


def save_obj(path, vertices, triangles, normals=None, uvs=None, texture=None):
    """Wavefront .obj: `v x y z` lines (shortest text that reads back as the same fp32) and 1-based `f a b c` lines.  normals [V,3]: `vn x y z`
    lines after the vertices (the same shortest text) and faces as `f a//a b//b c//c`.
    uvs [T,3,2] (`mesh_texture.atlas_uvs`: one pair per corner): `vt u v` lines (the same shortest text) after the vertices and normals, corner
    i of triangle t being vt 3t + i + 1, and faces as `f a/ta b/tb c/tc`, or `a/ta/na` with normals.  texture (needs uvs): a uint8 [H,W,3]
    image (or a `mesh_texture.Texture`, whose uvs are then the default) written with PIL as NAME.png next to NAME.obj, with NAME.mtl
    (`newmtl baked`, `Kd 1 1 1`, `map_Kd NAME.png`) and `mtllib NAME.mtl` / `usemtl baked` in the .obj.  uvs=None writes the bytes this
    function always wrote."""
    v, f = _host(vertices, np.float32).reshape(-1, 3), _host(triangles, np.int32).reshape(-1, 3)
    text = lambda x: np.format_float_positional(x, unique=True, trim='-')              # noqa: E731
    if texture is not None and hasattr(texture, 'image') and hasattr(texture, 'uvs'):
        uvs, texture = (texture.uvs if uvs is None else uvs), texture.image
    if uvs is not None:
        return _save_obj_uv(path, v, f, normals, uvs, texture, text)
    if texture is not None:
        raise ValueError('save_obj: a texture needs uvs (mesh_texture.atlas_uvs)')
    with open(path, 'w') as fh:
        fh.write(''.join(f'v {text(x)} {text(y)} {text(z)}\n' for x, y, z in v))
        if normals is None:
            fh.write(''.join(f'f {a + 1} {b + 1} {c + 1}\n' for a, b, c in f.tolist()))
        else:
            fh.write(''.join(f'vn {text(x)} {text(y)} {text(z)}\n' for x, y, z in _check_normals(normals, v)))
            fh.write(''.join(f'f {a + 1}//{a + 1} {b + 1}//{b + 1} {c + 1}//{c + 1}\n' for a, b, c in f.tolist()))


def _save_obj_uv(path, v, f, normals, uvs, image, text):
    """save_obj with texture coordinates (and the .mtl / .png pair when there is an image)."""
    import os
    uv = _host(uvs, np.float32)
    if uv.shape != (len(f), 3, 2):
        raise ValueError(f'uvs must be [T,3,2] for the {len(f)} triangles, got {uv.shape}')
    n = None if normals is None else _check_normals(normals, v)
    stem = os.path.splitext(os.path.basename(path))[0]
    if image is not None:
        from PIL import Image
        img = _host(image, np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f'texture must be a uint8 [H,W,3] image, got {img.shape}')
        if img.shape[0] == 0 or img.shape[1] == 0:
            raise ValueError('texture is empty (a mesh without triangles has no atlas): write the .obj without it')
        folder = os.path.dirname(path)
        Image.fromarray(img).save(os.path.join(folder, stem + '.png'))
        with open(os.path.join(folder, stem + '.mtl'), 'w') as fh:
            fh.write(f'newmtl baked\nKd 1 1 1\nmap_Kd {stem}.png\n')
    with open(path, 'w') as fh:
        if image is not None:
            fh.write(f'mtllib {stem}.mtl\n')
        fh.write(''.join(f'v {text(x)} {text(y)} {text(z)}\n' for x, y, z in v))
        if n is not None:
            fh.write(''.join(f'vn {text(x)} {text(y)} {text(z)}\n' for x, y, z in n))
        fh.write(''.join(f'vt {text(a)} {text(b)}\n' for a, b in uv.reshape(-1, 2)))
        if image is not None:
            fh.write('usemtl baked\n')
        if n is None:
            fh.write(''.join(f'f {a + 1}/{3 * t + 1} {b + 1}/{3 * t + 2} {c + 1}/{3 * t + 3}\n' for t, (a, b, c) in enumerate(f.tolist())))
        else:
            fh.write(''.join(f'f {a + 1}/{3 * t + 1}/{a + 1} {b + 1}/{3 * t + 2}/{b + 1} {c + 1}/{3 * t + 3}/{c + 1}\n' for t, (a, b, c) in enumerate(f.tolist())))


def save_ply(path, vertices, triangles, colours=None, normals=None):
    """Binary little-endian .ply: float32 x y z per vertex, then per face a uchar count (3) and three int32 indices.  colours [V,3] (uint8, or
    floating point in [0, 1]: clamped, scaled by 255 and rounded): `uchar red green blue` follow each vertex's coordinates.  normals [V,3]:
    `float nx ny nz` after x y z and before the colours."""
    v, f = _host(vertices, '<f4').reshape(-1, 3), _host(triangles, '<i4').reshape(-1, 3)
    rgb_props = ''
    nrm, n_props = (None, '') if normals is None else (_check_normals(normals, v), 'property float nx\nproperty float ny\nproperty float nz\n')
    if colours is not None:
        c = colours.detach().cpu().numpy() if isinstance(colours, torch.Tensor) else np.asarray(colours)
        if c.shape != v.shape:
            raise ValueError(f'colours must be [V,3] like the vertices {v.shape}, got {c.shape}')
        if c.dtype != np.uint8:
            c = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        rec = np.empty(len(v), dtype=[('p', '<f4', (3 if nrm is None else 6,)), ('c', 'u1', (3,))])
        rec['p'], rec['c'] = (v if nrm is None else np.concatenate([v, nrm], axis=1)), c
        v, rgb_props = rec, 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    elif nrm is not None:
        v = np.ascontiguousarray(np.concatenate([v, nrm], axis=1))
    header = ('ply\nformat binary_little_endian 1.0\n'
              f'element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n{n_props}{rgb_props}'
              f'element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n')
    faces = np.empty(len(f), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    faces['n'], faces['i'] = 3, f
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())


def save_mrc(path, volume):
    """MRC2014 map of a [D,H,W] fp32 volume, what `mrcfile.new_mmap(..., mrc_mode=2)` + `mrc.data[:] = sigma` leaves (extract_geometry.py:50-51):
    1024-byte header, mode 2, nx / ny / nz = W / H / D (x is the fastest axis), mx / my / mz and the unit cell equal to the dimensions
    (1 A voxels, 90 degree angles), mapc / mapr / maps = 1 / 2 / 3, dmin / dmax / dmean / rms filled in, ispg 1, nsymbt 0, nversion 20140,
    'MAP ' at byte 208, little-endian machine stamp 0x44 0x44 0 0, no labels, then the data.
    Written from the public format description (Cheng et al. 2015, J. Struct. Biol. 192:146); neither `mrcfile` nor ChimeraX was
    available to confirm that they read it."""
    vol = _host(volume, '<f4')
    if vol.ndim != 3:
        raise ValueError(f'save_mrc takes a [D,H,W] volume, got {vol.shape}')
    D, H, W = vol.shape
    hdr = bytearray(1024)
    v64 = vol.astype(np.float64)
    dmean = float(v64.mean()) if vol.size else 0.0
    rms = float(np.sqrt(((v64 - dmean) ** 2).mean())) if vol.size else 0.0
    struct.pack_into('<10i', hdr, 0, W, H, D, 2, 0, 0, 0, W, H, D)                  # nx ny nz mode nxstart nystart nzstart mx my mz
    struct.pack_into('<6f', hdr, 40, float(W), float(H), float(D), 90.0, 90.0, 90.0)    # cella, cellb
    struct.pack_into('<3i', hdr, 64, 1, 2, 3)                                       # mapc mapr maps
    struct.pack_into('<3f', hdr, 76, float(vol.min()) if vol.size else 0.0, float(vol.max()) if vol.size else 0.0, dmean)
    struct.pack_into('<2i', hdr, 88, 1, 0)                                          # ispg, nsymbt
    struct.pack_into('<i', hdr, 108, 20140)                                         # nversion
    hdr[208:212] = b'MAP '
    hdr[212:216] = bytes([0x44, 0x44, 0x00, 0x00])
    struct.pack_into('<f', hdr, 216, rms)
    struct.pack_into('<i', hdr, 220, 0)                                             # nlabl
    with open(path, 'wb') as fh:
        fh.write(bytes(hdr))
        fh.write(vol.tobytes())

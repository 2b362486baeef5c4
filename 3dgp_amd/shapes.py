"""Shape frames: iso-surface depth, normals and shading straight from the rays.

The reference shows geometry through a mesh (`scripts/extract_geometry.py` -> ChimeraX / Blender); `geometry.extract_geometry` is that route
here and pays volume_res^3 field evaluations per sample before a pixel exists.  This module renders the surface of a density level from the
cameras themselves: per ray S unjittered coarse depths, the first crossing of `level` (tdgp_iso_bracket), N refinement depths inside the
bracket and a linear interpolation of the crossing (tdgp_iso_locate), a 7-point stencil for the normal and a shade (tdgp_iso_shade) --
S + N + 7 field points per ray, on the planes the RGB frames of the same sample use (`SynthesisNetwork.tri_planes`).

`level` is RAW sigma, the quantity `geometry.density_grid` stores and `extract_geometry` thresholds: one number means the same surface on both
routes.  The arithmetic of the three kernels is fixed operation by operation (include/tdgp.h), so frames are the same bytes on every run and
under every chunking of the rays.  GPU only: the kernels have no CPU path.
"""
import ctypes

import torch

from . import _lib
from . import inference as _inference
from . import renderer as _renderer
from .generator import TensorGroup
from .geometry import FIELD_POINTS_MAX

MODES = {'shaded': 0, 'normals': 1, 'colour': 2}
MAX_STEPS, MAX_REFINE = 512, 64                 # tdgp_iso_bracket / tdgp_iso_locate (csrc/iso_surface.hip)
STENCIL = 7                                     # the hit point and +/- one step along each axis


# ----------------------------------------------------------------------------------------------------------------------
# the three kernels on tensors
# ----------------------------------------------------------------------------------------------------------------------
def _sigma_arg(sigma, rays, n, what):
    """(pointer, element stride) of a [rays, n] fp32 view whose elements sit at one uniform stride -- a contiguous tensor, or column 3 of the
    field kernels' rgbs (`rgbs.reshape(rays, n, 4)[..., 3]`), which is read in place."""
    _lib.require_cuda(sigma, what)
    if sigma.dtype != torch.float32 or tuple(sigma.shape) != (rays, n):
        raise ValueError(f'{what} must be fp32 [{rays}, {n}], got {sigma.dtype} {tuple(sigma.shape)}')
    if rays * n == 0:
        return sigma, 1
    es = sigma.stride(1) if n > 1 else (sigma.stride(0) if rays > 1 else 1)           # element i = ray * n + k sits at i * es
    if es < 1 or (n > 1 and rays > 1 and sigma.stride(0) != n * es):
        sigma, es = sigma.contiguous(), 1
    return sigma, es


def _vec3(v, what):
    v = [float(x) for x in v]
    if len(v) != 3:
        raise ValueError(f'{what} takes three numbers, got {v!r}')
    return (ctypes.c_float * 3)(*v)


def iso_bracket(sigma, t, num_refine, level):
    """tdgp_iso_bracket: sigma [rays,S] (see `_sigma_arg`), t [rays,S] ascending -> (idx int32 [rays], t_fine [rays,num_refine])."""
    _lib.require_cuda(t, 't')
    t = _lib.f32c(t)
    rays, S = t.shape
    sigma, es = _sigma_arg(sigma, rays, S, 'sigma')
    idx = torch.empty([rays], dtype=torch.int32, device=t.device)
    t_fine = torch.empty([rays, int(num_refine)], dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.call('tdgp_iso_bracket', sigma.data_ptr(), es, t.data_ptr(), rays, S, int(num_refine), float(level), idx.data_ptr(), t_fine.data_ptr(),
                  _lib.stream_of(t))
    return idx, t_fine


def iso_locate(sigma, t, idx, sigma_fine, t_fine, ray_o, ray_d, level, step, t_miss):
    """tdgp_iso_locate -> (t_hit [rays], status int32 [rays], points [rays,7,3])."""
    _lib.require_cuda(t, 't')
    t, t_fine, ray_o, ray_d = (_lib.f32c(x) for x in (t, t_fine, ray_o, ray_d))
    rays, S = t.shape
    N = t_fine.shape[1]
    sigma, es = _sigma_arg(sigma, rays, S, 'sigma')
    sigma_fine, esf = _sigma_arg(sigma_fine, rays, N, 'sigma_fine')
    if idx.dtype != torch.int32 or idx.numel() != rays or t_fine.shape[0] != rays or ray_o.numel() != rays * 3 or ray_d.numel() != rays * 3:
        raise ValueError(f'iso_locate: idx int32 [{rays}], t_fine [{rays}, N], ray_o / ray_d [{rays}, 3] expected')
    idx = idx.contiguous()
    t_hit = torch.empty([rays], dtype=torch.float32, device=t.device)
    status = torch.empty([rays], dtype=torch.int32, device=t.device)
    points = torch.empty([rays, STENCIL, 3], dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.call('tdgp_iso_locate', sigma.data_ptr(), es, t.data_ptr(), idx.data_ptr(), sigma_fine.data_ptr(), esf, t_fine.data_ptr(), ray_o.data_ptr(),
                  ray_d.data_ptr(), rays, S, N, float(level), float(step), float(t_miss), t_hit.data_ptr(), status.data_ptr(), points.data_ptr(),
                  _lib.stream_of(t))
    return t_hit, status, points


def iso_shade(stencil, status, ray_d, mode='shaded', light=None, ambient=0.2, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0), return_normal=True):
    """tdgp_iso_shade: stencil [rays,7,4] (the field's rgbs at iso_locate's points) -> (rgb [rays,3], normal [rays,3] or None)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    _lib.require_cuda(stencil, 'stencil')
    stencil, ray_d = _lib.f32c(stencil), _lib.f32c(ray_d)
    rays = status.numel()
    if stencil.numel() != rays * STENCIL * 4 or ray_d.numel() != rays * 3 or status.dtype != torch.int32:
        raise ValueError(f'iso_shade: stencil [{rays}, 7, 4], status int32 [{rays}], ray_d [{rays}, 3] expected')
    status = status.contiguous()
    rgb = torch.empty([rays, 3], dtype=torch.float32, device=stencil.device)
    normal = torch.empty([rays, 3], dtype=torch.float32, device=stencil.device) if return_normal else None
    with torch.cuda.device(stencil.device):
        _lib.call('tdgp_iso_shade', stencil.data_ptr(), status.data_ptr(), ray_d.data_ptr(), rays, MODES[mode], None if light is None else _vec3(light, 'light'),
                  float(ambient), _vec3(albedo, 'albedo'), _vec3(background, 'background'), rgb.data_ptr(), _lib.ptr(normal), _lib.stream_of(stencil))
    return rgb, normal


# ----------------------------------------------------------------------------------------------------------------------
# frames
# ----------------------------------------------------------------------------------------------------------------------
def _check_options(mode, num_steps, num_refine):
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if int(num_refine) != num_refine or not 1 <= int(num_refine) <= MAX_REFINE:
        raise ValueError(f'num_refine must be an integer in 1..{MAX_REFINE}, got {num_refine!r}')
    if int(num_steps) != num_steps or not 2 <= int(num_steps) <= MAX_STEPS:
        raise ValueError(f'num_steps must be an integer in 2..{MAX_STEPS}, got {num_steps!r}')


def field_functions(syn):
    """(ray_field(planes, ray_o, ray_d, t, ray_w), point_field(planes, coords)) -> rgbs [B,P,4], through the kernel `geometry.density_grid` would
    choose for this decoder: two layers -> tdgp_triplane_field, 3 / 4 layers -> the deep form, anything else the eager path."""
    mlp, scale = syn.tri_plane_mlp, syn.cfg.cube_scale
    deep = _renderer.deep_form(mlp)
    if _renderer.fused_form(mlp) or deep:
        params = _renderer._mlp_params_deep(mlp) if deep else _renderer._mlp_params(mlp)
        return (lambda p, o, d, t, w: _renderer._field(p, params, scale, ray_o=o, ray_d=d, t=t, ray_w=w),
                lambda p, c: _renderer._field(p, params, scale, coords=c))
    return (lambda p, o, d, t, w: _renderer._field_eager(p, mlp, scale, ray_o=o, ray_d=d, t=t),
            lambda p, c: _renderer._field_eager(p, mlp, scale, coords=c))


def coarse_depths(syn, rays, num_steps, device):
    """[rays, num_steps] unjittered coarse depths over cfg.ray_start .. cfg.ray_end: tdgp_sample_stratified with u = 0.5 everywhere (frames of a
    trajectory do not shimmer)."""
    cfg = syn.cfg
    u = torch.full([rays, num_steps], 0.5, dtype=torch.float32, device=device)
    sdist, tdist = torch.empty_like(u), torch.empty_like(u)
    with torch.cuda.device(device):
        _lib.call('tdgp_sample_stratified', u.data_ptr(), sdist.data_ptr(), tdist.data_ptr(), rays, num_steps, _renderer.MARCHER_IDS[cfg.ray_marcher_type],
                  float(cfg.ray_start), float(cfg.ray_end), _lib.stream_of(u))
    return tdist


@torch.no_grad()
def render_shape_views(G, planes, camera_params, level=25.0, mode='shaded', num_steps=None, num_refine=16, step=None, light=None, ambient=0.2,
                       albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0), max_rays_per_call=None):
    """V shape frames of each of B samples from that sample's planes (`G.synthesis.tri_planes`): the surface sigma == `level` as seen by the
    cameras (B * V of them, sample-major as in `render_views`).

    -> TensorGroup(rgb [B*V,R,3], depth [B*V,R,1], normal [B*V,R,3], status int32 [B*V,R]), ray-major, on the device.  status 1: the ray crosses
    the level, 2: the level is already met at the near plane, 0: a miss (rgb = background, normal = 0, depth = cfg.ray_end).  depth is the ray
    parameter of the hit.  mode: 'shaded' (Lambert, `albedo`), 'normals' (the unit normal as colour), 'colour' (the field's colour at the hit,
    shaded).  light: a unit vector toward the light, None = a headlight.  num_steps (default cfg.num_ray_steps) coarse and num_refine fine
    depths per ray; step: the normal's stencil step (default one tri-plane texel, 2 * cube_scale / tri_plane_res).
    Rays are taken `max_rays_per_call` at a time (default 16 images' worth; never more than the field kernel's points per call allow); they
    are independent, so the chunking does not change a byte.  Eval mode only."""
    syn, cfg = G.synthesis, G.cfg
    S = int(cfg.num_ray_steps) if num_steps is None else num_steps
    _check_options(mode, S, num_refine)
    S, N = int(S), int(num_refine)
    if syn.training:
        raise RuntimeError('render_shape_views is the inference route: call .eval() first (training mode renders patches with density noise)')
    if not isinstance(planes, _renderer.HWCPlanes):
        raise TypeError('render_shape_views takes the HWCPlanes that tri_planes returns')
    if max_rays_per_call is not None and int(max_rays_per_call) < 1:
        raise ValueError(f'max_rays_per_call must be positive, got {max_rays_per_call!r}')
    B, BV = int(planes.t.shape[0]), int(_renderer.cam_get(camera_params)('angles').shape[0])
    V = _renderer.views_per_sample(BV, B, f'plane batch {B} (sample-major: camera n * V + v is view v of sample n)')
    _lib.require_cuda(planes.t, 'planes')
    dev = planes.t.device
    h = w = syn.test_resolution
    R = h * w
    T = V * R                                                          # rays per sample: V frames of h rows of w rays
    step = 2.0 * float(cfg.cube_scale) / int(cfg.tri_plane_res) if step is None else float(step)
    ray_field, point_field = field_functions(syn)
    ray_o, ray_d = (x.reshape(B, T, 3) for x in _renderer.camera_rays(camera_params, (h, w)))
    # rays per call: the caller's bound, and the field kernel's points per call (the 7-point pass is the largest per ray when S < 7)
    max_rays = min(16 * R if max_rays_per_call is None else int(max_rays_per_call), FIELD_POINTS_MAX // max(S, N, STENCIL))
    if B * T <= max_rays:
        bstep, rstep = B, T
    elif max_rays >= B:
        bstep, rstep = B, min(T, max_rays // B)
    else:
        bstep, rstep = 1, min(T, max_rays)
    if w < rstep < T:
        rstep -= rstep % w                                             # whole image rows, so the ray-mode passes keep their tile walk
    out, t_coarse = _renderer.Gather(B, T), None
    for b0 in range(0, B, bstep):
        bs = slice(b0, min(b0 + bstep, B))
        nb = bs.stop - bs.start
        p_c = planes if nb == B else _renderer.HWCPlanes(planes.t[bs])
        for r0 in range(0, T, rstep):
            rs = slice(r0, min(r0 + rstep, T))
            n = rs.stop - rs.start
            rays = nb * n
            o, d = ray_o[bs, rs].contiguous(), ray_d[bs, rs].contiguous()
            ray_w = w if n % w == 0 else 0
            if t_coarse is None or t_coarse.shape[0] != rays:
                t_coarse = coarse_depths(syn, rays, S, dev)
            rgbs_c = ray_field(p_c, o, d, t_coarse.reshape(nb, n, S), ray_w)
            sig_c = rgbs_c.reshape(rays, S, 4)[..., 3]
            idx, t_fine = iso_bracket(sig_c, t_coarse, N, level)
            rgbs_f = ray_field(p_c, o, d, t_fine.reshape(nb, n, N), ray_w)
            t_hit, status, points = iso_locate(sig_c, t_coarse, idx, rgbs_f.reshape(rays, N, 4)[..., 3], t_fine, o, d, level, step, float(cfg.ray_end))
            stencil = point_field(p_c, points.reshape(nb, n * STENCIL, 3))
            rgb, normal = iso_shade(stencil, status, d, mode=mode, light=light, ambient=ambient, albedo=albedo, background=background)
            out.put(bs, rs, rgb=rgb.reshape(nb, n, 3), depth=t_hit.reshape(nb, n, 1), normal=normal.reshape(nb, n, 3), status=status.reshape(nb, n))
    rgb, depth, normal, status = out.result()
    return TensorGroup(rgb=rgb.reshape(BV, R, 3), depth=depth.reshape(BV, R, 1), normal=normal.reshape(BV, R, 3), status=status.reshape(BV, R))


def _shape_batches(G, ws, camera_params, plane_batch, **kw):
    """`tri_planes` on `plane_batch` samples at a time, `render_shape_views` on their cameras (the structure of inference._plane_batches)."""
    num_samples = len(ws)
    V = _renderer.views_per_sample(len(camera_params), num_samples, f'{num_samples} samples')
    if int(plane_batch) < 1:
        raise ValueError(f'plane_batch must be positive, got {plane_batch!r}')
    S = int(G.cfg.num_ray_steps) if kw.get('num_steps') is None else kw['num_steps']
    _check_options(kw.get('mode', 'shaded'), S, kw.get('num_refine', 16))
    if G.synthesis.training:
        raise RuntimeError('render_shapes is the inference route: call .eval() first (training mode renders patches with density noise)')
    camera_params = camera_params.to(dtype=torch.float32, device=ws.device)
    for n0 in range(0, num_samples, int(plane_batch)):
        n1 = min(n0 + int(plane_batch), num_samples)
        planes = G.synthesis.tri_planes(ws[n0:n1], noise_mode='const')
        yield render_shape_views(G, planes, camera_params[n0 * V:n1 * V], **kw)


def _all_frames(G, ws, camera_params, plane_batch, **kw):
    parts = list(_shape_batches(G, ws, camera_params, plane_batch, **kw))
    return parts[0] if len(parts) == 1 else TensorGroup.cat(parts, dim=0)


def render_shapes(G, ws, camera_params, plane_batch=4, return_all=False, **kw):
    """Shape frames of every `ws` under its cameras (sample-major), the tri-plane backbone run once per plane batch -> images [B*V,3,h,w]
    (tdgp_rays_to_image of the ray-major rgb); return_all=True: TensorGroup(img, depth [B*V,1,h,w], normal [B*V,3,h,w], status [B*V,h,w]).
    kw: the options of `render_shape_views`."""
    frames = _all_frames(G, ws, camera_params, plane_batch, **kw)
    h = w = G.synthesis.test_resolution
    BV = frames.rgb.shape[0]
    img = _renderer.rays_to_image(frames.rgb, h, w)
    if not return_all:
        return img
    return TensorGroup(img=img, depth=frames.depth.reshape(BV, 1, h, w), normal=_renderer.rays_to_image(frames.normal, h, w),
                       status=frames.status.reshape(BV, h, w))


def render_shape_video_grid(G, ws, camera_params, nrow='auto', show='rgb', plane_batch=4, num_videos=None, padding=2, as_numpy=False, **kw):
    """`inference.render_video_grid` of shape frames: frame t of the video is the make_grid of every sample's shape view t -> uint8
    [T, GH, GW, 3] on the device (as_numpy=True: one copy to the host).  show='depth': the hit depths, normalised by the ray range."""
    num_samples = len(ws)
    return _inference.video_grid_of(G, num_samples, len(camera_params) // max(num_samples, 1),
                                    lambda: _inference.shown(show, lambda: _all_frames(G, ws, camera_params, plane_batch, **kw)),
                                    nrow, num_videos, padding, show == 'depth', as_numpy)


def render_shape_strips(G, ws, camera_params, show='rgb', plane_batch=4, as_numpy=False, **kw):
    """`inference.render_image_strips` of shape frames: per sample, its shape views side by side -> uint8 [num_samples, h, V * w, 3] on the device."""
    num_samples = len(ws)
    return _inference.strips_of(G, num_samples, len(camera_params) // max(num_samples, 1),
                                lambda: _inference.shown(show, lambda: _all_frames(G, ws, camera_params, plane_batch, **kw)), show == 'depth', as_numpy)

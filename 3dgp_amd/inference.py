"""Inference harness around the generator forward.

Reference: `src/training/inference_utils.py:88-215` -- `generate`, `generate_trajectory`, `generate_camera_trajectory`,
`approximate_mean_camera_params`, `sample_posterior_camera_params`; `scripts/inference.py:87-150` -- `sample_z_from_seeds`,
`sample_c_from_seeds`, `c_idx_to_c`, `sample_ws_from_seeds`.  Host-side orchestration only: every frame is one
`G.synthesis` call on the HIP path; trajectories are a few hundred floats of tensor arithmetic kept on the CPU like the reference.

Trajectories of one sample share its tri-planes (`generate_trajectory(share_planes=True)`, `generate_videos`, `render_video_grid`,
`render_image_strips`: `SynthesisNetwork.tri_planes` once per sample, `render_views` for its cameras), and frames become uint8 grids on the
device (`frames_to_grid`, csrc/frames_grid.hip) -- DESIGN.md 5.11.
"""
import numpy as np
import torch

from . import _lib
from . import renderer as _renderer
from .generator import TensorGroup
from .metrics import camera_base, sample_camera_params


def _tg(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


def configure_for_inference(G, img_resolution, ray_step_multiplier, force_whiteback=False, far_plane_offset=0.0):
    """scripts/inference.py:38-48 on this package's `Generator`, in place: render at `img_resolution` (synthesis.img_resolution and
    synthesis.test_resolution), `cfg.num_ray_steps` multiplied by `ray_step_multiplier` (the coarse and the fine pass alike), a white
    background when `force_whiteback`, the far plane (`cfg.ray_end`) moved by `far_plane_offset`, no density noise.  Returns G.

    The eval forward renders up to renderer.MAX_STEPS (512) coarse + 512 fine samples per ray; a larger product is refused here, before
    anything is changed.  The differentiable forward (`forward_autograd`) keeps its own limit of renderer.MAX_GRAD_SAMPLES (256) merged
    samples per ray.  A `graphs.GraphedGenerator` captured BEFORE this call keeps the resolution and sample counts it was captured with
    (the kernels' arguments are frozen in the graph): capture a new one afterwards."""
    from .renderer import MAX_STEPS
    cfg, syn = G.cfg, G.synthesis
    if int(ray_step_multiplier) != ray_step_multiplier or ray_step_multiplier < 1:
        raise ValueError(f'ray_step_multiplier must be a positive integer, got {ray_step_multiplier!r}')
    steps = int(cfg.num_ray_steps) * int(ray_step_multiplier)
    if steps > MAX_STEPS:
        raise NotImplementedError(f'{cfg.num_ray_steps} ray steps x {ray_step_multiplier} = {steps} samples per ray and pass: the renderer takes at most '
                                  f'{MAX_STEPS} (beyond it torch\'s summation order of the pdf normaliser is not restated)')
    assert syn.cfg is cfg, 'G and G.synthesis share one configuration'
    syn.img_resolution = syn.test_resolution = int(img_resolution)
    cfg.num_ray_steps = steps
    if force_whiteback:
        cfg.white_back = True
    cfg.ray_end = cfg.ray_end + far_plane_offset
    syn.nerf_noise_std = 0.0
    return G


def generate(G, ws, camera_params, batch_size=8, **synthesis_kwargs):
    """inference_utils.py:107-126: frames for (ws[i], camera[i]) in chunks of `batch_size`, `noise_mode='const'`, mapped to
    [0, 1] on the CPU; depth (when requested) normalised to [-1, 1] by the ray range first."""
    frames = []
    for b0 in range(0, len(ws), batch_size):
        sl = slice(b0, b0 + batch_size)
        frame = G.synthesis(ws[sl], camera_params=camera_params[sl], noise_mode='const', **synthesis_kwargs)
        if isinstance(frame, TensorGroup) and 'depth' in frame:
            depth_range = G.cfg.ray_end - G.cfg.ray_start
            depth_mid = (G.cfg.ray_start + G.cfg.ray_end) * 0.5
            frame.depth = (frame.depth - depth_mid) / depth_range * 2.0
        frames.append(frame.clamp(-1, 1).cpu() * 0.5 + 0.5)             # a synchronisation point
        if ws.is_cuda:
            _lib.raise_on_device_fault('generate()')
    return TensorGroup.cat(frames, dim=0) if isinstance(frames[0], TensorGroup) else torch.cat(frames, dim=0)


def _plane_batches(G, ws, camera_params, plane_batch, u_coarse=None, u_fine=None, render_opts={}, max_rays_per_call=None, ray_major=False,
                   batch_size=None, **block_kwargs):
    """The shared-planes route: `tri_planes` on `plane_batch` samples at a time (block kwargs and noise_mode='const' go there), `render_views` on
    their cameras.  Yields what render_views returns, per plane batch, sample-major.  `batch_size` (the per-frame route's chunk) has no role here."""
    num_samples = len(ws)
    V = _renderer.views_per_sample(len(camera_params), num_samples, f'{num_samples} samples')
    if int(plane_batch) < 1:
        raise ValueError(f'plane_batch must be positive, got {plane_batch!r}')
    camera_params = camera_params.to(dtype=torch.float32, device=ws.device)
    syn = G.synthesis
    draws = _renderer.Draws(num_samples, V * syn.test_resolution ** 2, u_coarse, u_fine)
    for n0 in range(0, num_samples, int(plane_batch)):
        n1 = min(n0 + int(plane_batch), num_samples)
        planes = syn.tri_planes(ws[n0:n1], noise_mode='const', **block_kwargs)
        d = draws.take(slice(n0, n1)).opts()
        yield syn.render_views(planes, camera_params[n0 * V:n1 * V], ws=ws[n0:n1], render_opts=render_opts, u_coarse=d['u_coarse'], u_fine=d['u_fine'],
                               max_rays_per_call=max_rays_per_call, ray_major=ray_major)


def generate_trajectory(G, ws, camera_params, share_planes=False, plane_batch=4, **generate_kwargs):
    """inference_utils.py:88-103: every `ws` under every camera of its trajectory -> [num_cameras, num_samples, c, h, w].

    share_planes=False is the reference's structure: `ws` repeated per camera, the whole `G.synthesis` (tri-plane backbone included) once per
    frame.  share_planes=True runs the backbone once per SAMPLE (`SynthesisNetwork.tri_planes`, `plane_batch` samples at a time) and renders all
    cameras of those samples from their planes (`render_views`); same layout, same [0, 1] mapping, one host copy per plane batch."""
    num_cameras = len(camera_params) // len(ws)
    num_samples = len(camera_params) // num_cameras
    if share_planes:
        frames = []
        for frame in _plane_batches(G, ws, camera_params, plane_batch, **generate_kwargs):
            if isinstance(frame, TensorGroup) and 'depth' in frame:
                depth_range = G.cfg.ray_end - G.cfg.ray_start
                depth_mid = (G.cfg.ray_start + G.cfg.ray_end) * 0.5
                frame.depth = (frame.depth - depth_mid) / depth_range * 2.0
            frames.append(frame.clamp(-1, 1).cpu() * 0.5 + 0.5)         # a synchronisation point
            if ws.is_cuda:
                _lib.raise_on_device_fault('generate_trajectory()')
        images = TensorGroup.cat(frames, dim=0) if isinstance(frames[0], TensorGroup) else torch.cat(frames, dim=0)
    else:
        camera_params = camera_params.to(dtype=torch.float32, device=ws.device)
        ws = ws.repeat_interleave(num_cameras, dim=0)
        images = generate(G, ws=ws, camera_params=camera_params, **generate_kwargs)
    if isinstance(images, TensorGroup):
        images = images.reshape_each(lambda x: [num_samples, num_cameras, *x.shape[1:]])
    else:
        images = images.reshape(num_samples, num_cameras, *images.shape[1:])
    return images.permute(1, 0, 2, 3, 4)


def generate_camera_trajectory(trajectory, canonical_camera_params):
    """inference_utils.py:140-186: per canonical camera, the frames of a 'point' / 'front_circle' / 'points' / 'wiggle' / 'line'
    trajectory (all on the CPU); 'wiggle' raises, as it does in the reference."""
    name = _tg(trajectory, 'name')
    num_samples = len(canonical_camera_params)
    num_frames = len(_tg(trajectory, 'yaw_offsets')) if name == 'points' else _tg(trajectory, 'num_frames')
    cp = canonical_camera_params.repeat_interleave(num_frames, dim=0)
    if name == 'point':
        assert num_frames == 1
        angles = cp.angles.cpu() + torch.tensor([_tg(trajectory, 'yaw_offset'), _tg(trajectory, 'pitch_offset'), 0.0]).unsqueeze(0)
        fov = cp.fov.cpu() + _tg(trajectory, 'fov_offset')
    elif name == 'front_circle':
        steps = torch.linspace(0, 1, num_frames).repeat(num_samples)
        yaw = cp.angles[:, 0].cpu() + _tg(trajectory, 'yaw_diff') * torch.sin(steps * 2 * np.pi)
        pitch = cp.angles[:, 1].cpu() + _tg(trajectory, 'pitch_diff') * torch.cos(steps * 2 * np.pi)
        angles = torch.stack([yaw, pitch, cp.angles[:, 2].cpu()], dim=1)
        fov = cp.fov.cpu() + _tg(trajectory, 'fov_diff') * torch.sin(steps * 2 * np.pi)
    elif name == 'points':
        yaw = cp.angles[:, 0].cpu() + torch.tensor(_tg(trajectory, 'yaw_offsets')).repeat(num_samples)
        pitch = cp.angles[:, 1].cpu() + _tg(trajectory, 'pitch_offset')
        angles = torch.stack([yaw, pitch, cp.angles[:, 2].cpu()], dim=1)
        fov = cp.fov.cpu()
    elif name == 'wiggle':
        # inference_utils.py:167-170 builds numpy angles of length num_frames and fails TensorGroup's own type assertion
        raise NotImplementedError("the reference's 'wiggle' trajectory does not run (numpy angles in a TensorGroup, util.py:81)")
    elif name == 'line':
        yaws = torch.linspace(_tg(trajectory, 'yaw_start'), _tg(trajectory, 'yaw_end'), num_frames).repeat(num_samples)
        pitches = torch.linspace(_tg(trajectory, 'pitch_start'), _tg(trajectory, 'pitch_end'), num_frames).repeat(num_samples)
        angles = torch.stack([yaws, pitches, torch.zeros_like(yaws)], axis=1)
        fov = cp.fov.cpu() if _tg(trajectory, 'fov') is None else torch.ones_like(cp.fov.cpu()) * _tg(trajectory, 'fov')
    else:
        raise NotImplementedError(f'Unknown trajectory: {name}')
    return TensorGroup(angles=angles, fov=fov + _tg(trajectory, 'fov_offset', 0.0), radius=cp.radius.cpu(), look_at=cp.look_at.cpu())


def sample_posterior_camera_params(G, z, c, camera_cfg=None):
    """inference_utils.py:208-214: prior sample, passed through the camera adaptor when the generator has one."""
    prior = sample_camera_params(camera_base() if camera_cfg is None else camera_cfg, len(z), device=z.device)
    ca = getattr(G.synthesis, 'camera_adaptor', None)
    return prior if ca is None else ca(prior, z, c)


def approximate_mean_camera_params(G, num_samples=1024, device='cpu', camera_cfg=None, c_sampler=None):
    """inference_utils.py:196-204: Monte-Carlo mean of the (posterior) camera distribution, [1, ...]."""
    z = torch.randn(num_samples, G.z_dim, device=device)
    c = c_sampler(num_samples).to(device) if c_sampler is not None else torch.zeros(num_samples, G.c_dim, device=device)
    return sample_posterior_camera_params(G, z, c, camera_cfg).mean(dim=0, keepdim=True)


def get_mean_camera_params(G, device='cpu', camera_cfg=None):
    """inference_utils.py:182-191.  The 'custom' branch (dataset-provided angles) is taken where the mapping network carries
    `mean_camera_params` (yaw, pitch, roll, fov, radius); otherwise the Monte-Carlo mean of 1024 posterior samples.  [1, ...]."""
    m = getattr(G.mapping, 'mean_camera_params', None)
    if m is not None and m.numel() >= 5:
        m = m.to(device)
        return TensorGroup(angles=m[[0, 1, 2]].unsqueeze(0), fov=m[[3]], radius=m[[4]], look_at=torch.zeros(1, 3, device=device)).float()
    return approximate_mean_camera_params(G, num_samples=1024, device=device, camera_cfg=camera_cfg)


def generate_camera_params(G, z, c, trajectory, camera_cfg=None):
    """inference_utils.py:127-133: the canonical camera of every sample (the mean camera repeated with `use_mean_camera`, a posterior sample
    otherwise), then its trajectory -> [num_samples * num_frames, ...], sample-major."""
    if _tg(trajectory, 'use_mean_camera', False):
        canonical = get_mean_camera_params(G, device=z.device, camera_cfg=camera_cfg).repeat_interleave(len(z), dim=0)
    else:
        canonical = sample_posterior_camera_params(G, z, c, camera_cfg)
    return generate_camera_trajectory(trajectory, canonical_camera_params=canonical)


SNAPSHOT_TRAJECTORY = dict(name='front_circle', num_frames=32, fov_diff=1.0, yaw_diff=0.5, pitch_diff=0.3, use_mean_camera=True)


def generate_videos(G, z, c, gen_depths=False, plane_batch=4):
    """inference_utils.py:63-77, the training snapshots' videos: 9 (resolution >= 1024) or 16 samples under 32 `front_circle` frames around the
    mean camera -> TensorGroup(img [num_videos, 32, c, h, w], ...) in [0, 1] on the host.  Built on the shared-planes route (the reference's
    vis_cfg.batch_size = 4 is the plane batch here)."""
    num_videos = 9 if G.img_resolution >= 1024 else 16
    z, c = z[:num_videos], c[:num_videos]
    camera_params = generate_camera_params(G, z, c, SNAPSHOT_TRAJECTORY)
    ws = G.mapping(z, c)
    render_opts = dict(return_depth=gen_depths, return_depth_adapted=gen_depths)
    images = generate_trajectory(G, ws, camera_params, share_planes=True, plane_batch=plane_batch, render_opts=render_opts).permute(1, 0, 2, 3, 4)
    return images if isinstance(images, TensorGroup) else TensorGroup(img=images)


# ----------------------------------------------------------------------------------------------------------------------
# frames -> uint8 grids on the device (csrc/frames_grid.hip), video / image files
# ----------------------------------------------------------------------------------------------------------------------
def grid_shape(h, w, tiles, nrow, padding=2):
    """(GH, GW) of torchvision's make_grid(nrow, padding) over `tiles` images of h x w: xmaps = min(nrow, tiles), ymaps = ceil(tiles / xmaps),
    GH = (h + padding) * ymaps + padding, GW = (w + padding) * xmaps + padding; a single tile is returned as it is, unpadded."""
    for name, v, lo in (('h', h, 1), ('w', w, 1), ('tiles', tiles, 1), ('nrow', nrow, 1), ('padding', padding, 0)):
        if int(v) != v or v < lo:
            raise ValueError(f'{name} must be an integer >= {lo}, got {v!r}')
    if tiles == 1:
        return int(h), int(w)
    xmaps = min(int(nrow), int(tiles))
    ymaps = -(-int(tiles) // xmaps)
    return (int(h) + int(padding)) * ymaps + int(padding), (int(w) + int(padding)) * xmaps + int(padding)


def frames_to_grid(frames, h, w, tiles, images, stride_image, stride_tile, nrow, padding=2, normalise=None):
    """Ray-major fp32 frames [num_frames, h*w, C] (C in {1, 3}: the renderer's `rgb` / `depth` buffers, `render_views(ray_major=True)`) ->
    uint8 [images, GH, GW, 3] on the device, the [T,H,W,C] block a video or image encoder takes (tdgp_frames_to_grid_u8: one streaming kernel,
    no rays_to_image, no fp32 image, no host copy in between).  Tile k of image i shows frame i * stride_image + k * stride_tile: a video grid
    over V-frame trajectories is (images = V, tiles = samples, stride_image = 1, stride_tile = V), a strip of one sample's views
    (images = samples, tiles = V, stride_image = V, stride_tile = 1).  Layout: `grid_shape` (make_grid with pad_value 0; C = 1 is replicated).

    Values follow `generate` + `(x * 255).to(uint8)` as torch's CPU kernels evaluate them, each operation rounded once in fp32: with
    normalise = (mid, range) first y = ((x - mid) / range) * 2 (a true division), then clamp to [-1, 1], * 0.5 + 0.5, * 255, truncation; NaN
    gives 0.  (`generate` run on a GPU tensor multiplies by the reciprocal of `range` instead -- torch's GPU kernel for a division by a
    scalar -- which may move a depth value by an ulp; this function follows the CPU chain.)  GPU only; arguments are checked first."""
    GH, GW = grid_shape(h, w, tiles, nrow, padding)
    for name, v, lo in (('images', images, 1), ('stride_image', stride_image, 0), ('stride_tile', stride_tile, 0)):
        if int(v) != v or v < lo:
            raise ValueError(f'{name} must be an integer >= {lo}, got {v!r}')
    if not isinstance(frames, torch.Tensor) or frames.ndim != 3 or frames.shape[1] != h * w or frames.shape[2] not in (1, 3) or frames.shape[0] < 1:
        raise ValueError(f'frames must be a tensor [num_frames, h*w = {h * w}, 1 or 3], got {tuple(getattr(frames, "shape", ()))}')
    last = (images - 1) * stride_image + (tiles - 1) * stride_tile
    if last >= frames.shape[0]:
        raise ValueError(f'source frame index {last} (image {images - 1}, tile {tiles - 1}) is out of range: there are {frames.shape[0]} frames')
    if GH * GW * 3 >= 2 ** 31:
        raise ValueError(f'one {GH} x {GW} grid exceeds 2^31 bytes')
    if normalise is not None:
        mid, rng = (float(v) for v in normalise)
    else:
        mid, rng = 0.0, 1.0
    _lib.require_cuda(frames, 'frames')
    frames = _lib.f32c(frames)
    out = torch.empty([int(images), GH, GW, 3], dtype=torch.uint8, device=frames.device)
    with torch.cuda.device(frames.device):
        _lib.call('tdgp_frames_to_grid_u8', frames.data_ptr(), frames.shape[0], int(h), int(w), frames.shape[2], out.data_ptr(), int(images), int(tiles),
                  int(stride_image), int(stride_tile), int(nrow), int(padding), int(normalise is not None), mid, rng, _lib.stream_of(frames))
    return out


def _ray_major_frames(G, ws, camera_params, depth, plane_batch, **kwargs):
    """All frames of all samples, ray-major and sample-major on the device: rgb [num_samples * V, R, C] or depth [num_samples * V, R, 1]."""
    parts = [(out.depth if depth else out.rgb) for out in _plane_batches(G, ws, camera_params, plane_batch, ray_major=True, **kwargs)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def _depth_normalisation(G):
    return ((G.cfg.ray_start + G.cfg.ray_end) * 0.5, G.cfg.ray_end - G.cfg.ray_start)


def shown(show, make_all):
    """The buffer `show` names ('rgb' | 'depth') of the frames make_all() renders (a TensorGroup with both); `show` is checked first."""
    if show not in ('rgb', 'depth'):
        raise ValueError(f"show must be 'rgb' or 'depth', got {show!r}")
    frames = make_all()
    return frames.depth if show == 'depth' else frames.rgb


def video_grid_of(G, num_samples, V, make_frames, nrow, num_videos, padding, depth, as_numpy):
    """The tail of every video grid (pixels, shape frames, mesh frames): frame t is the make_grid of every sample's view t.  make_frames()
    renders the ray-major frames [num_samples * V, R, C], sample-major; it is called only after `grid_shape` has accepted the layout, so a bad
    nrow / padding is refused before anything is rendered.  depth: the frames are depths, shown normalised by the ray range."""
    if nrow == 'auto':
        nrow = int(np.ceil(min(num_samples if num_videos is None else num_videos, num_samples) ** 0.5))
    res = G.synthesis.test_resolution
    grid_shape(res, res, num_samples, nrow, padding)
    out = frames_to_grid(make_frames(), res, res, tiles=num_samples, images=V, stride_image=1, stride_tile=V, nrow=nrow, padding=padding,
                         normalise=_depth_normalisation(G) if depth else None)
    return _to_host(out) if as_numpy else out


def strips_of(G, num_samples, V, make_frames, depth, as_numpy):
    """The tail of every set of image strips: per sample, its V views side by side (make_frames, depth: as `video_grid_of`)."""
    res = G.synthesis.test_resolution
    out = frames_to_grid(make_frames(), res, res, tiles=V, images=num_samples, stride_image=V, stride_tile=1, nrow=V, padding=0,
                         normalise=_depth_normalisation(G) if depth else None)
    return _to_host(out) if as_numpy else out


def render_video_grid(G, ws, camera_params, nrow='auto', depth=False, plane_batch=4, num_videos=None, padding=2, as_numpy=False, **kwargs):
    """scripts/inference.py:68-75 (`video_grid`) on the device: frame t of the video is the make_grid of every sample's view t ->
    uint8 [T, GH, GW, 3] (a device tensor; as_numpy=True: one copy to the host).  Shared planes, ray-major buffers, `frames_to_grid`.
    nrow='auto' = ceil(sqrt(min(num_videos, num_samples))) as the reference script sets it (num_videos: its num_videos_per_grid, default all
    samples).  depth=True shows the depth maps, normalised by the ray range.  kwargs: render_opts, u_coarse, u_fine, max_rays_per_call, block kwargs."""
    num_samples = len(ws)
    return video_grid_of(G, num_samples, len(camera_params) // max(num_samples, 1),
                         lambda: _ray_major_frames(G, ws, camera_params, depth, plane_batch, **kwargs), nrow, num_videos, padding, depth, as_numpy)


def render_image_strips(G, ws, camera_params, depth=False, plane_batch=4, as_numpy=False, **kwargs):
    """scripts/inference.py:63-66 (`image_grid`): per sample, its views side by side (`torch.cat(list(images), dim=3)`) ->
    uint8 [num_samples, h, V * w, 3] on the device."""
    num_samples = len(ws)
    return strips_of(G, num_samples, len(camera_params) // max(num_samples, 1),
                     lambda: _ray_major_frames(G, ws, camera_params, depth, plane_batch, **kwargs), depth, as_numpy)


def _to_host(out):
    host = out.cpu().numpy()                                           # a synchronisation point
    _lib.raise_on_device_fault('frames_to_grid()')
    return host


def save_video(frames_u8, path, fps=25):
    """uint8 [T, H, W, 3] (device / host tensor or numpy) -> `path`, by extension: .gif through PIL exactly as scripts/inference.py:78-79 writes
    it; .png one grid (T == 1, or a single [H, W, 3] image); .npy the raw block; .mp4 through torchvision.io or PyAV when one of them is
    installed (h264, as scripts/inference.py:81) -- no encoder is vendored."""
    from PIL import Image
    x = _to_host(frames_u8) if isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda else np.asarray(frames_u8)
    if x.ndim == 3:
        x = x[None]
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[-1] != 3 or x.shape[0] < 1:
        raise ValueError(f'save_video takes uint8 [T, H, W, 3], got {x.dtype} {x.shape}')
    ext = str(path).rsplit('.', 1)[-1].lower()
    if ext == 'gif':
        frames = [Image.fromarray(f, 'RGB') for f in x]
        frames[0].save(path, quality=75, save_all=True, append_images=frames[1:], duration=1000 / fps, loop=0)
    elif ext == 'png':
        if x.shape[0] != 1:
            raise ValueError(f'.png holds one grid, got {x.shape[0]} frames (use .gif / .npy / .mp4)')
        Image.fromarray(x[0], 'RGB').save(path)
    elif ext == 'npy':
        np.save(path, x)
    elif ext == 'mp4':
        try:
            from torchvision.io import write_video
        except ImportError:
            write_video = None
        if write_video is not None:
            write_video(path, torch.from_numpy(x), fps=fps, video_codec='h264', options={'crf': '10'})
            return path
        try:
            import av
        except ImportError:
            raise RuntimeError('.mp4 needs an encoder: install PyAV (`av`) or torchvision (`torchvision.io`); neither imports here. '
                               '.gif, .png and .npy need nothing else') from None
        with av.open(path, mode='w') as container:
            stream = container.add_stream('h264', rate=int(fps))
            stream.height, stream.width, stream.pix_fmt = x.shape[1], x.shape[2], 'yuv420p'
            stream.options = {'crf': '10'}
            for f in x:
                for packet in stream.encode(av.VideoFrame.from_ndarray(f, format='rgb24')):
                    container.mux(packet)
            for packet in stream.encode():
                container.mux(packet)
    else:
        raise ValueError(f'unknown extension {ext!r}: .gif, .png, .npy or .mp4')
    return path


# ----------------------------------------------------------------------------------------------------------------------
# seeds -> (z, c) -> ws, scripts/inference.py:87-150
# ----------------------------------------------------------------------------------------------------------------------
def sample_z_from_seeds(seeds, z_dim):
    """scripts/inference.py:87-89: one `RandomState(seed).randn(1, z_dim)` row per seed (fp64 draw, cast to fp32)."""
    rows = [np.random.RandomState(s).randn(1, z_dim) for s in seeds]
    return torch.from_numpy(np.concatenate(rows, axis=0)).float()


def c_idx_to_c(c_idx, c_dim, device='cpu'):
    """scripts/inference.py:101-106: class indices -> one-hot rows [n, c_dim]."""
    idx = np.asarray(c_idx)
    c = np.zeros((len(idx), c_dim))
    c[np.arange(len(idx)), idx] = 1.0
    return torch.from_numpy(c).float().to(device)


def sample_c_from_seeds(seeds, c_dim, device='cpu'):
    """scripts/inference.py:93-97: the class of a seed is the first `choice` draw of its own RandomState."""
    if c_dim == 0:
        return torch.empty(len(seeds), 0)
    return c_idx_to_c([np.random.RandomState(s).choice(np.arange(c_dim), size=1).item() for s in seeds], c_dim, device)


def sample_ws_from_seeds(G, seeds, truncation_psi=1.0, device='cpu', num_interp_steps=0, classes=None, num_samples_to_avg=256):
    """scripts/inference.py:110-150 (`cfg.truncation_psi` passed as a number).

    num_interp_steps == 0: ws for every seed (x every class of `classes` when given).  With truncation_psi < 1 on a conditional
    generator the truncation centre is the PER-CLASS mean of `num_samples_to_avg` mapped samples (torch RNG on `device`), not
    `w_avg`.  Otherwise seeds are consumed pairwise and ws is `num_interp_steps` linear blends between the two ends."""
    if num_interp_steps == 0:
        z = sample_z_from_seeds(seeds, G.z_dim).to(device)
        c = sample_c_from_seeds(seeds, G.c_dim, device=device) if classes is None else c_idx_to_c(classes, G.c_dim, device)
        per_class_centre = truncation_psi < 1.0 and G.c_dim > 0
        if per_class_centre:
            z_avg = torch.randn(len(c) * num_samples_to_avg, G.z_dim, device=z.device)
            ws_avg = G.mapping(z_avg, c.repeat_interleave(num_samples_to_avg, dim=0))
            ws_avg = ws_avg.view(len(c), num_samples_to_avg, G.num_ws, ws_avg.shape[-1]).mean(dim=1)
            if classes is not None:
                ws_avg = ws_avg.repeat_interleave(len(seeds), dim=0)
        if classes is not None:                                            # class-major: every seed under class 0, then class 1, ...
            z = z.repeat(len(c), 1)
            c = c.repeat_interleave(len(seeds), dim=0)
        if per_class_centre:
            ws = G.mapping(z, c) * truncation_psi + ws_avg * (1 - truncation_psi)
        else:
            ws = G.mapping(z, c, truncation_psi=truncation_psi)
        return ws, z, c
    assert classes is None
    z_from, z_to = sample_z_from_seeds(seeds[0::2], G.z_dim).to(device), sample_z_from_seeds(seeds[1::2], G.z_dim).to(device)
    c_from, c_to = sample_c_from_seeds(seeds[0::2], G.c_dim, device=device), sample_c_from_seeds(seeds[1::2], G.c_dim, device=device)
    ws_from = G.mapping(z_from, c_from, truncation_psi=truncation_psi)
    ws_to = G.mapping(z_to, c_to, truncation_psi=truncation_psi)
    alpha = torch.linspace(0, 1, num_interp_steps, device=device).view(num_interp_steps, 1, 1, 1)
    return ws_from.unsqueeze(0) * (1 - alpha) + ws_to.unsqueeze(0) * alpha, (z_from, z_to), (c_from, c_to)

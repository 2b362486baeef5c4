"""Trajectory rendering on the GPU: tdgp_frames_to_grid_u8 bit for bit against a numpy restatement of its contract, tri-planes shared by the
views of a sample (`SynthesisNetwork.tri_planes` / `render_views`) bit for bit against per-view `G.synthesis` calls, and the harness on top
(`generate_trajectory(share_planes=True)`, `render_video_grid`, `render_image_strips`, `generate_videos`, `save_video`)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.as_tensor(a).to(DEV)


# ------------------------------------------------------------------------------------------------ the yardstick: numpy, written from the contract
def grid_shape_np(h, w, tiles, nrow, padding):
    if tiles == 1:
        return h, w, 1, 0
    xmaps = min(nrow, tiles)
    ymaps = -(-tiles // xmaps)
    return (h + padding) * ymaps + padding, (w + padding) * xmaps + padding, xmaps, padding


def bytes_np(x, normalise=None):
    """The value chain in numpy float32, one rounding per operation: ((x - mid) / range) * 2 when normalising, clamp to [-1, 1], * 0.5 + 0.5,
    * 255, truncation; NaN -> 0."""
    y = np.asarray(x, np.float32)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if normalise is not None:
            mid, rng = np.float32(normalise[0]), np.float32(normalise[1])
            y = ((y - mid) / rng).astype(np.float32) * np.float32(2.0)
        nan = np.isnan(y)
        y = np.where(nan, np.float32(0), np.minimum(np.maximum(y, np.float32(-1)), np.float32(1))).astype(np.float32)
        z = (y * np.float32(0.5)).astype(np.float32) + np.float32(0.5)
        b = np.trunc((z * np.float32(255.0)).astype(np.float32)).astype(np.uint8)
    return np.where(nan, np.uint8(0), b)


def grid_np(frames, h, w, tiles, images, stride_image, stride_tile, nrow, padding, normalise=None):
    frames = np.asarray(frames, np.float32)
    C = frames.shape[2]
    GH, GW, xmaps, pad = grid_shape_np(h, w, tiles, nrow, padding)
    out = np.zeros([images, GH, GW, 3], np.uint8)
    for i in range(images):
        for k in range(tiles):
            tile = bytes_np(frames[i * stride_image + k * stride_tile], normalise).reshape(h, w, C)
            y0, x0 = (k // xmaps) * (h + pad) + pad, (k % xmaps) * (w + pad) + pad
            out[i, y0:y0 + h, x0:x0 + w, :] = tile if C == 3 else np.repeat(tile, 3, axis=2)
    return out


def special_values():
    """+-1 and their neighbours, +-0, for every k the fp32 nearest 2k/255 - 1 and its two neighbours (the truncation boundaries), +-inf, NaN."""
    one = np.float32(1.0)
    v = [one, -one, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(-2)), np.nextafter(-one, np.float32(0)),
         np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
    for k in range(256):
        t = np.float32(2.0 * k / 255.0 - 1.0)
        v += [t, np.nextafter(t, np.float32(2)), np.nextafter(t, np.float32(-2))]
    return np.array(v, np.float32)


def make_frames(n, hw, C, seed, affine=None):
    """randn * 1.2 with the special values scattered over it (all of them when the tensor is large enough); affine = (mid, range): the
    values are carried to the depth domain so that the normalised chain meets the same boundaries."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(n, hw, C) * 1.2).astype(np.float32)
    sp = special_values()
    flat = x.reshape(-1)
    m = min(len(sp), flat.size)
    flat[rs.permutation(flat.size)[:m]] = sp[rs.permutation(len(sp))[:m]] if m < len(sp) else sp
    if affine is not None:
        with np.errstate(invalid='ignore'):
            x = (x * np.float32(affine[1] * 0.5) + np.float32(affine[0])).astype(np.float32)
    return x


GRID_CASES = dict(
    one_tile=dict(n=1, h=4, w=4, C=3, tiles=1, images=1, si=1, st=1, nrow=8, padding=2),
    ragged=dict(n=5, h=4, w=5, C=3, tiles=5, images=1, si=5, st=1, nrow=2, padding=2),
    strip_c1=dict(n=4, h=8, w=8, C=1, tiles=4, images=1, si=4, st=1, nrow=4, padding=0),
    video=dict(n=21, h=6, w=7, C=3, tiles=7, images=3, si=1, st=3, nrow=3, padding=2),
    strips=dict(n=21, h=6, w=7, C=3, tiles=7, images=3, si=7, st=1, nrow=3, padding=2),
    values=dict(n=4, h=16, w=20, C=3, tiles=4, images=1, si=4, st=1, nrow=2, padding=2),        # 3840 values: every special value is present
)


def _run_grid(tdgp, frames, c, normalise=None):
    out = tdgp.inference.frames_to_grid(T(frames), c['h'], c['w'], c['tiles'], c['images'], c['si'], c['st'], c['nrow'], c['padding'], normalise=normalise)
    torch.cuda.synchronize()
    return out


def _fill_allocator_with(byte, nbytes):
    """The next torch.empty of this size reuses this block: an output byte the kernel does not write shows as `byte`."""
    blk = torch.full([nbytes], byte, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    del blk


@pytest.mark.parametrize('name', list(GRID_CASES))
@pytest.mark.parametrize('mode', ['colour', 'depth'])
def test_frames_to_grid_bit_exact(tdgp, name, mode):
    """tdgp_frames_to_grid_u8 against the numpy restatement of its contract, whole buffers, byte for byte.  The output is written into a
    buffer pre-filled with 0xAA through the entry point itself (and the binding's own allocation reuses a block filled with 0xAA), so bytes
    the kernel leaves unwritten -- padding, ragged cells, the tail that is no whole dword -- show.  The yardstick's value chain is
    cross-checked against torch's CPU kernels."""
    c = GRID_CASES[name]
    normalise = (1.0, 0.5) if mode == 'depth' else None
    frames = make_frames(c['n'], c['h'] * c['w'], c['C'], seed=len(name), affine=normalise)
    if name == 'values':
        present = frames[~np.isnan(frames)]
        if mode == 'colour':
            assert all((present == v).any() for v in special_values() if not np.isnan(v)) and np.isnan(frames).any()
    want = grid_np(frames, c['h'], c['w'], c['tiles'], c['images'], c['si'], c['st'], c['nrow'], c['padding'], normalise)
    # the yardstick's chain vs torch CPU (non-NaN values; torch's cast of NaN is undefined)
    x = torch.from_numpy(frames)
    ok = ~torch.isnan(x)
    y = x if normalise is None else (x - normalise[0]) / normalise[1] * 2.0
    cpu = ((y.clamp(-1, 1) * 0.5 + 0.5) * 255).nan_to_num(0.0).to(torch.uint8)
    assert torch.equal(cpu[ok], torch.from_numpy(bytes_np(frames, normalise))[ok])
    assert (bytes_np(frames, normalise)[np.isnan(frames)] == 0).all()
    # through the entry point into a caller-owned, pre-filled buffer
    GH, GW, _, _ = grid_shape_np(c['h'], c['w'], c['tiles'], c['nrow'], c['padding'])
    assert tdgp.inference.grid_shape(c['h'], c['w'], c['tiles'], c['nrow'], c['padding']) == (GH, GW)
    fr = T(frames).contiguous()
    out = torch.full([c['images'], GH, GW, 3], 0xAA, dtype=torch.uint8, device=DEV)
    mid, rng = normalise if normalise is not None else (0.0, 1.0)
    tdgp._lib.call('tdgp_frames_to_grid_u8', fr.data_ptr(), fr.shape[0], c['h'], c['w'], c['C'], out.data_ptr(), c['images'], c['tiles'], c['si'], c['st'],
                   c['nrow'], c['padding'], int(normalise is not None), mid, rng, tdgp._lib.stream_of(fr))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), f'{int((got != want).sum())} of {want.size} bytes differ, first at {np.argwhere(got != want)[0]}'
    # the Python binding, twice: the same bytes on every run
    _fill_allocator_with(0xAA, want.size)
    a = _run_grid(tdgp, frames, c, normalise).cpu().numpy()
    b = _run_grid(tdgp, frames, c, normalise).cpu().numpy()
    assert a.dtype == np.uint8 and np.array_equal(a, want) and np.array_equal(b, want)


def test_frames_to_grid_beyond_4_gib(tdgp):
    """An output of more than 2^32 bytes takes the kernel's 64-bit index arithmetic (below that it divides in 32 bits): 1400 images of 16 tiles
    of 256^2, all showing the same 16 single-channel frames (stride_image = 0), so image 0 is checked against numpy and every other image
    against image 0 on the device."""
    h = w = 256
    tiles, images, nrow, padding = 16, 1400, 4, 2
    frames = make_frames(tiles, h * w, 1, seed=7)
    GH, GW, _, _ = grid_shape_np(h, w, tiles, nrow, padding)
    assert images * GH * GW * 3 > 2 ** 32
    fr = T(frames).contiguous()
    out = torch.full([images, GH, GW, 3], 0xAA, dtype=torch.uint8, device=DEV)
    tdgp._lib.call('tdgp_frames_to_grid_u8', fr.data_ptr(), tiles, h, w, 1, out.data_ptr(), images, tiles, 0, 1, nrow, padding, 0, 0.0, 1.0, tdgp._lib.stream_of(fr))
    torch.cuda.synchronize()
    want = grid_np(frames, h, w, tiles, 1, 0, 1, nrow, padding)
    assert np.array_equal(out[0].cpu().numpy(), want[0])
    for i in range(1, images, 200):
        assert bool((out[i:i + 200] == out[0]).all()), f'images {i}..{i + 199} differ from image 0'


def test_frames_to_grid_refuses_bad_arguments(tdgp):
    fr = torch.zeros(6, 20, 3, device=DEV)
    with pytest.raises(ValueError, match='out of range'):
        tdgp.inference.frames_to_grid(fr, 4, 5, tiles=3, images=2, stride_image=3, stride_tile=2, nrow=2)          # frame 3 + 4 = 7 >= 6
    out = torch.zeros(2, 14, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match='out of range'):                                                             # and the entry point itself
        tdgp._lib.call('tdgp_frames_to_grid_u8', fr.data_ptr(), 6, 4, 5, 3, out.data_ptr(), 2, 3, 3, 2, 2, 2, 0, 0.0, 1.0, tdgp._lib.stream_of(fr))
    with pytest.raises(RuntimeError, match='C must be 1 or 3'):
        tdgp._lib.call('tdgp_frames_to_grid_u8', fr.data_ptr(), 6, 4, 5, 2, out.data_ptr(), 1, 1, 1, 1, 1, 2, 0, 0.0, 1.0, tdgp._lib.stream_of(fr))
    with pytest.raises(RuntimeError, match='GPU'):
        tdgp.inference.frames_to_grid(fr.cpu(), 4, 5, tiles=3, images=2, stride_image=3, stride_tile=1, nrow=2)


# ------------------------------------------------------------------------------------------------ shared planes
V = 3            # the golden 'points' trajectory


@pytest.fixture(scope='module')
def scene(tdgp):
    """config_tiny, seeded weights, b = 2 samples, the 'points' trajectory, explicit draws, and the yardstick: per view v,
    G.synthesis(ws, cameras of view v) -- computed once at each resolution and left unchanged."""
    cfg = tdgp.config.config_tiny()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=21, exercise_all=True))
    G = G.to(DEV)
    inp = tdgp.weights.synthetic_inputs(cfg, batch=2, seed=9)
    ws = G.mapping(T(inp['z']), T(inp['c']))
    canon = tdgp.generator.TensorGroup(**{k: T(v) for k, v in inp['camera'].items()})
    cams = tdgp.inference.generate_camera_trajectory(tdgp.inference_golden_trajectories()['points'], canon).to(dtype=torch.float32, device=DEV)
    assert len(cams) == 2 * V
    out = {}
    for res in (cfg.img_resolution, 10):
        if res != cfg.img_resolution:
            tdgp.inference.configure_for_inference(G, res, 1)
        R, S = res * res, G.cfg.num_ray_steps
        gen = torch.Generator(device='cpu').manual_seed(res)
        u1, u2 = torch.rand(2 * V, R, S, generator=gen).to(DEV), torch.rand(2 * V * R, S, generator=gen).to(DEV)
        per_view = []
        for v in range(V):
            idx = torch.tensor([v, V + v], device=DEV)                                        # view v of sample 0 and of sample 1
            per_view.append(G.synthesis(ws, camera_params=cams[idx], noise_mode='const', render_opts=dict(return_depth=True),
                                        u_coarse=u1[idx], u_fine=u2.reshape(2 * V, R, S)[idx].reshape(2 * R, S)))
        img = torch.stack([p.img for p in per_view], dim=1).reshape(2 * V, *per_view[0].img.shape[1:])         # sample-major [b * V, ...]
        depth = torch.stack([p.depth for p in per_view], dim=1).reshape(2 * V, *per_view[0].depth.shape[1:])
        out[res] = dict(u1=u1, u2=u2, img=img.clone(), depth=depth.clone())
    return dict(G=G, ws=ws, cams=cams, native=cfg.img_resolution, **{f'r{k}': v for k, v in out.items()})


def _at(tdgp, scene, res):
    G = scene['G']
    if G.synthesis.test_resolution != res:
        G.synthesis.img_resolution = G.synthesis.test_resolution = res
    return G, scene[f'r{res}']


@pytest.mark.parametrize('res', ['native', 10])
@pytest.mark.parametrize('frames_per_call', [None, 1, 2, 4])
def test_render_views_equals_per_view_synthesis(tdgp, scene, res, frames_per_call):
    """render_views(tri_planes(ws), cameras) == G.synthesis(ws, cameras of view v) for every view v, torch.equal on img and depth: both sides
    run the backbone on the SAME batch of 2, hence on the same planes.  (Not compared against the repeated-ws batch of 6: the convolution launch
    plan may depend on the batch size, and equality across batch sizes is not claimed.)  At h = 10 -- no multiple of the field kernel's 4-row
    tiles -- frame boundaries fall inside tiles of the V * h-row image.  max_rays_per_call of one, two and four frames (one view of one
    sample; one view of both samples; 2 + 1 views of both samples) gives the same bits."""
    res = scene['native'] if res == 'native' else res
    G, y = _at(tdgp, scene, res)
    planes = G.synthesis.tri_planes(scene['ws'], noise_mode='const')
    assert isinstance(planes, tdgp.renderer.HWCPlanes) and planes.t.shape[0] == 2
    got = G.synthesis.render_views(planes, scene['cams'], render_opts=dict(return_depth=True), u_coarse=y['u1'], u_fine=y['u2'],
                                   max_rays_per_call=None if frames_per_call is None else frames_per_call * res * res)
    torch.cuda.synchronize()
    assert got.img.shape == (2 * V, 3, res, res) and got.depth.shape == (2 * V, 1, res, res)
    assert torch.equal(got.img, y['img']) and torch.equal(got.depth, y['depth'])
    rm = G.synthesis.render_views(planes, scene['cams'], u_coarse=y['u1'], u_fine=y['u2'], ray_major=True)
    assert rm.rgb.shape == (2 * V, res * res, 3) and rm.depth.shape == (2 * V, res * res, 1)
    assert torch.equal(rm.rgb.reshape(2 * V, res, res, 3).permute(0, 3, 1, 2), y['img']) and torch.equal(rm.depth.reshape(2 * V, 1, res, res), y['depth'])


def test_render_views_refusals(tdgp, scene):
    G, _ = _at(tdgp, scene, scene['native'])
    syn, ws, cams = G.synthesis, scene['ws'], scene['cams']
    planes = syn.tri_planes(ws, noise_mode='const')
    with pytest.raises(NotImplementedError, match='cut_quantile'):
        syn.render_views(planes, cams, render_opts=dict(cut_quantile=0.5))
    with pytest.raises(NotImplementedError, match='patch_params'):
        syn.render_views(planes, cams, patch_params=dict(scales=torch.ones(6, 2, device=DEV), offsets=torch.zeros(6, 2, device=DEV)))
    with pytest.raises(ValueError, match='multiple of the plane batch'):
        syn.render_views(planes, cams[:5])
    syn.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            syn.render_views(planes, cams)
        with pytest.raises(RuntimeError, match='eval'):
            syn.tri_planes(ws)
    finally:
        syn.eval()


# ------------------------------------------------------------------------------------------------ end to end
def test_generate_trajectory_share_planes(tdgp, scene):
    """Layout [V, b, c, h, w] and the [0, 1] mapping of `generate`, on the frames of the composition above; plane_batch = 1 runs the backbone
    on batches of 1 (other planes: not compared bit for bit), same layout and range."""
    G, y = _at(tdgp, scene, scene['native'])
    res = scene['native']
    fr = tdgp.inference.generate_trajectory(G, scene['ws'], scene['cams'], share_planes=True, plane_batch=2, render_opts=dict(return_depth=True),
                                            u_coarse=y['u1'], u_fine=y['u2'])
    assert fr.img.shape == (V, 2, 3, res, res) and fr.depth.shape == (V, 2, 1, res, res) and not fr.img.is_cuda
    img = (y['img'].clamp(-1, 1).cpu() * 0.5 + 0.5).reshape(2, V, 3, res, res).permute(1, 0, 2, 3, 4)
    mid, rng = (G.cfg.ray_start + G.cfg.ray_end) * 0.5, G.cfg.ray_end - G.cfg.ray_start
    dep = (((y['depth'] - mid) / rng * 2.0).clamp(-1, 1).cpu() * 0.5 + 0.5).reshape(2, V, 1, res, res).permute(1, 0, 2, 3, 4)
    assert torch.equal(fr.img, img) and torch.equal(fr.depth, dep)
    one = tdgp.inference.generate_trajectory(G, scene['ws'], scene['cams'], share_planes=True, plane_batch=1)
    assert one.shape == (V, 2, 3, res, res) and float(one.min()) >= 0.0 and float(one.max()) <= 1.0


@pytest.mark.parametrize('depth', [False, True])
def test_video_grid_and_image_strips(tdgp, scene, depth):
    """render_video_grid / render_image_strips == the numpy grid of the composition's frames, byte for byte (the ray-major depth with depth=True)."""
    G, y = _at(tdgp, scene, scene['native'])
    res = scene['native']
    if depth:
        frames = y['depth'].reshape(2 * V, res * res, 1).cpu().numpy()
        norm = ((G.cfg.ray_start + G.cfg.ray_end) * 0.5, G.cfg.ray_end - G.cfg.ray_start)
    else:
        frames = y['img'].permute(0, 2, 3, 1).reshape(2 * V, res * res, 3).cpu().numpy()
        norm = None
    kw = dict(depth=depth, plane_batch=2, u_coarse=y['u1'], u_fine=y['u2'])
    video = tdgp.inference.render_video_grid(G, scene['ws'], scene['cams'], **kw)
    assert video.is_cuda and video.dtype == torch.uint8
    want = grid_np(frames, res, res, tiles=2, images=V, stride_image=1, stride_tile=V, nrow=2, padding=2, normalise=norm)       # nrow 'auto' = ceil(sqrt(2))
    assert np.array_equal(video.cpu().numpy(), want)
    strips = tdgp.inference.render_image_strips(G, scene['ws'], scene['cams'], as_numpy=True, **kw)
    want = grid_np(frames, res, res, tiles=V, images=2, stride_image=V, stride_tile=1, nrow=V, padding=0, normalise=norm)
    assert isinstance(strips, np.ndarray) and strips.shape == (2, res, V * res, 3) and np.array_equal(strips, want)
    if not depth:                                        # scripts/inference.py:66: torch.cat(list(images), dim=3)
        imgs = y['img'].reshape(2, V, 3, res, res).permute(1, 0, 2, 3, 4).cpu()
        cat = torch.cat(list(imgs), dim=3)
        assert np.array_equal(strips, ((cat.clamp(-1, 1) * 0.5 + 0.5) * 255).to(torch.uint8).permute(0, 2, 3, 1).numpy())


def test_generate_videos_snapshot_shape(tdgp):
    """inference_utils.py:63-77 on a tiny configuration: 16 samples x 32 front_circle frames around the mean camera."""
    cfg = dataclasses.replace(tdgp.config.config_tiny(), img_resolution=8)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=5, exercise_all=True))
    G = G.to(DEV)
    torch.manual_seed(0)
    z, c = torch.randn(18, G.z_dim, device=DEV), torch.zeros(18, G.c_dim, device=DEV)
    if G.c_dim:
        c[:, 0] = 1.0
    vids = tdgp.inference.generate_videos(G, z, c)
    assert isinstance(vids, tdgp.generator.TensorGroup) and vids.img.shape == (16, 32, 3, 8, 8)
    assert float(vids.img.min()) >= 0.0 and float(vids.img.max()) <= 1.0 and bool(torch.isfinite(vids.img).all())


def test_save_video_files(tdgp, tmp_path, monkeypatch):
    from PIL import Image
    rs = np.random.RandomState(0)
    block = torch.from_numpy(rs.randint(0, 256, (5, 12, 14, 3)).astype(np.uint8)).to(DEV)
    tdgp.inference.save_video(block, str(tmp_path / 'v.gif'), fps=10)
    with Image.open(tmp_path / 'v.gif') as im:
        assert im.size == (14, 12) and getattr(im, 'n_frames', 1) == 5
    tdgp.inference.save_video(block[:1], str(tmp_path / 'g.png'))
    with Image.open(tmp_path / 'g.png') as im:
        assert np.array_equal(np.asarray(im.convert('RGB')), block[0].cpu().numpy())
    tdgp.inference.save_video(block, str(tmp_path / 'b.npy'))
    assert np.array_equal(np.load(tmp_path / 'b.npy'), block.cpu().numpy())
    with pytest.raises(ValueError, match='one grid'):
        tdgp.inference.save_video(block, str(tmp_path / 'many.png'))
    import sys
    for mod in ('av', 'torchvision', 'torchvision.io'):
        monkeypatch.setitem(sys.modules, mod, None)               # neither module imports
    with pytest.raises(RuntimeError, match='PyAV.*torchvision'):
        tdgp.inference.save_video(block, str(tmp_path / 'v.mp4'))
    assert not os.path.exists(tmp_path / 'v.mp4')

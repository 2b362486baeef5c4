"""Trajectory rendering, the parts that need no GPU: camera parameters of a trajectory, grid-shape arithmetic, argument validation of
`frames_to_grid` / `render_views` before any device call, the CLI's arguments."""
import importlib.util
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location('render_trajectory_cli', os.path.join(REPO, 'tools', 'render_trajectory.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _G(tdgp):
    return tdgp.generator.Generator(tdgp.config.config_tiny())


def test_generate_camera_params_mean_and_posterior(tdgp):
    """inference_utils.py:127-133: `use_mean_camera` repeats ONE canonical camera per sample before the trajectory is laid over it; without
    it the canonical cameras are `sample_posterior_camera_params` under the same seed."""
    I = tdgp.inference
    G = _G(tdgp)
    z, c = torch.randn(3, G.z_dim), torch.zeros(3, G.c_dim)
    traj = dict(tdgp.inference_golden_trajectories()['front_circle'], use_mean_camera=True)
    torch.manual_seed(3)
    np.random.seed(3)
    cams = I.generate_camera_params(G, z, c, traj)
    T = traj['num_frames']
    assert len(cams) == 3 * T and cams.angles.shape == (3 * T, 3) and cams.fov.shape == (3 * T,)
    for k in ('angles', 'fov', 'radius', 'look_at'):                       # sample-major, the same camera path for every sample
        per = cams[k].reshape(3, T, -1)
        assert torch.equal(per[0], per[1]) and torch.equal(per[0], per[2])
    torch.manual_seed(3)
    np.random.seed(3)
    mean = I.get_mean_camera_params(G, device='cpu')
    assert len(mean) == 1
    want = I.generate_camera_trajectory(traj, mean.repeat_interleave(3, dim=0))
    assert all(torch.equal(cams[k], want[k]) for k in want)
    # posterior cameras: one draw per sample
    traj = dict(traj, use_mean_camera=False)
    torch.manual_seed(5)
    np.random.seed(5)
    cams = I.generate_camera_params(G, z, c, traj)
    torch.manual_seed(5)
    np.random.seed(5)
    want = I.generate_camera_trajectory(traj, I.sample_posterior_camera_params(G, z, c))
    assert len(cams) == 3 * T and all(torch.equal(cams[k], want[k]) for k in want)


def test_mean_camera_custom_branch(tdgp):
    """inference_utils.py:183-189: a mapping network that carries `mean_camera_params` (yaw, pitch, roll, fov, radius) answers from them."""
    G = _G(tdgp)
    G.mapping.mean_camera_params = torch.tensor([0.1, 1.5, 0.0, 18.0, 2.7])
    m = tdgp.inference.get_mean_camera_params(G, device='cpu')
    assert torch.equal(m.angles, torch.tensor([[0.1, 1.5, 0.0]])) and torch.equal(m.fov, torch.tensor([18.0])) and torch.equal(m.radius, torch.tensor([2.7]))
    assert torch.equal(m.look_at, torch.zeros(1, 3)) and m.fov.dtype == torch.float32


def test_grid_shape_arithmetic(tdgp):
    gs = tdgp.inference.grid_shape
    assert gs(4, 4, 1, 8, 2) == (4, 4)                                  # one tile: unpadded
    assert gs(4, 5, 5, 2, 2) == (3 * 6 + 2, 2 * 7 + 2)                  # ragged last row
    assert gs(8, 8, 4, 4, 0) == (8, 32)                                 # strip
    assert gs(6, 7, 7, 3, 2) == (3 * 8 + 2, 3 * 9 + 2)
    assert gs(256, 256, 16, 4, 2) == (4 * 258 + 2, 4 * 258 + 2)
    assert gs(5, 5, 3, 8, 2) == (9, 3 * 7 + 2)                          # nrow above the tile count
    for bad in ((0, 4, 1, 1, 2), (4, 4, 0, 1, 2), (4, 4, 2, 0, 2), (4, 4, 2, 1, -1), (4.5, 4, 2, 1, 2)):
        with pytest.raises(ValueError):
            gs(*bad)


def test_frames_to_grid_validates_before_the_device(tdgp):
    f2g = tdgp.inference.frames_to_grid
    fr = torch.zeros(6, 20, 3)                                           # a CPU tensor: a valid request ends at the GPU requirement ...
    with pytest.raises(RuntimeError, match='GPU'):
        f2g(fr, 4, 5, tiles=3, images=2, stride_image=3, stride_tile=1, nrow=2)
    with pytest.raises(ValueError, match='out of range'):               # ... and an invalid one before it
        f2g(fr, 4, 5, tiles=3, images=2, stride_image=3, stride_tile=2, nrow=2)
    with pytest.raises(ValueError, match='frames must be'):
        f2g(fr, 4, 4, tiles=3, images=2, stride_image=3, stride_tile=1, nrow=2)
    with pytest.raises(ValueError, match='frames must be'):
        f2g(torch.zeros(6, 20, 2), 4, 5, tiles=3, images=2, stride_image=3, stride_tile=1, nrow=2)
    with pytest.raises(ValueError, match='nrow'):
        f2g(fr, 4, 5, tiles=3, images=2, stride_image=3, stride_tile=1, nrow=0)
    with pytest.raises(ValueError, match='stride_tile'):
        f2g(fr, 4, 5, tiles=3, images=2, stride_image=3, stride_tile=-1, nrow=2)
    with pytest.raises(ValueError, match='images'):
        f2g(fr, 4, 5, tiles=3, images=0, stride_image=3, stride_tile=1, nrow=2)


def test_render_views_validates_before_the_device(tdgp):
    G = _G(tdgp)
    syn = G.synthesis
    planes = tdgp.renderer.HWCPlanes(torch.zeros(2, 3, 4, 4, G.cfg.feat_dim))
    cams = tdgp.generator.TensorGroup(angles=torch.zeros(6, 3), fov=torch.full([6], 18.0), radius=torch.ones(6), look_at=torch.zeros(6, 3))
    with pytest.raises(NotImplementedError, match='cut_quantile'):
        syn.render_views(planes, cams, render_opts=dict(cut_quantile=0.5))
    with pytest.raises(NotImplementedError, match='patch_params'):
        syn.render_views(planes, cams, patch_params=dict(scales=torch.ones(6, 2), offsets=torch.zeros(6, 2)))
    with pytest.raises(ValueError, match='multiple of the plane batch'):
        syn.render_views(planes, cams[:5])
    with pytest.raises(ValueError, match='max_rays_per_call'):
        syn.render_views(planes, cams, max_rays_per_call=0)
    with pytest.raises(TypeError, match='HWCPlanes'):
        syn.render_views(torch.zeros(2, 3, 4, 4, 8), cams)
    syn.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            syn.render_views(planes, cams)
        with pytest.raises(RuntimeError, match='eval'):
            syn.tri_planes(torch.zeros(2, syn.num_ws, G.cfg.w_dim))
    finally:
        syn.eval()
    with pytest.raises(RuntimeError, match='GPU'):                       # a valid request on CPU tensors ends at the GPU requirement
        syn.render_views(planes, cams)
    with pytest.raises(ValueError, match='multiple'):
        list(tdgp.inference._plane_batches(G, torch.zeros(4, syn.num_ws, G.cfg.w_dim), cams, 2))


def test_save_video_refuses_what_it_cannot_write(tdgp, tmp_path):
    with pytest.raises(ValueError, match='uint8'):
        tdgp.inference.save_video(np.zeros((2, 4, 4, 3), np.float32), str(tmp_path / 'a.npy'))
    with pytest.raises(ValueError, match='extension'):
        tdgp.inference.save_video(np.zeros((2, 4, 4, 3), np.uint8), str(tmp_path / 'a.avi'))
    tdgp.inference.save_video(np.zeros((4, 6, 3), np.uint8), str(tmp_path / 'one.png'))                 # a single [H, W, 3] image
    assert os.path.getsize(tmp_path / 'one.png') > 0


def test_cli_arguments():
    cli = _cli()
    assert cli.parse_range('0-15') == list(range(16)) and cli.parse_range('1,4,7') == [1, 4, 7] and cli.parse_range('0-2,8') == [0, 1, 2, 8]
    a = cli.build_parser().parse_args(['--ckpt', 'd', '--seeds', '0-15', '--trajectory', 'front_circle', '--num-frames', '32', '--vis', 'video_grid',
                                       '--img-resolution', '256', '--ray-step-multiplier', '2', '--out', 'x.gif'])
    assert a.seeds == list(range(16)) and a.num_frames == 32 and a.vis == 'video_grid' and a.img_resolution == 256 and a.ray_step_multiplier == 2
    assert a.nrow == 'auto' and a.plane_batch == 4 and not a.depth
    t = cli.build_trajectory(a)
    assert t == dict(name='front_circle', num_frames=32, use_mean_camera=True, fov_offset=0.0, yaw_diff=0.5, pitch_diff=0.3, fov_diff=1.0)
    a = cli.build_parser().parse_args(['--ckpt', 'd', '--vis', 'image_grid', '--trajectory', 'points', '--yaw-offsets=-0.4,0,0.4', '--out', 'x.png'])
    assert cli.build_trajectory(a)['yaw_offsets'] == [-0.4, 0.0, 0.4] and a.vis == 'image_grid'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--ckpt', 'd', '--vis', 'movie', '--out', 'x.gif'])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--seeds', '0-3', '--out', 'x.gif'])                            # --ckpt is required

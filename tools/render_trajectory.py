#!/usr/bin/env python3
"""Render camera trajectories of generated samples into a video grid or image strips (the reference's scripts/inference.py): one JSON line.

    python tools/render_trajectory.py --ckpt exported_dir/ --seeds 0-15 --trajectory front_circle --num-frames 32 --vis video_grid \\
        --img-resolution 256 --ray-step-multiplier 2 --out grid.gif

`--ckpt` is a directory written by tools/export_reference_checkpoint.py.  `--vis video_grid`: frame t of the output shows every sample's view t
in a make_grid (`--nrow auto` = ceil(sqrt(samples))); write it as .gif, .npy or -- with PyAV or torchvision installed -- .mp4.  `--vis image_grid`:
one strip per sample, its views side by side; .png (the strips stacked into one image) or .npy.  The tri-plane backbone runs once per sample
(`--plane-batch` samples at a time), every frame is rendered from its sample's planes, and the frames become the uint8 grid on the device.
`--vis shape_grid` / `--vis shape_strips`: the same two layouts of SHAPE frames -- the surface where the raw density reaches `--level`, found on
the rays and shaded (`--shape-mode shaded | normals | colour`, `--num-refine`, `--ambient`, `--background`; `--depth` shows the hit depths).
`--vis mesh_grid` / `--vis mesh_strips`: the same layouts of MESH frames -- the surface extracted once per sample (`--volume-res`, `--cube-size`,
marching cubes at `--level`) and rasterised for every frame; `--mesh-normals face` shades the flat facets, `vertex` interpolates the mesh's own vertex normals, `field` takes the normals from the field;
`--mesh-smooth-iters N` Taubin-smooths every mesh on the device before it is drawn; `--mesh-simplify-cell X` then clusters its vertices in cells of
X voxels (quadric placement) and draws the simplified mesh; `--mesh-ao-rays N [--mesh-ao-radius R]` darkens each mesh by its per-vertex ambient occlusion (N rays per vertex); `--mesh-decimate-triangles N` collapses edges until at most N triangles are left
(the surface stays closed and of the same topology); `--mesh-texture-texels N` bakes a texture of N texels per triangle leg from the field
on every final mesh and draws the frames in colour mode from it (`--mesh-texture-filter nearest | bilinear`); `--mesh-samples 4 | 16` draws the
frames with 4 or 16 coverage samples per pixel (anti-aliased silhouettes; face or vertex normals).
"""
import argparse
import importlib
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_range(s):
    """'0-15', '1,4,7' or '0-3,8' -> list of ints (scripts/inference.py's seed syntax)."""
    out = []
    for part in str(s).split(','):
        m = re.fullmatch(r'\s*(\d+)\s*-\s*(\d+)\s*', part)
        if m:
            out.extend(range(int(m.group(1)), int(m.group(2)) + 1))
        elif part.strip():
            out.append(int(part))
    if not out:
        raise argparse.ArgumentTypeError(f'empty range {s!r}')
    return out


def build_trajectory(args):
    """The trajectory entries of configs/scripts/inference.yaml, from the command line."""
    t = dict(name=args.trajectory, num_frames=args.num_frames, use_mean_camera=not args.posterior_camera, fov_offset=args.fov_offset)
    if args.trajectory == 'front_circle':
        t.update(yaw_diff=args.yaw_diff, pitch_diff=args.pitch_diff, fov_diff=args.fov_diff)
    elif args.trajectory == 'points':
        t.update(yaw_offsets=[float(v) for v in args.yaw_offsets.split(',')], pitch_offset=args.pitch_offset)
    elif args.trajectory == 'point':
        t.update(num_frames=1, yaw_offset=args.yaw_offset, pitch_offset=args.pitch_offset)
    elif args.trajectory == 'line':
        t.update(yaw_start=args.yaw_start, yaw_end=args.yaw_end, pitch_start=args.pitch_start, pitch_end=args.pitch_end, fov=None)
    return t


class _Parser(argparse.ArgumentParser):
    """The surface options act on mesh frames alone: given with another --vis they are a usage error, not silently ignored."""
    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if not a.vis.startswith('mesh_') and (a.mesh_normals == 'vertex' or a.mesh_smooth_iters):
            self.error('--mesh-normals vertex and --mesh-smooth-iters need --vis mesh_grid or mesh_strips')
        if a.mesh_simplify_cell is not None:
            if not a.vis.startswith('mesh_'):
                self.error('--mesh-simplify-cell needs --vis mesh_grid or mesh_strips')
            if not 0 < a.mesh_simplify_cell < float('inf'):
                self.error(f'--mesh-simplify-cell takes a positive finite number, got {a.mesh_simplify_cell}')
        if a.mesh_decimate_triangles is not None:
            if not a.vis.startswith('mesh_'):
                self.error('--mesh-decimate-triangles needs --vis mesh_grid or mesh_strips')
            if a.mesh_decimate_triangles < 0:
                self.error(f'--mesh-decimate-triangles takes a non-negative integer, got {a.mesh_decimate_triangles}')
        if a.mesh_texture_texels is not None or a.mesh_texture_filter is not None:
            if not a.vis.startswith('mesh_'):
                self.error('--mesh-texture-texels and --mesh-texture-filter need --vis mesh_grid or mesh_strips')
            if a.mesh_texture_texels is None:
                self.error('--mesh-texture-filter needs --mesh-texture-texels')
            if not 2 <= a.mesh_texture_texels <= 64:
                self.error(f'--mesh-texture-texels takes an integer in [2, 64], got {a.mesh_texture_texels}')
            if a.mesh_normals == 'field':
                self.error('--mesh-texture-texels draws with face or vertex normals (--mesh-normals field takes its colour from the field)')
        if a.mesh_samples is not None:
            if not a.vis.startswith('mesh_'):
                self.error('--mesh-samples needs --vis mesh_grid or mesh_strips')
            if a.mesh_samples > 1 and a.mesh_normals == 'field':
                self.error('--mesh-samples 4 | 16 draws with face or vertex normals (--mesh-normals field is evaluated once per pixel)')
        if a.mesh_smooth_iters < 0:
            self.error(f'--mesh-smooth-iters takes a non-negative integer, got {a.mesh_smooth_iters}')
        if a.mesh_ao_rays is not None or a.mesh_ao_radius is not None:
            if not a.vis.startswith('mesh_'):
                self.error('--mesh-ao-rays and --mesh-ao-radius need --vis mesh_grid or mesh_strips')
            if a.mesh_ao_rays is None:
                self.error('--mesh-ao-radius needs --mesh-ao-rays')
            if a.mesh_ao_radius is not None and not a.mesh_ao_radius > 0:
                self.error(f'--mesh-ao-radius takes a positive number, got {a.mesh_ao_radius}')
            if a.mesh_normals == 'field' or a.mesh_texture_texels is not None or a.shape_mode == 'normals':
                self.error('--mesh-ao-rays darkens the shaded or coloured surface: it draws with face or vertex normals, without a texture, in --shape-mode shaded or colour')
        return a


def build_parser():
    p = _Parser(description=__doc__.split('\n')[0])
    p.add_argument('--ckpt', required=True, metavar='DIR', help='directory written by tools/export_reference_checkpoint.py')
    p.add_argument('--seeds', type=parse_range, default=parse_range('0-15'), help="e.g. '0-15' or '1,4,7'")
    p.add_argument('--classes', type=parse_range, default=None, help='class indices of a conditional generator (every seed under every class)')
    p.add_argument('--truncation-psi', type=float, default=1.0)
    p.add_argument('--trajectory', choices=['front_circle', 'points', 'point', 'line'], default='front_circle')
    p.add_argument('--num-frames', type=int, default=32)
    p.add_argument('--yaw-diff', type=float, default=0.5)
    p.add_argument('--pitch-diff', type=float, default=0.3)
    p.add_argument('--fov-diff', type=float, default=1.0)
    p.add_argument('--fov-offset', type=float, default=0.0)
    p.add_argument('--yaw-offsets', default='-0.5,0.0,0.5', help="the 'points' trajectory; write --yaw-offsets=-0.5,0,0.5 (a leading minus needs the '=')")
    p.add_argument('--yaw-offset', type=float, default=0.0)
    p.add_argument('--pitch-offset', type=float, default=0.0)
    p.add_argument('--yaw-start', type=float, default=-0.6)
    p.add_argument('--yaw-end', type=float, default=0.6)
    p.add_argument('--pitch-start', type=float, default=np.pi / 2)
    p.add_argument('--pitch-end', type=float, default=np.pi / 2)
    p.add_argument('--posterior-camera', action='store_true', help='a posterior camera sample per seed instead of the mean camera')
    p.add_argument('--vis', choices=['video_grid', 'image_grid', 'shape_grid', 'shape_strips', 'mesh_grid', 'mesh_strips'], default='video_grid')
    p.add_argument('--nrow', default='auto', help="'auto' or an integer (video_grid)")
    p.add_argument('--fps', type=float, default=25)
    p.add_argument('--depth', action='store_true', help='show the depth maps (normalised by the ray range) instead of the colours')
    p.add_argument('--level', type=float, default=25.0, help='shape frames: the raw density whose surface is shown (extract_geometry\'s thresh_value)')
    p.add_argument('--shape-mode', choices=['shaded', 'normals', 'colour'], default='shaded')
    p.add_argument('--num-refine', type=int, default=16, help='shape frames: refinement depths inside the bracket of the first crossing (1..64)')
    p.add_argument('--ambient', type=float, default=0.2, help='shape frames: ambient share of the shade')
    p.add_argument('--background', type=float, default=1.0, help='shape frames: grey level of the rays that miss, in [-1, 1]')
    p.add_argument('--volume-res', type=int, default=256, help='mesh frames: points per side of the density grid the mesh is extracted from')
    p.add_argument('--cube-size', type=float, default=None, help='mesh frames: side of the cube the grid spans (default: the whole field, 2 * cube_scale)')
    p.add_argument('--mesh-normals', choices=['face', 'field', 'vertex'], default='face',
                   help='mesh frames: flat facet normals, normals from the field at the hits, or interpolated vertex normals of the mesh')
    p.add_argument('--mesh-smooth-iters', type=int, default=0, metavar='N', help='mesh frames: Taubin-smooth each mesh, N lambda | mu iterations (default: none)')
    p.add_argument('--mesh-simplify-cell', type=float, default=None, metavar='X',
                   help='mesh frames: simplify each mesh on the device, one vertex per cell of X voxels, placed by its error quadric (default: none)')
    p.add_argument('--mesh-decimate-triangles', type=int, default=None, metavar='N',
                   help='mesh frames: collapse edges of each mesh on the device until at most N triangles are left; the surface stays closed (default: none)')
    p.add_argument('--mesh-texture-texels', type=int, default=None, metavar='N',
                   help='mesh frames: bake a texture of N texels per triangle leg (2..64) on each final mesh and draw it (implies --shape-mode colour; default: none)')
    p.add_argument('--mesh-texture-filter', choices=['nearest', 'bilinear'], default=None, help='mesh frames: how the texture is fetched (default bilinear)')
    p.add_argument('--mesh-samples', type=int, choices=[1, 4, 16], default=None, metavar='S',
                   help='mesh frames: coverage samples per pixel, 1 | 4 | 16 (default 1: one point sample at the pixel centre)')
    p.add_argument('--mesh-ao-rays', type=int, choices=[16, 32, 64], default=None, metavar='N',
                   help='mesh frames: ambient occlusion per vertex of each final mesh from N (16, 32 or 64) rays, multiplied into the surface colour (default: none)')
    p.add_argument('--mesh-ao-radius', type=float, default=None, metavar='R', help='mesh frames: how far an occluder counts, in world units (default: any distance)')
    p.add_argument('--keep-components', type=parse_keep, default=None, metavar='K',
                   help="mesh frames: draw only the K largest connected components of each mesh ('all': no limit; default: the raw level set)")
    p.add_argument('--component-by', choices=['triangles', 'area'], default='triangles', help='mesh frames: what "largest" measures')
    p.add_argument('--min-component-triangles', type=int, default=None, metavar='N', help='mesh frames: drop components with fewer than N triangles')
    p.add_argument('--img-resolution', type=int, default=None, help='default: the checkpoint\'s')
    p.add_argument('--ray-step-multiplier', type=int, default=1)
    p.add_argument('--force-whiteback', action='store_true')
    p.add_argument('--far-plane-offset', type=float, default=0.0)
    p.add_argument('--plane-batch', type=int, default=4, help='samples whose tri-planes are held at a time')
    p.add_argument('--seed', type=int, default=0, help='fixes the non-z randomness (stratified / importance draws, posterior cameras)')
    p.add_argument('--out', required=True, metavar='PATH', help='.gif / .npy / .mp4 (video_grid), .png / .npy (image_grid)')
    return p


def parse_keep(s):
    if s == 'all':
        return s
    k = int(s)
    if k < 1:
        raise argparse.ArgumentTypeError(f'--keep-components takes a positive integer or "all", got {s!r}')
    return k


def component_options(args):
    """The `components` argument of mesh.render_mesh_frames from the command line: None unless a flag asks for the filter."""
    if args.keep_components is None and args.min_component_triangles is None:
        return None
    return dict(keep='all' if args.keep_components is None else args.keep_components, by=args.component_by,
                min_triangles=args.min_component_triangles or 0)


def shape_options(args):
    """The options of shapes.render_shape_views, from the command line."""
    return dict(level=args.level, mode=args.shape_mode, num_refine=args.num_refine, ambient=args.ambient, background=(args.background,) * 3)


def mesh_options(args):
    """The options of mesh.render_mesh_frames, from the command line."""
    texture = None if args.mesh_texture_texels is None else dict(texels=args.mesh_texture_texels, filter=args.mesh_texture_filter or 'bilinear')
    return dict(level=args.level, volume_res=args.volume_res, cube_size=args.cube_size, mode='colour' if texture else args.shape_mode, normals=args.mesh_normals,
                ambient=args.ambient, background=(args.background,) * 3, plane_batch=args.plane_batch, components=component_options(args),
                smooth=dict(iterations=args.mesh_smooth_iters) if args.mesh_smooth_iters > 0 else None,
                simplify=dict(cell=args.mesh_simplify_cell) if args.mesh_simplify_cell is not None else None, **({'texture': texture} if texture else {}),
                **({'decimate': dict(target_triangles=args.mesh_decimate_triangles)} if args.mesh_decimate_triangles is not None else {}),
                **({'samples': args.mesh_samples} if (args.mesh_samples or 1) > 1 else {}),
                **({'ao': dict(rays=args.mesh_ao_rays, radius=args.mesh_ao_radius)} if args.mesh_ao_rays is not None else {}))


def main(argv=None):
    args = build_parser().parse_args(argv)
    nrow = args.nrow if args.nrow == 'auto' else int(args.nrow)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    tdgp = importlib.import_module('3dgp_amd')
    I = tdgp.inference
    cfg, sd = tdgp.weights.load_exported(args.ckpt)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(sd)
    G = G.to('cuda').eval()
    I.configure_for_inference(G, args.img_resolution or G.img_resolution, args.ray_step_multiplier, force_whiteback=args.force_whiteback,
                              far_plane_offset=args.far_plane_offset)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    t0 = time.perf_counter()
    with torch.no_grad():
        ws, z, c = I.sample_ws_from_seeds(G, args.seeds, truncation_psi=args.truncation_psi, device='cuda', classes=args.classes)
        cams = I.generate_camera_params(G, z, c, build_trajectory(args))
        show = 'depth' if args.depth else 'rgb'
        if args.vis == 'video_grid':
            block = I.render_video_grid(G, ws, cams, nrow=nrow, depth=args.depth, plane_batch=args.plane_batch, as_numpy=True)
        elif args.vis == 'shape_grid':
            block = tdgp.shapes.render_shape_video_grid(G, ws, cams, nrow=nrow, show=show, plane_batch=args.plane_batch, as_numpy=True, **shape_options(args))
        elif args.vis == 'mesh_grid':
            block, counts = tdgp.mesh.render_mesh_video_grid(G, ws, cams, nrow=nrow, show=show, as_numpy=True, return_counts=True, **mesh_options(args))
        else:
            if args.vis == 'mesh_strips':
                block, counts = tdgp.mesh.render_mesh_strips(G, ws, cams, show=show, as_numpy=True, return_counts=True, **mesh_options(args))
            elif args.vis == 'shape_strips':
                block = tdgp.shapes.render_shape_strips(G, ws, cams, show=show, plane_batch=args.plane_batch, as_numpy=True, **shape_options(args))
            else:
                block = I.render_image_strips(G, ws, cams, depth=args.depth, plane_batch=args.plane_batch, as_numpy=True)
            if not args.out.lower().endswith('.npy'):
                block = block.reshape(1, -1, *block.shape[2:])                  # the strips under each other: one image
    seconds = time.perf_counter() - t0
    I.save_video(block, args.out, fps=args.fps)
    line = dict(out=args.out, vis=args.vis, shape=list(block.shape), samples=len(ws), frames=len(cams) // len(ws), trajectory=args.trajectory,
                img_resolution=G.synthesis.test_resolution, ray_steps=G.cfg.num_ray_steps, depth=args.depth, seconds=seconds, ckpt=args.ckpt)
    if args.vis.startswith('shape_'):
        line.update(level=args.level, shape_mode=args.shape_mode, num_refine=args.num_refine)
    if args.vis.startswith('mesh_'):
        line.update(level=args.level, shape_mode=args.shape_mode, volume_res=args.volume_res, cube_size=args.cube_size, mesh_normals=args.mesh_normals,
                    vertices=[v for v, _ in counts], triangles=[t for _, t in counts], components=component_options(args),
                    mesh_smooth_iters=args.mesh_smooth_iters, mesh_simplify_cell=args.mesh_simplify_cell,
                    triangles_before_simplify=[c.triangles_before for c in counts], mesh_samples=args.mesh_samples or 1)
        if args.mesh_decimate_triangles is not None:
            line.update(mesh_decimate_triangles=args.mesh_decimate_triangles, decimate_rounds=[c.decimate['rounds'] for c in counts],
                        decimate_stopped=[c.decimate['stopped'] for c in counts])
        if args.mesh_ao_rays is not None:
            line.update(ao_rays=args.mesh_ao_rays, ao_radius=args.mesh_ao_radius)
        if args.mesh_texture_texels is not None:
            line.update(shape_mode='colour', mesh_texture_texels=args.mesh_texture_texels, mesh_texture_filter=args.mesh_texture_filter or 'bilinear',
                        atlas=[[c.atlas.width, c.atlas.height] for c in counts])
    print(json.dumps(line))


if __name__ == '__main__':
    main()

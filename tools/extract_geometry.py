#!/usr/bin/env python3
"""Extract shapes from a generator: density grid -> marching cubes on the GPU -> .mrc / .obj / .ply (scripts/extract_geometry.py).

    python tools/extract_geometry.py --ckpt exported_dir/ --seeds 0,1,5-7 --save-obj

`--ckpt` is a directory written by tools/export_reference_checkpoint.py.  The options carry the keys and defaults of the reference's
configs/scripts/extract_geometry.yaml; exactly one of --seeds / --num-seeds must be given.  Files are named `{seed:04d}` or, with
--classes, `c{class:04d}-s{seed:04d}`.  `num_ply_points` (unused by the reference script too) has no counterpart.
"""
import argparse
import importlib
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_range(s):
    """'1,2,5-7' -> [1, 2, 5, 6, 7] (scripts/inference.py:166-180)."""
    out = []
    for p in s.split(','):
        m = re.match(r'^(\d+)-(\d+)$', p)
        if m:
            out.extend(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.append(int(p))
    return out


def _flag(parser, name, default, help):
    parser.add_argument(f'--{name}', dest=name.replace('-', '_'), action=argparse.BooleanOptionalAction, default=default, help=help)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--seeds', type=parse_range, default=None, help="seeds, e.g. '0,1,5-7'")
    p.add_argument('--num-seeds', type=int, default=None, help='use seeds 0 .. N-1')
    p.add_argument('--classes', type=parse_range, default=None, help='class indices (conditional generators); every seed is extracted under every class')
    p.add_argument('--cube-size', type=float, default=0.3)
    p.add_argument('--volume-res', type=int, default=256)
    p.add_argument('--voxel-origin', type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=('X', 'Y', 'Z'))
    p.add_argument('--output-dir', default='shapes')
    p.add_argument('--thresh-value', type=float, default=25.0)
    p.add_argument('--truncation-psi', type=float, default=0.7)
    _flag(p, 'verbose', True, 'print one line per shape')
    _flag(p, 'save-mrc', True, 'write the cropped density grid as an MRC2014 map (for UCSF ChimeraX)')
    _flag(p, 'save-obj', False, 'write the mesh as Wavefront .obj')
    _flag(p, 'save-ply', False, 'write the mesh as binary .ply')
    p.add_argument('--ckpt', default=None, metavar='DIR', help='directory written by tools/export_reference_checkpoint.py')
    # the component filter is this project's own: its flags are absent from the namespace unless given (argparse.SUPPRESS), so the parsed
    # defaults stay exactly the keys of the reference's extract_geometry.yaml; component_options() reads them
    p.add_argument('--keep-components', type=parse_keep, default=argparse.SUPPRESS, metavar='K',
                   help="keep only the K largest connected components of the mesh ('all': no limit; default: the raw level set, floaters included)")
    p.add_argument('--component-by', choices=['triangles', 'area'], default=argparse.SUPPRESS, help='what "largest" measures (default: triangles)')
    p.add_argument('--min-component-triangles', type=int, default=argparse.SUPPRESS, metavar='N', help='drop components with fewer than N triangles')
    # so is the surface pass (mesh_surface.py): Taubin smoothing of the extracted mesh and vertex normals in the .obj / .ply
    p.add_argument('--smooth-iters', type=int, default=argparse.SUPPRESS, metavar='N', help='Taubin-smooth the mesh on the device: N lambda | mu iterations (default: none)')
    p.add_argument('--smooth-lambda', type=float, default=argparse.SUPPRESS, help='the shrinking step (default 0.5)')
    p.add_argument('--smooth-mu', type=float, default=argparse.SUPPRESS, help='the inflating step (default -0.53)')
    p.add_argument('--smooth-free-boundary', action='store_true', default=argparse.SUPPRESS, help='let the open rims (crop, grid boundary) move too')
    p.add_argument('--vertex-normals', action='store_true', default=argparse.SUPPRESS, help='write area-weighted vertex normals into the .obj / .ply')
    # and the simplification (mesh_simplify.py): vertex clustering with quadric placement, after the smoothing, cells in voxels
    p.add_argument('--simplify-cell', type=float, default=argparse.SUPPRESS, metavar='X', help='simplify the mesh on the device: one vertex per cell of X voxels (default: none)')
    p.add_argument('--simplify-max-triangles', type=int, default=argparse.SUPPRESS, metavar='N',
                   help='simplify with the first cell of the ladder 1, 1.41, 2, ... voxels that leaves at most N triangles')
    p.add_argument('--simplify-placement', choices=['quadric', 'mean'], default=argparse.SUPPRESS, help='where a cell puts its vertex (default quadric)')
    # and the decimation (mesh_decimate.py): quadric edge collapse that keeps the surface closed and of the same topology, after the simplification
    p.add_argument('--decimate-triangles', type=int, default=argparse.SUPPRESS, metavar='N', help='collapse edges on the device until at most N triangles are left (default: none)')
    p.add_argument('--decimate-max-error', type=float, default=argparse.SUPPRESS, metavar='E',
                   help='collapse edges while the RMS distance of a new vertex to the planes it stands for stays within E voxels (with --decimate-triangles: both hold)')
    # and the texture (mesh_texture.py): a per-triangle atlas baked from the field on the final mesh, written next to the .obj
    p.add_argument('--texture-texels', type=int, default=argparse.SUPPRESS, metavar='N',
                   help='bake a texture of N texels per triangle leg (2..64) and write NAME.obj with vt lines, NAME.mtl and NAME.png (needs --save-obj; default: none)')
    # and the distance report (mesh_distance.py): how far the simplified / decimated result is from the mesh it came from
    p.add_argument('--distance-report', action='store_true', default=argparse.SUPPRESS,
                   help='with simplification or decimation on: print the sampled two-sided surface distance (Hausdorff, mean, RMS) of the result to the unsimplified mesh')
    # and ambient occlusion (mesh_rays.py): per vertex of the finished mesh, as grey vertex colours of the .ply
    p.add_argument('--ao-rays', type=int, choices=[16, 32, 64], default=argparse.SUPPRESS, metavar='N',
                   help='cast N (16, 32 or 64) cosine-weighted rays per vertex of the finished mesh and write the unoccluded share as grey vertex colours (needs --save-ply; default: none)')
    return p


def parse_keep(s):
    if s == 'all':
        return s
    k = int(s)
    if k < 1:
        raise argparse.ArgumentTypeError(f'--keep-components takes a positive integer or "all", got {s!r}')
    return k


def component_options(args):
    """The `components` argument of geometry.extract_geometry / mesh.render_mesh_frames from the command line: None unless a flag asks for the filter."""
    keep, least = getattr(args, 'keep_components', None), getattr(args, 'min_component_triangles', None)
    if keep is None and least is None:
        return None
    return dict(keep='all' if keep is None else keep, by=getattr(args, 'component_by', 'triangles'), min_triangles=least or 0)


def smooth_options(args):
    """The `smooth` argument of geometry.extract_geometry / mesh.render_mesh_frames from the command line: None unless --smooth-iters asks for it."""
    iters = getattr(args, 'smooth_iters', None)
    if not iters:
        return None
    if iters < 0:
        raise SystemExit(f'--smooth-iters takes a non-negative integer, got {iters}')
    return dict(iterations=iters, lam=getattr(args, 'smooth_lambda', 0.5), mu=getattr(args, 'smooth_mu', -0.53),
                fix_boundary=not getattr(args, 'smooth_free_boundary', False))


def simplify_options(args):
    """The `simplify` argument of geometry.extract_geometry from the command line: None unless --simplify-cell or --simplify-max-triangles asks for it."""
    cell, most = getattr(args, 'simplify_cell', None), getattr(args, 'simplify_max_triangles', None)
    if cell is None and most is None:
        return None
    opts = dict(cell=cell) if cell is not None else dict(max_triangles=most)
    opts['placement'] = getattr(args, 'simplify_placement', 'quadric')
    return opts


def decimate_options(args):
    """The `decimate` argument of geometry.extract_geometry from the command line: None unless --decimate-triangles or --decimate-max-error asks for it."""
    most, err = getattr(args, 'decimate_triangles', None), getattr(args, 'decimate_max_error', None)
    if most is None and err is None:
        return None
    return {k: v for k, v in (('target_triangles', most), ('max_error', err)) if v is not None}


def texture_options(args):
    """The `texture` argument of geometry.extract_geometry from the command line: None unless --texture-texels asks for it."""
    texels = getattr(args, 'texture_texels', None)
    return None if texels is None else dict(texels=texels)


def ao_options(args):
    """The `ao` argument of geometry.extract_geometry from the command line: None unless --ao-rays asks for it."""
    rays = getattr(args, 'ao_rays', None)
    return None if rays is None else dict(rays=rays)


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if hasattr(args, 'ao_rays') and not args.save_ply:
        p.error('--ao-rays writes the occlusion as vertex colours of the .ply: it needs --save-ply (the .obj carries no vertex colours)')
    if hasattr(args, 'texture_texels'):
        if not 2 <= args.texture_texels <= 64:
            p.error(f'--texture-texels takes an integer in [2, 64], got {args.texture_texels}')
        if not args.save_obj:
            p.error('--texture-texels writes the texture next to the .obj: it needs --save-obj (a .ply carries no texture coordinates)')
    if hasattr(args, 'simplify_cell') and hasattr(args, 'simplify_max_triangles'):
        p.error('--simplify-cell and --simplify-max-triangles exclude each other')
    if hasattr(args, 'simplify_placement') and simplify_options(args) is None:
        p.error('--simplify-placement needs --simplify-cell or --simplify-max-triangles')
    if not 0 < getattr(args, 'simplify_cell', 1.0) < float('inf'):                  # false for NaN too
        p.error(f'--simplify-cell takes a positive finite number, got {args.simplify_cell}')
    if getattr(args, 'simplify_max_triangles', 0) < 0:
        p.error(f'--simplify-max-triangles takes a non-negative integer, got {args.simplify_max_triangles}')
    if getattr(args, 'decimate_triangles', 0) < 0:
        p.error(f'--decimate-triangles takes a non-negative integer, got {args.decimate_triangles}')
    if not 0 < getattr(args, 'decimate_max_error', 1.0) < float('inf'):             # false for NaN too
        p.error(f'--decimate-max-error takes a positive finite number, got {args.decimate_max_error}')
    if args.seeds is None and args.num_seeds is None:
        p.error('You must specify either `num_seeds` or `seeds`')
    if args.seeds is not None and args.num_seeds is not None:
        p.error('You cannot specify both `num_seeds` and `seeds`')
    return args


def sample_names(seeds, classes):
    return [f'{s:04d}' for s in seeds] if classes is None else [f'c{c:04d}-s{s:04d}' for c in classes for s in seeds]


def main(argv=None):
    args = parse_args(argv)
    if args.ckpt is None:
        raise SystemExit('--ckpt DIR is required (a directory written by tools/export_reference_checkpoint.py)')
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    tdgp = importlib.import_module('3dgp_amd')
    geometry = tdgp.geometry
    torch.manual_seed(42)                                       # set_seed(42): "to fix non-z randomization"
    seeds = args.seeds if args.num_seeds is None else list(range(args.num_seeds))
    cfg, sd = tdgp.weights.load_exported(args.ckpt)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(sd)
    G = G.to('cuda').eval()
    ws, _z, _c = tdgp.inference.sample_ws_from_seeds(G, seeds, truncation_psi=args.truncation_psi, device='cuda', classes=args.classes)
    names = sample_names(seeds, args.classes)
    os.makedirs(args.output_dir, exist_ok=True)
    need_mesh = args.save_obj or args.save_ply
    comp, smooth, with_normals = component_options(args), smooth_options(args), getattr(args, 'vertex_normals', False)
    simplify, texture, decimate, ao = simplify_options(args), texture_options(args), decimate_options(args), ao_options(args)
    for name, w in zip(names, ws.split(1, dim=0)):
        if need_mesh:
            shapes, counts = geometry.extract_geometry(G, w, volume_res=args.volume_res, voxel_origin=args.voxel_origin, cube_size=args.cube_size,
                                                       thresh_value=args.thresh_value, crop='reference', normalize=True, components=comp, smooth=smooth,
                                                       simplify=simplify, return_counts=True, **({} if texture is None else dict(texture=texture)),
                                                       **({} if decimate is None else dict(decimate=decimate)), **({} if ao is None else dict(ao=ao)))
            shape = shapes[0]
            sigma = shape.sigma
            normals = tdgp.mesh_surface.vertex_normals(shape.vertices, shape.triangles) if with_normals else None
            if args.save_obj:
                if texture is not None and shape.triangles.shape[0] > 0:
                    geometry.save_obj(os.path.join(args.output_dir, f'{name}.obj'), shape.vertices, shape.triangles, normals=normals, texture=shape.texture)
                else:
                    geometry.save_obj(os.path.join(args.output_dir, f'{name}.obj'), shape.vertices, shape.triangles, normals=normals)
            if args.save_ply:
                grey = {} if ao is None else dict(colours=shape.occlusion[:, None].expand(-1, 3))
                geometry.save_ply(os.path.join(args.output_dir, f'{name}.ply'), shape.vertices, shape.triangles, normals=normals, **grey)
            if args.verbose:
                print(f'{name}: {shape.vertices.shape[0]} vertices, {shape.triangles.shape[0]} triangles')
                if simplify is not None:
                    print(json.dumps(dict(name=name, simplify=simplify, vertices=counts[0][0], triangles=counts[0][1], triangles_before_simplify=counts[0].triangles_before)))
                if decimate is not None:
                    print(json.dumps(dict(name=name, decimate=decimate, vertices=counts[0][0], triangles=counts[0][1], triangles_before=counts[0].triangles_before,
                                          triangles_before_decimate=counts[0].decimate['triangles_before'], rounds=counts[0].decimate['rounds'],
                                          stopped=counts[0].decimate['stopped'])))
                if getattr(args, 'distance_report', False) and (simplify is not None or decimate is not None):
                    # one more extraction with everything but the simplification and the decimation: the mesh the result came from, same units
                    full = geometry.extract_geometry(G, w, volume_res=args.volume_res, voxel_origin=args.voxel_origin, cube_size=args.cube_size,
                                                     thresh_value=args.thresh_value, crop='reference', normalize=True, components=comp, smooth=smooth)[0]
                    d = tdgp.mesh_distance.mesh_distance(shape.vertices, shape.triangles, full.vertices, full.triangles)
                    print(json.dumps(dict(name=name, distance=dict(hausdorff=d.hausdorff, mean=d.mean, rms=d.rms, result_to_full_max=d.a_to_b.max,
                                                                   full_to_result_max=d.b_to_a.max, samples=[d.a_to_b.samples, d.b_to_a.samples]),
                                          triangles=int(shape.triangles.shape[0]), triangles_full=int(full.triangles.shape[0]))))
                if ao is not None:
                    occ = shape.occlusion
                    print(json.dumps(dict(name=name, ao_rays=ao['rays'], vertices=int(occ.shape[0]), occlusion_mean=float(occ.mean()) if occ.numel() else None,
                                          occlusion_min=float(occ.min()) if occ.numel() else None)))
                if texture is not None:
                    atlas = counts[0].atlas
                    print(json.dumps(dict(name=name, texture_texels=atlas.texels, atlas=[atlas.width, atlas.height], tiles_per_row=atlas.tiles_per_row,
                                          triangles=counts[0][1])))
                if comp is not None:
                    # the report measures the raw level set of the grid the shape was cut from (one more marching-cubes pass, verbose runs only)
                    raw_v, raw_t = geometry.marching_cubes(sigma, args.thresh_value)
                    if raw_v.shape[0]:
                        found = tdgp.mesh_components.components(raw_v, raw_t)
                        kept = int(tdgp.mesh_components.select(found, **comp).sum())
                        print(f'{name}: {found.triangles.shape[0]} components found, {kept} kept, '
                              f'{raw_t.shape[0] - shape.triangles.shape[0]} triangles dropped')
        else:
            sigma = geometry.density_grid(G, w, args.volume_res, args.voxel_origin, args.cube_size)[0][geometry.crop_reference(args.volume_res)]
            if args.verbose:
                print(f'{name}: density grid {tuple(sigma.shape)}')
        if args.save_mrc:
            geometry.save_mrc(os.path.join(args.output_dir, f'{name}.mrc'), sigma)


if __name__ == '__main__':
    main()

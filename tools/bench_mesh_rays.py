#!/usr/bin/env python3
"""Time the mesh rays on the GPU (mesh_rays.py); writes profiles/mesh_rays_bench.json.

    python tools/bench_mesh_rays.py [--config c3] [--volume-res 256] [--samples 16] [--reps 7] [--out profiles/mesh_rays_bench.json]

The scene and the mesh are those of tools/bench_mesh_distance.py (seeded weights, the level from the scene, the sample whose triangle count
is the median), in world units, and what `simplify(cell=2)` leaves of it.  Protocol of DESIGN.md 5.22 - 5.26: GPU time from events on the
launch stream, one warm-up, min / median / max over the repetitions.  Per mesh:
  build       `build_grid`
  camera      the rays of one --resolution^2 frame through `first_hits` and `occluded`: time, rays per second, triangles evaluated per ray, the
              share that hits; next to it the rasteriser's frame (`render_mesh_views`) and on how many pixels the two agree
  brute       the scan on a subsample of the rays, and whether it returns the bits of the walk
  occlusion   `vertex_occlusion` at 16 / 32 / 64 rays per vertex (grid and vertex normals given: the kernel alone), its mean
Nothing is asserted: this tool reports.
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decimate_bench():
    spec = importlib.util.spec_from_file_location('bench_mesh_decimate', os.path.join(REPO, 'tools', 'bench_mesh_decimate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='c3', help='generator configuration (tdgp.config.config_<name>)')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--volume-res', type=int, default=256)
    ap.add_argument('--resolution', type=int, default=256, help='side of the frame whose camera rays are cast')
    ap.add_argument('--cell', type=float, default=2.0, help='the second mesh is what simplify leaves at this cell (voxels)')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--brute-rays', type=int, default=4096, help='rays of the brute-force subsample')
    ap.add_argument('--commit', default=None, help='what the numbers were measured on (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mesh_rays_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_rays.py measures on a GPU; none found')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    B = _decimate_bench()
    I, Sh, S, M, Md, Me, Ms, g = tdgp.inference, tdgp.shapes, tdgp.mesh_simplify, tdgp.mesh_rays, tdgp.mesh_distance, tdgp.mesh, tdgp.mesh_surface, tdgp.geometry
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_mesh_rays] {msg}', file=sys.stderr, flush=True)              # noqa: E731
    cfg = getattr(tdgp.config, f'config_{args.config}')()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=0))
    G = G.to(dev).eval()
    syn = G.synthesis
    n, res, vol, side = args.samples, syn.test_resolution, args.volume_res, args.resolution
    R, Sr = res * res, int(cfg.num_ray_steps)
    box = 2.0 * float(cfg.cube_scale)
    inp = tdgp.weights.synthetic_inputs(cfg, batch=n, seed=1)
    z, c = torch.as_tensor(inp['z']).to(dev), torch.as_tensor(inp['c']).to(dev)
    torch.manual_seed(0)
    np.random.seed(0)
    ws = G.mapping(z, c)
    cams = I.generate_camera_params(G, z, c, dict(I.SNAPSHOT_TRAJECTORY, num_frames=1)).to(dtype=torch.float32, device=dev)
    ray_field = Sh.field_functions(syn)[0]
    o0, d0 = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cams[:1]), fov=cams.fov[:1], resolution=(res, res), device=dev)
    t0 = Sh.coarse_depths(syn, R, Sr, dev)
    counts, level = [], None
    for b in range(n):                                                                                # the median sample, as bench_mesh_decimate.py finds it
        planes = tdgp.renderer.HWCPlanes(syn.tri_planes(ws[b:b + 1], noise_mode='const').t)
        if level is None:
            level = float(ray_field(planes, o0, d0, t0.reshape(1, R, Sr), res).reshape(R, Sr, 4)[..., 3].max(dim=1).values.median())
        sigma = g.density_grid_from_planes(G, planes, vol, cube_size=box)[0]
        counts.append(int(g.marching_cubes(sigma, level)[1].shape[0]))
        del sigma, planes
    mid = sorted(range(n), key=lambda b: counts[b])[n // 2]
    planes = tdgp.renderer.HWCPlanes(syn.tri_planes(ws[mid:mid + 1], noise_mode='const').t)
    sigma = g.density_grid_from_planes(G, planes, vol, cube_size=box)[0]
    v, t = g.marching_cubes(sigma, level)
    del sigma
    s = S.simplify(v, t, args.cell)
    cam = cams[mid:mid + 1]
    ray_o, ray_d = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cam), fov=cam.fov, resolution=(side, side), device=dev)
    o, d = ray_o.reshape(-1, 3).contiguous(), ray_d.reshape(-1, 3).contiguous()
    N = int(o.shape[0])
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, commit=args.commit or B.commit_id(), config=args.config, samples=n, volume_res=vol,
               level=level, cube_size=box, sample=mid, units='world', resolution=side, rays=N, meshes={})

    def measure(fn, k=args.reps):
        fn()
        return B.stat([B.timed_device(fn) for _ in range(k)])

    for name, (mv, mt) in (('full', (v, t)), (f'simplify_cell_{args.cell:g}', (s.vertices, s.triangles))):
        world = g.grid_to_world(mv, vol, (0.0, 0.0, 0.0), box, None).contiguous()
        grid = Md.build_grid(world, mt)
        cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
        hits, evaluated = M.first_hits(o, d, grid, return_evaluated=True)
        frame = Me.render_mesh_views(world, mt, cam, side, G=G)
        cast_status = (hits.triangle >= 0).int()
        agree = (frame.status.reshape(-1) == cast_status) & (frame.tri.reshape(-1) == hits.triangle)
        first = measure(lambda: M.first_hits(o, d, grid))
        row = dict(vertices=int(mv.shape[0]), triangles=int(mt.shape[0]), build=measure(lambda: Md.build_grid(world, mt)),
                   grid=dict(cell=grid.cell, dims=list(grid.dims), cells=cells, pairs=int(grid.pair_triangle.shape[0])),
                   camera=dict(first_hits=first, rays_per_second=N / (first['ms_median'] * 1e-3), occluded=measure(lambda: M.occluded(o, d, grid)),
                               evaluated_per_ray=float(evaluated.double().mean()), evaluated_max=int(evaluated.max()), hit_share=float(cast_status.double().mean()),
                               rasteriser_frame=measure(lambda: Me.render_mesh_views(world, mt, cam, side, G=G)),
                               pixels_agreeing_with_the_rasteriser=float(agree.double().mean())))
        k = min(args.brute_rays, N)
        pick = torch.linspace(0, N - 1, k, device=dev).long()
        so, sd = o[pick].contiguous(), d[pick].contiguous()
        brute = M.first_hits(so, sd, grid, brute_force=True)
        row['brute'] = dict(measure(lambda: M.first_hits(so, sd, grid, brute_force=True), k=3), rays=k, walk_same_rays=measure(lambda: M.first_hits(so, sd, grid), k=3),
                            same_bits=bool(all(torch.equal(torch.nan_to_num(getattr(brute, f).double(), nan=-7.0), torch.nan_to_num(getattr(hits, f)[pick].double(), nan=-7.0))
                                               for f in brute._fields)))
        normals = Ms.vertex_normals(world, mt)
        row['occlusion'] = {}
        for rays in (16, 32, 64):
            ao = M.vertex_occlusion(world, mt, rays=rays, grid=grid, vertex_normals=normals)
            row['occlusion'][str(rays)] = dict(measure(lambda: M.vertex_occlusion(world, mt, rays=rays, grid=grid, vertex_normals=normals)), mean=float(ao.double().mean()),
                                               fully_open_share=float((ao == 1).double().mean()), same_twice=bool(torch.equal(ao, M.vertex_occlusion(world, mt, rays=rays, grid=grid, vertex_normals=normals))))
        say(f'{name}: {row["triangles"]} triangles, grid {grid.dims}; first_hits {first["ms_median"]:.3f} ms ({row["camera"]["rays_per_second"] / 1e6:.1f} M rays/s, '
            f'{row["camera"]["evaluated_per_ray"]:.1f} triangles per ray), rasteriser {row["camera"]["rasteriser_frame"]["ms_median"]:.3f} ms, agree on '
            f'{row["camera"]["pixels_agreeing_with_the_rasteriser"]:.4f}; scan of {k} rays {row["brute"]["ms_median"]:.1f} ms, same bits {row["brute"]["same_bits"]}; '
            f'occlusion 16 / 32 / 64: ' + ' / '.join(f'{row["occlusion"][str(r)]["ms_median"]:.2f}' for r in (16, 32, 64)) + ' ms')
        out['meshes'][name] = row
    tdgp._lib.raise_on_device_fault('bench_mesh_rays')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

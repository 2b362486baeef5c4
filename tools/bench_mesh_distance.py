#!/usr/bin/env python3
"""Time the mesh distance on the GPU (mesh_distance.py) and measure what simplification and decimation cost in distance;
writes profiles/mesh_distance_bench.json.

    python tools/bench_mesh_distance.py [--config c3] [--volume-res 256] [--samples 16] [--reps 7] [--out profiles/mesh_distance_bench.json]

The scene and the mesh are those of tools/bench_mesh_decimate.py (seeded weights, the level from the scene, the sample whose triangle count
is the median, index units = voxels); the meshes measured against it are what `simplify` leaves at cells 2 and 4 and what `decimate` leaves
at the same triangle counts.  Protocol of DESIGN.md 5.22 / 5.25: GPU time from events on the launch stream with the read-backs inside, one
warm-up, min / median / max over the repetitions.  Per result:
  build       `build_grid` of the full mesh and of the result: time, cells, pairs per cell and per triangle
  query       `sample_surface` + `one_sided` in each direction: time, samples, triangles evaluated per point
  total       `mesh_distance` (both grids, both sample sets, both queries)
  brute       the same query with brute_force=True on a subsample of the points small enough to finish, scaled to all of them: the
              yardstick the grid has to beat; the two agree bit for bit on the subsample
  distance    the two-sided maximum (sampled Hausdorff), RMS, mean and p99, next to the first-order figures of 5.25 at the result's vertices
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
    ap.add_argument('--cells', type=float, nargs='+', default=[2.0, 4.0], help='the targets are the triangle counts simplify leaves at these cells')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--brute-points', type=int, default=4096, help='points of the brute-force subsample')
    ap.add_argument('--commit', default=None, help='what the numbers were measured on (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mesh_distance_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_distance.py measures on a GPU; none found')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    B = _decimate_bench()
    I, Sh, S, Dm, M, g = tdgp.inference, tdgp.shapes, tdgp.mesh_simplify, tdgp.mesh_decimate, tdgp.mesh_distance, tdgp.geometry
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_mesh_distance] {msg}', file=sys.stderr, flush=True)              # noqa: E731
    cfg = getattr(tdgp.config, f'config_{args.config}')()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=0))
    G = G.to(dev).eval()
    syn = G.synthesis
    n, res, vol = args.samples, syn.test_resolution, args.volume_res
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
    nv, nt = int(v.shape[0]), int(t.shape[0])
    say(f'{vol}^3, sample {mid}: {nv} vertices, {nt} triangles')
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, commit=args.commit or B.commit_id(), config=args.config, samples=n, volume_res=vol,
               level=level, cube_size=box, sample=mid, vertices=nv, triangles=nt, units='index (voxels)', default_cell=M.default_cell(v, t))
    flip = B.level_distance(v, sigma, level, True)['rms_voxels'] <= B.level_distance(v, sigma, level, False)['rms_voxels']

    def measure(fn, k=args.reps):
        fn()
        return B.stat([B.timed_device(fn) for _ in range(k)])

    def grid_figures(grid):
        cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
        sizes = (grid.cell_start[1:] - grid.cell_start[:-1]).double()
        used = int((sizes > 0).sum())
        P = int(grid.pair_triangle.shape[0])
        return dict(cell=grid.cell, dims=list(grid.dims), cells=cells, cells_used=used, pairs=P, pairs_per_cell=P / max(cells, 1), pairs_per_used_cell=P / max(used, 1),
                    pairs_per_triangle=P / max(grid.valid_count, 1), longest_list=int(sizes.max()) if cells else 0)

    def direction(va, ta, grid):
        sm = M.sample_surface(va, ta)
        close, evaluated = M.closest_points(sm.points, grid, return_evaluated=True)
        S_ = int(sm.points.shape[0])
        row = dict(samples=S_, evaluated_per_point=float(evaluated.double().mean()) if S_ else 0.0, evaluated_max=int(evaluated.max()) if S_ else 0,
                   query=measure(lambda: M.one_sided(M.sample_surface(va, ta), grid)))
        k = min(args.brute_points, S_)
        if k:
            pick = torch.linspace(0, S_ - 1, k, device=dev).long()
            sub = sm.points[pick].contiguous()
            brute = M.closest_points(sub, grid, brute_force=True)
            row['brute'] = dict(measure(lambda: M.closest_points(sub, grid, brute_force=True), k=3), points=k,
                                same_bits=bool(torch.equal(brute.sqdist, close.sqdist[pick]) and torch.equal(brute.triangle, close.triangle[pick])))
            row['grid_same_points'] = measure(lambda: M.closest_points(sub, grid), k=3)
            row['brute_ms_scaled_to_all_points'] = row['brute']['ms_median'] * S_ / k
        nonzero = sm.weight > 0
        d = close.distance[nonzero]
        row['p99_unweighted'] = float(tdgp.renderer.quantile_select(d, 0.99)[2]) if d.numel() else None      # over the centroid samples, equal weights
        return row

    full_grid = M.build_grid(v, t)
    out['full'] = dict(build=measure(lambda: M.build_grid(v, t)), grid=grid_figures(full_grid))
    out['results'] = {}
    for cell in args.cells:
        s = S.simplify(v, t, cell)
        target = int(s.triangles.shape[0])
        d = Dm.decimate(v, t, target_triangles=target)
        for method, (rv, rt) in (('simplify', (s.vertices, s.triangles)), ('decimate', (d.vertices, d.triangles))):
            grid = M.build_grid(rv, rt)
            md = M.mesh_distance(rv, rt, v, t)
            row = dict(method=method, cell=cell, target_triangles=target, vertices=int(rv.shape[0]), triangles=int(rt.shape[0]),
                       build=measure(lambda: M.build_grid(rv, rt)), grid=grid_figures(grid), total=measure(lambda: M.mesh_distance(rv, rt, v, t)),
                       result_to_full=direction(rv, rt, full_grid), full_to_result=direction(v, t, grid),
                       distance=dict(hausdorff=md.hausdorff, mean=md.mean, rms=md.rms, result_to_full=dict(md.a_to_b._asdict()), full_to_result=dict(md.b_to_a._asdict())),
                       first_order_at_vertices=B.level_distance(rv, sigma, level, flip))
            again = M.mesh_distance(rv, rt, v, t)
            row['same_twice'] = bool(again == md)
            say(f'{method} to {row["triangles"]} triangles: total {row["total"]["ms_median"]:.2f} ms (build {row["build"]["ms_median"]:.2f} + {out["full"]["build"]["ms_median"]:.2f}); '
                f'hausdorff {md.hausdorff:.4f}, rms {md.rms:.4f} voxel; first order at the vertices: max {row["first_order_at_vertices"]["max_voxels"]:.3f}, rms '
                f'{row["first_order_at_vertices"]["rms_voxels"]:.4f}; evaluated per point {row["result_to_full"]["evaluated_per_point"]:.1f} / {row["full_to_result"]["evaluated_per_point"]:.1f}')
            out['results'][f'{method}_{target}'] = row
    tdgp._lib.raise_on_device_fault('bench_mesh_distance')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

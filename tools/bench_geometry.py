#!/usr/bin/env python3
"""Measure shape extraction on the GPU: backbone, density slabs, marching cubes (count / scan / emit per kernel) and the copies, next to what the
reference's route pays at least -- the device-to-host copy of the cropped fp32 grid a CPU marcher needs -- and the one-call
`compute_densities` on the full coordinate tensor with its peak allocation.

    python tools/bench_geometry.py [--config config_c3] [--volume-res 256] [--reps 9] [--out profiles/geometry_bench.json]

Times are medians over `--reps` runs after a warm-up: host clock around work that ends in a device synchronise for the stages, the
library's per-dispatch events (tdgp_profile_enable) for the marching-cubes kernels.  Weights are seeded random ones, so the threshold is taken
from the grid itself: its median (the densest surface a grid can carry -- the marcher's worst case) and its 90th percentile.  Needs a GPU;
there is no fallback.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='config_c3')
    ap.add_argument('--volume-res', type=int, default=256)
    ap.add_argument('--cube-size', type=float, default=0.3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'geometry_bench.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_geometry needs a GPU')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    geo, _lib = tdgp.geometry, tdgp._lib
    cfg = getattr(tdgp.config, args.config)()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=105, exercise_all=True))
    G = G.to('cuda').eval()
    inp = tdgp.weights.synthetic_inputs(cfg, batch=1, seed=106)
    ws = G.mapping(torch.as_tensor(inp['z']).cuda(), torch.as_tensor(inp['c']).cuda())
    res, cube = args.volume_res, args.cube_size
    sync = torch.cuda.synchronize

    def timed(fn, reps=args.reps, warm=2):
        for _ in range(warm):
            fn()
        out = []
        for _ in range(reps):
            sync()
            t0 = time.perf_counter()
            r = fn()
            sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), r

    def peak(fn):
        sync()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = fn()
        sync()
        p = torch.cuda.max_memory_allocated() - base
        del r
        return int(p)

    result = dict(config=args.config, volume_res=res, cube_size=cube, reps=args.reps, device=torch.cuda.get_device_name(0))
    syn = G.synthesis
    result['backbone_ms'], _ = timed(lambda: syn.tri_plane_decoder(ws[:, :syn.tri_plane_decoder.num_ws], hwc=True, noise_mode='const'))
    result['backbone_peak_bytes'] = peak(lambda: syn.tri_plane_decoder(ws[:, :syn.tri_plane_decoder.num_ws], hwc=True, noise_mode='const'))
    t_grid, grid = timed(lambda: geo.density_grid(G, ws, res, (0.0, 0.0, 0.0), cube))
    result['density_grid_ms'] = t_grid
    result['density_slabs_ms'] = t_grid - result['backbone_ms']
    result['density_grid_peak_bytes'] = peak(lambda: geo.density_grid(G, ws, res, (0.0, 0.0, 0.0), cube))

    def parent_style():
        coords = geo.create_voxel_coords(res, (0.0, 0.0, 0.0), cube, 1)
        return syn.compute_densities(ws, coords, noise_mode='const')
    result['compute_densities_full_ms'], whole = timed(parent_style, reps=max(3, args.reps // 3), warm=1)
    result['density_grid_equals_compute_densities'] = bool(torch.equal(whole.reshape(grid.shape), grid))
    del whole
    result['compute_densities_full_peak_bytes'] = peak(parent_style)

    sigma = grid[0][geo.crop_reference(res)].contiguous()
    D, H, W = sigma.shape
    result['crop_shape'] = [D, H, W]
    result['crop_grid_d2h_ms'], _ = timed(lambda: sigma.cpu())
    pinned = torch.empty(sigma.shape, dtype=sigma.dtype, pin_memory=True)
    result['crop_grid_d2h_pinned_ms'], _ = timed(lambda: pinned.copy_(sigma, non_blocking=True))
    cases = {}
    for tag, q in (('median', 0.5), ('p90', 0.9)):
        thresh = float(torch.quantile(sigma.flatten()[::7].float(), q))
        t_mc, (v, t) = timed(lambda: geo.marching_cubes(sigma, thresh))
        c = dict(thresh=thresh, vertices=int(v.shape[0]), triangles=int(t.shape[0]), marching_cubes_ms=t_mc)
        c['mesh_d2h_ms'], _ = timed(lambda: (v.cpu(), t.cpu()))
        _lib.profile_enable(True)
        for _ in range(args.reps):
            geo.marching_cubes(sigma, thresh)
        rep = _lib.profile_report()
        _lib.profile_enable(False)
        for k in ('mc_count_kernel', 'mc_scan_kernel', 'mc_emit_verts_kernel', 'mc_emit_tris_kernel'):
            c[k + '_ms'] = rep[k]['total_ms'] / rep[k]['launches'] if k in rep else None
            c[k + '_min_ms'] = rep[k]['min_ms'] if k in rep else None
        kernels = [c[k + '_ms'] for k in ('mc_count_kernel', 'mc_scan_kernel', 'mc_emit_verts_kernel', 'mc_emit_tris_kernel')]
        c['kernels_sum_ms'] = sum(x for x in kernels if x is not None)
        ideal = 4.0 * D * H * W                                  # one fp32 read per grid point (= per cell, up to the boundary)
        c['count_ideal_bytes'] = ideal
        c['count_achieved_GBps_vs_ideal_bytes'] = ideal / (c['mc_count_kernel_ms'] * 1e-3) / 1e9 if c['mc_count_kernel_ms'] else None
        c['count_moved_bytes'] = ideal + 2.0 * D * H * W         # + the 2-byte code it writes per point
        cases[tag] = c
    result['marching_cubes'] = cases
    m = cases['median']
    result['marcher_faster_than_crop_grid_copy'] = bool(m['marching_cubes_ms'] < result['crop_grid_d2h_ms'])
    result['density_grid_peak_fraction_of_full'] = result['density_grid_peak_bytes'] / max(result['compute_densities_full_peak_bytes'], 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Time mesh decimation on the GPU (mesh_decimate.py) -- quadric edge collapse in rounds -- next to vertex clustering
(mesh_simplify.py) at the same triangle counts, re-measured in the same run; writes profiles/mesh_decimate_bench.json.

    python tools/bench_mesh_decimate.py [--config c3] [--volume-res 256] [--samples 16] [--reps 7] [--out profiles/mesh_decimate_bench.json]

The scene is that of tools/bench_mesh_simplify.py: seeded weights, the level taken from the scene so that about half the rays hit, a
volume_res^3 grid over the whole field; the mesh measured is the sample whose triangle count is the median, in index units (voxels).  The
targets are the triangle counts `simplify` leaves at cells 2 and 4, so the two methods stand side by side.  Everything runs in this one
process, after a warm-up each; GPU time from events on the launch stream (the read-backs of every round included), min / median / max over
the repetitions.
  decimate    per target: the whole call, its rounds, the share of the vertices a round removes, and the time split by stage from the
              library's per-launch events (corner table / candidates / claim + select / apply / triangles / the rest)
  simplify    `mesh_simplify.simplify` at the cell that gave the target, in the same run
  quality     for both outputs: edges used by one triangle (the rim) and by more than two (non-manifold), and the distance of the output vertices from the level set, to
              first order through the field: |sigma - level| / |grad sigma| with sigma trilinear in the grid the mesh was extracted from
  host        the same decimation through host code, where a decimator is importable (none is required)
  files       the size of the binary .ply
Nothing is asserted: this tool reports, the stages where another route wins included.
"""
import argparse
import importlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = {'corner_table': ('ct_', 'ms_scan_kernel'), 'candidates': ('candidate_kernel',), 'claim_select': ('claim_kernel', 'select_kernel', 'dc_'),
          'apply': ('apply_kernel',), 'triangles': ('tri_', 'tk_', 'sp_scan_kernel')}
HOST_DECIMATORS = ('fast_simplification', 'pyfqmr', 'open3d', 'trimesh')


def stat(times, **more):
    med = float(np.median(times))
    return dict(ms_min=min(times), ms_median=med, ms_max=max(times), reps=len(times), spread=(max(times) - min(times)) / med if med else 0.0, **more)


def timed_device(fn):
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def commit_id():
    try:
        r = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else 'unknown'
    except OSError:
        return 'unknown'


def stage_of(kernel):
    for stage, prefixes in STAGES.items():
        if any(kernel.startswith(p) for p in prefixes):
            return stage
    return 'rest'


def odd_edges(t):
    """Undirected edges by use: dict(boundary: used by one triangle, non_manifold: used by more than two)."""
    import torch
    t = t.long()
    e = torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e = torch.sort(e, dim=1).values
    counts = torch.unique(e[:, 0] * (int(t.max()) + 1 if t.numel() else 1) + e[:, 1], return_counts=True)[1]
    return dict(boundary=int((counts == 1).sum()), non_manifold=int((counts > 2).sum()))


def level_distance(v, sigma, level, flip=True):
    """First-order distance of the points from the level set, in voxels: |sigma - level| / |grad sigma|, trilinear in the grid.  flip: the vertex
    columns are the grid's (i, j, k), and grid_sample takes (x, y, z) = (k, j, i) in [-1, 1]; main() takes the order under which the input mesh lies on its level set."""
    import torch
    D = torch.tensor(sigma.shape if flip else sigma.shape[::-1], device=v.device, dtype=torch.float64)

    def at(p):
        q = 2.0 * p.double() / (D - 1.0) - 1.0
        q = (q.flip(-1) if flip else q).float()
        return torch.nn.functional.grid_sample(sigma[None, None], q[None, None, None], mode='bilinear', padding_mode='border', align_corners=True).reshape(-1).double()
    h = 0.5
    s0 = at(v)
    grad = torch.stack([(at(v + torch.tensor(e, device=v.device) * h) - at(v - torch.tensor(e, device=v.device) * h)) / (2 * h)
                        for e in ((1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0))], -1)
    d = (s0 - level).abs() / grad.norm(dim=-1).clamp_min(1e-12)
    return dict(max_voxels=float(d.max()), rms_voxels=float((d * d).mean().sqrt()), p99_voxels=float(torch.quantile(d[:min(len(d), 2 ** 24)], 0.99)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='c3', help='generator configuration (tdgp.config.config_<name>)')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--volume-res', type=int, default=256)
    ap.add_argument('--cells', type=float, nargs='+', default=[2.0, 4.0], help='the targets are the triangle counts simplify leaves at these cells')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default=None, help='what the numbers were measured on (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mesh_decimate_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_decimate.py measures on a GPU; none found')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    I, Sh, S, Dm, g = tdgp.inference, tdgp.shapes, tdgp.mesh_simplify, tdgp.mesh_decimate, tdgp.geometry
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_mesh_decimate] {msg}', file=sys.stderr, flush=True)              # noqa: E731
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
    for b in range(n):                                                                                # the median sample, as bench_mesh_simplify.py finds it
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
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, commit=args.commit or commit_id(), config=args.config, samples=n, volume_res=vol,
               level=level, cube_size=box, sample=mid, vertices=nv, triangles=nt, units='index (voxels)',
               distance='first order through the field: |sigma - level| / |grad sigma|, sigma trilinear in the grid the mesh was extracted from',
               input=dict(odd_edges=odd_edges(t)))
    flip = level_distance(v, sigma, level, True)['rms_voxels'] <= level_distance(v, sigma, level, False)['rms_voxels']
    dist = lambda p: level_distance(p, sigma, level, flip)                                            # noqa: E731
    out['input']['distance'] = dist(v)
    out['vertex_columns'] = 'grid (i, j, k)' if flip else 'grid (k, j, i)'
    host = [m for m in HOST_DECIMATORS if importlib.util.find_spec(m) is not None]
    out['host'] = dict(importable=host, note='no host decimator is importable here; the restatement of the tests (plain Python, about 0.25 ms per edge per round) is not a '
                       'route anybody would take at this size' if not host else 'importable but not driven by this tool')

    def measure(fn, k=args.reps):
        fn()
        return stat([timed_device(fn) for _ in range(k)])

    def ply_bytes(vv, tt):
        with tempfile.TemporaryDirectory() as tmp:
            g.save_ply(os.path.join(tmp, 'a.ply'), vv, tt)
            return os.path.getsize(os.path.join(tmp, 'a.ply'))

    out['ply_bytes_before'] = ply_bytes(v, t)
    out['targets'] = {}
    for cell in args.cells:
        s = S.simplify(v, t, cell)
        target = int(s.triangles.shape[0])
        row = dict(cell=cell, target_triangles=target)
        row['simplify'] = dict(measure(lambda: S.simplify(v, t, cell)), vertices=int(s.vertices.shape[0]), triangles=target, odd_edges=odd_edges(s.triangles),
                               distance=dist(s.vertices), ply_bytes=ply_bytes(s.vertices, s.triangles))
        history = []
        d = Dm.decimate(v, t, target_triangles=target, history=history)
        dec = dict(measure(lambda: Dm.decimate(v, t, target_triangles=target)), vertices=int(d.vertices.shape[0]), triangles=int(d.triangles.shape[0]), rounds=d.rounds,
                   stopped=d.stopped, odd_edges=odd_edges(d.triangles), distance=dist(d.vertices), ply_bytes=ply_bytes(d.vertices, d.triangles))
        alive, shares = nv, []
        for T_before, selected, applied in history:
            shares.append(applied / max(alive, 1))
            alive -= applied
        dec['vertices_removed_per_round'] = dict(min=min(shares), median=float(np.median(shares)), max=max(shares), first=shares[0], last=shares[-1])
        dec['selected_per_round'] = [h[1] for h in history]
        dec['ms_per_round'] = dec['ms_median'] / max(d.rounds, 1)
        tdgp._lib.profile_enable(True)
        Dm.decimate(v, t, target_triangles=target)
        rep = tdgp._lib.profile_report()
        tdgp._lib.profile_enable(False)
        stages = {}
        for k_, r_ in rep.items():
            stages[stage_of(k_)] = stages.get(stage_of(k_), 0.0) + r_['total_ms']
        dec['kernel_ms_by_stage'] = stages
        dec['kernel_ms_per_round_by_stage'] = {k_: x / max(d.rounds, 1) for k_, x in stages.items()}
        dec['kernel_ms'] = {k_: r_['total_ms'] for k_, r_ in rep.items()}
        dec['kernel_launches'] = {k_: r_['launches'] for k_, r_ in rep.items()}
        dec['kernel_ms_total'] = sum(stages.values())
        again = Dm.decimate(v, t, target_triangles=target)
        dec['same_bytes_twice'] = bool(torch.equal(d.vertices, again.vertices) and torch.equal(d.triangles, again.triangles))
        row['decimate'] = dec
        row['decimate_over_simplify'] = dec['ms_median'] / row['simplify']['ms_median']
        say(f'target {target}: decimate {dec["ms_median"]:.1f} ms in {d.rounds} rounds ({d.stopped}), kernels {dec["kernel_ms_total"]:.1f} ms; simplify cell {cell:g} '
            f'{row["simplify"]["ms_median"]:.2f} ms; non-manifold edges {dec["odd_edges"]["non_manifold"]} vs {row["simplify"]["odd_edges"]["non_manifold"]}; rms distance {dec["distance"]["rms_voxels"]:.4f} vs '
            f'{row["simplify"]["distance"]["rms_voxels"]:.4f} voxel')
        out['targets'][str(target)] = row
    bound = Dm.decimate(v, t, max_error=0.05)
    out['max_error_0.05'] = dict(measure(lambda: Dm.decimate(v, t, max_error=0.05), k=3), triangles=int(bound.triangles.shape[0]), rounds=bound.rounds, stopped=bound.stopped,
                                 odd_edges=odd_edges(bound.triangles), distance=dist(bound.vertices))
    tdgp._lib.raise_on_device_fault('bench_mesh_decimate')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

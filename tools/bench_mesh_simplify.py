#!/usr/bin/env python3
"""Time mesh simplification on the GPU (mesh_simplify.py) -- clustering, triangle filter, corner table, quadric placement --
next to the same algorithm through stock tensor ops on the same GPU and through numpy on a host copy; writes profiles/mesh_simplify_bench.json.

    python tools/bench_mesh_simplify.py [--config c3] [--volume-res 256] [--samples 16] [--reps 7] [--out profiles/mesh_simplify_bench.json]

The scene is that of tools/bench_mesh_surface.py: seeded weights, the level taken from the scene so that about half the rays hit, a
volume_res^3 grid over the whole field; the mesh measured is the sample whose triangle count is the median, in index units (cells are in
voxels).  Everything runs in this one process, after a warm-up each; GPU time from events on the launch stream (read-backs included),
min / median / max over the repetitions.
  device      per cell (2 and 4 voxels): cluster_vertices (keys + sort + ids), the triangle pass (relabel + three sorts + flags + count + emit),
              the corner table of the relabelled triangles, the placement kernel on a given table, `simplify` as a whole under both
              placements, the kernels' own times from the library's per-launch events; and the ladder of cell_for_triangles(100000)
  torch       the same algorithm from stock tensor ops on the same GPU: torch.unique of the keys, index_add_ of the corner quadrics and the
              member sums, batched linalg.eigh, torch.unique(dim=0) of the rotated triples.  Its sums are floating-point ATOMICS
  host        copy out, numpy (unique, add.at, linalg.eigh), copy back: the route through host code, host clock
  files       the size of the binary .ply before and after
Nothing is asserted: this tool reports, the stages where another route wins included.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_HALF = 2 ** 20


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


def timed_host(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def commit_id():
    try:
        r = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else 'unknown'
    except OSError:
        return 'unknown'


# ---- the torch route: stock tensor ops on the device -------------------------------------------------------------------------------------
def torch_keys(v, cell):
    import torch
    q = torch.floor(v.double() / cell).long() + K_HALF
    return (q[:, 2] * 2 ** 21 + q[:, 1]) * 2 ** 21 + q[:, 0]


def torch_simplify(v, t, cell, rank_tol=1e-3, quadrics_only=False):
    """The algorithm of mesh_simplify.simplify(placement='quadric') from stock tensor ops -> (vertices [C,3], triangles [T',3])."""
    import torch
    x = v.double()
    ukey, cluster = torch.unique(torch_keys(v, cell), return_inverse=True)
    C = int(ukey.shape[0])
    tl = t.long()
    ct = cluster[tl]
    live = (ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2])
    idx = live.nonzero().squeeze(1)
    c = ct[idx]
    s = c.argmin(dim=1, keepdim=True)
    rot = torch.gather(c, 1, (s + torch.arange(3, device=v.device)) % 3)
    _, inv = torch.unique(rot, dim=0, return_inverse=True)
    first = torch.full([int(inv.max()) + 1 if inv.numel() else 0], 2 ** 62, dtype=torch.long, device=v.device).scatter_reduce_(0, inv, idx, 'amin')
    out_t = ct[first.sort().values].int()
    # placement
    k = torch.stack([(ukey & (2 ** 21 - 1)) - K_HALF, ((ukey >> 21) & (2 ** 21 - 1)) - K_HALF, (ukey >> 42) - K_HALF], dim=1).double()
    centre = (k + 0.5) * cell
    rel = x - centre[cluster]
    count = torch.bincount(cluster, minlength=C).double().unsqueeze(1)
    mean = torch.zeros(C, 3, dtype=torch.float64, device=v.device).index_add_(0, cluster, rel) / count
    A = torch.zeros(C, 3, 3, dtype=torch.float64, device=v.device)
    b = torch.zeros(C, 3, dtype=torch.float64, device=v.device)
    for i in range(3):
        ci = ct[:, i]
        p = x[tl] - centre[ci].unsqueeze(1)
        n = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
        d = -(n * p[:, 0]).sum(dim=1, keepdim=True)
        A.index_add_(0, ci, n.unsqueeze(2) * n.unsqueeze(1))
        b.index_add_(0, ci, n * d)
    if quadrics_only:
        return A
    lam, U = torch.linalg.eigh(A)
    r = -b - torch.einsum('cij,cj->ci', A, mean)
    coef = torch.einsum('cji,cj->ci', U, r) / lam.clamp_min(1e-300)
    coef = torch.where(lam > rank_tol * lam.max(dim=1, keepdim=True).values, coef, torch.zeros_like(coef))
    xq = mean + torch.einsum('cji,ci->cj', U, coef)
    ok = (torch.isfinite(xq) & (xq.abs() <= cell * 0.5)).all(dim=1, keepdim=True)
    return (centre + torch.where(ok, xq, mean)).float(), out_t


# ---- the host route: copy out, numpy, copy back ------------------------------------------------------------------------------------------
def host_simplify(v_dev, t_dev, cell, rank_tol=1e-3):
    import torch
    x, t = v_dev.cpu().numpy().astype(np.float64), t_dev.cpu().numpy().astype(np.int64)
    q = np.floor(x / cell).astype(np.int64) + K_HALF
    key = (q[:, 2] * 2 ** 21 + q[:, 1]) * 2 ** 21 + q[:, 0]
    ukey, cluster = np.unique(key, return_inverse=True)
    C = len(ukey)
    ct = cluster[t]
    idx = np.flatnonzero((ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2]))
    c = ct[idx]
    s = c.argmin(axis=1)[:, None]
    rot = np.take_along_axis(c, (s + np.arange(3)) % 3, axis=1)
    packed = (rot[:, 0] * C + rot[:, 1]) * C + rot[:, 2] if C < 2 ** 20 else None
    _, first = np.unique(packed, return_index=True) if packed is not None else np.unique(rot, axis=0, return_index=True)
    out_t = ct[idx[np.sort(first)]].astype(np.int32)
    k = np.stack([(ukey & (2 ** 21 - 1)) - K_HALF, ((ukey >> 21) & (2 ** 21 - 1)) - K_HALF, (ukey >> 42) - K_HALF], axis=1).astype(np.float64)
    centre = (k + 0.5) * cell
    rel = x - centre[cluster]
    count = np.bincount(cluster, minlength=C)[:, None].astype(np.float64)
    mean = np.stack([np.bincount(cluster, weights=rel[:, a], minlength=C) for a in range(3)], 1) / count
    A, b = np.zeros((C, 9)), np.zeros((C, 3))
    for i in range(3):
        ci = ct[:, i]
        p = x[t] - centre[ci][:, None, :]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        d = -(n * p[:, 0]).sum(axis=1, keepdims=True)
        nn = (n[:, :, None] * n[:, None, :]).reshape(-1, 9)
        for e in range(9):
            A[:, e] += np.bincount(ci, weights=nn[:, e], minlength=C)
        for e in range(3):
            b[:, e] += np.bincount(ci, weights=(n * d)[:, e], minlength=C)
    A = A.reshape(C, 3, 3)
    lam, U = np.linalg.eigh(A)
    r = -b - np.einsum('cij,cj->ci', A, mean)
    coef = np.einsum('cji,cj->ci', U, r) / np.maximum(lam, 1e-300)
    coef = np.where(lam > rank_tol * lam.max(axis=1, keepdims=True), coef, 0.0)
    xq = mean + np.einsum('cji,ci->cj', U, coef)
    ok = (np.isfinite(xq) & (np.abs(xq) <= cell * 0.5)).all(axis=1, keepdims=True)
    out_v = (centre + np.where(ok, xq, mean)).astype(np.float32)
    return torch.as_tensor(out_v).to(v_dev.device), torch.as_tensor(out_t).to(v_dev.device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='c3', help='generator configuration (tdgp.config.config_<name>)')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--volume-res', type=int, default=256)
    ap.add_argument('--cells', type=float, nargs='+', default=[2.0, 4.0])
    ap.add_argument('--max-triangles', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--commit', default=None, help='what the numbers were measured on (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mesh_simplify_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_simplify.py measures on a GPU; none found')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    I, Sh, S, Su, g = tdgp.inference, tdgp.shapes, tdgp.mesh_simplify, tdgp.mesh_surface, tdgp.geometry
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_mesh_simplify] {msg}', file=sys.stderr, flush=True)              # noqa: E731
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
    meshes, level = [], None
    for b in range(n):
        planes = tdgp.renderer.HWCPlanes(syn.tri_planes(ws[b:b + 1], noise_mode='const').t)
        if level is None:
            level = float(ray_field(planes, o0, d0, t0.reshape(1, R, Sr), res).reshape(R, Sr, 4)[..., 3].max(dim=1).values.median())
        sigma = g.density_grid_from_planes(G, planes, vol, cube_size=box)[0]
        meshes.append(g.marching_cubes(sigma, level))                                                 # index units: a cell is so many voxels
        del sigma, planes
    order = sorted(range(n), key=lambda b: int(meshes[b][1].shape[0]))
    mid = order[len(order) // 2]
    v, t = meshes[mid]
    del meshes
    nv, nt = int(v.shape[0]), int(t.shape[0])
    say(f'{vol}^3, sample {mid}: {nv} vertices, {nt} triangles')
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, commit=args.commit or commit_id(), config=args.config, samples=n,
               volume_res=vol, level=level, cube_size=box, sample=mid, vertices=nv, triangles=nt, rank_tol=1e-3, units='index (voxels)')
    reps = args.reps

    def measure(fn, timer=timed_device, k=reps):
        fn()
        return stat([timer(fn) for _ in range(k)])

    out['cells'] = {}
    for cell in args.cells:
        grid = S._grid(cell, (0, 0, 0))
        cl = S.cluster_vertices(v, cell)
        C = int(cl.key.shape[0])
        ct, rotated = S._relabel(t, nv, cl.cluster)
        table = Su._corner_table(ct, C)
        sq, sm = S.simplify(v, t, cell), S.simplify(v, t, cell, placement='mean')
        row = dict(clusters=C, triangles_out=int(sq.triangles.shape[0]), largest_cluster=int((cl.start[1:] - cl.start[:-1]).max()),
                   corners=int(table.corner.shape[0]), most_corners=int(table.degree.max()))

        def triangle_pass():
            ct_, rotated_ = S._relabel(t, nv, cl.cluster)
            return S._emit(ct_, *S._count(rotated_, True))

        device = dict(
            keys_ids=measure(lambda: S.cluster_vertices(v, cell)),
            triangles=measure(triangle_pass),
            triangles_no_dedup=measure(lambda: S._emit(ct, *S._count(rotated, False))),
            corner_table=measure(lambda: Su._corner_table(ct, C)),
            place_quadric=measure(lambda: S._place(v, t, cl, grid, table)),
            place_mean=measure(lambda: S._place(v, t, cl, grid, None)),
            simplify_quadric=measure(lambda: S.simplify(v, t, cell)),
            simplify_mean=measure(lambda: S.simplify(v, t, cell, placement='mean')))
        tdgp._lib.profile_enable(True)
        S.simplify(v, t, cell)
        rep = tdgp._lib.profile_report()
        tdgp._lib.profile_enable(False)
        device['kernel_ms'] = {k: r['total_ms'] / r['launches'] for k, r in rep.items()}
        device['kernel_launches'] = {k: r['launches'] for k, r in rep.items()}
        again = S.simplify(v, t, cell)
        device['same_bytes_twice'] = bool(torch.equal(sq.vertices, again.vertices) and torch.equal(sq.triangles, again.triangles))
        row['device'] = device
        for k_, s_ in device.items():
            if isinstance(s_, dict) and 'ms_median' in s_:
                say(f'cell {cell:g} device {k_}: {s_["ms_median"]:.3f} ms (spread {s_["spread"]:.0%})')
        # the torch route
        tv, tt = torch_simplify(v, t, cell)
        tor = dict(simplify_quadric=measure(lambda: torch_simplify(v, t, cell)))
        tor['unique_keys'] = measure(lambda: torch.unique(torch_keys(v, cell), return_inverse=True))
        quadrics = torch_simplify(v, t, cell, quadrics_only=True)
        tor['eigh'] = measure(lambda: torch.linalg.eigh(quadrics))
        tor['same_counts_as_device'] = bool(tv.shape == sq.vertices.shape and tt.shape == sq.triangles.shape)
        tor['same_triangles_as_device'] = bool(tt.shape == sq.triangles.shape and torch.equal(tt, sq.triangles))
        tor['vertices_max_abs_diff_vs_device'] = float((tv - sq.vertices).abs().max()) if tv.shape == sq.vertices.shape else None
        tor['vertices_median_abs_diff_vs_device'] = float((tv - sq.vertices).abs().median()) if tv.shape == sq.vertices.shape else None
        tv2 = torch_simplify(v, t, cell)[0]
        tor['same_bytes_twice'] = bool(torch.equal(tv, tv2))
        tor['note'] = 'index_add_ sums with floating-point atomics: the order of the additions is not fixed; eigh orders and signs its vectors its own way'
        row['torch'] = tor
        say(f'cell {cell:g} torch simplify: {tor["simplify_quadric"]["ms_median"]:.3f} ms; max |dv| {tor["vertices_max_abs_diff_vs_device"]}')
        # the host route
        hv, ht = host_simplify(v, t, cell)
        host = dict(simplify_quadric=measure(lambda: host_simplify(v, t, cell), timed_host, args.host_reps), route='copy out, numpy (unique, bincount, linalg.eigh), copy back')
        host['same_triangles_as_device'] = bool(ht.shape == sq.triangles.shape and torch.equal(ht, sq.triangles))
        host['vertices_max_abs_diff_vs_device'] = float((hv - sq.vertices).abs().max()) if hv.shape == sq.vertices.shape else None
        row['host'] = host
        say(f'cell {cell:g} host simplify: {host["simplify_quadric"]["ms_median"]:.1f} ms')
        row['ratios'] = dict(torch_over_device=tor['simplify_quadric']['ms_median'] / device['simplify_quadric']['ms_median'],
                             host_over_device=host['simplify_quadric']['ms_median'] / device['simplify_quadric']['ms_median'],
                             torch_unique_over_device_keys_ids=tor['unique_keys']['ms_median'] / device['keys_ids']['ms_median'])
        # files
        with tempfile.TemporaryDirectory() as tmp:
            g.save_ply(os.path.join(tmp, 'a.ply'), v, t)
            g.save_ply(os.path.join(tmp, 'b.ply'), sq.vertices, sq.triangles)
            row['ply_bytes_before'], row['ply_bytes_after'] = os.path.getsize(os.path.join(tmp, 'a.ply')), os.path.getsize(os.path.join(tmp, 'b.ply'))
        del sm
        out['cells'][f'{cell:g}'] = row

    # ---- the ladder ----
    cell = S.cell_for_triangles(v, t, args.max_triangles)
    lad = measure(lambda: S.cell_for_triangles(v, t, args.max_triangles))
    rungs = [c_ for c_ in S.ladder() if c_ <= cell]
    lad.update(max_triangles=args.max_triangles, cell=cell, rungs=len(rungs), counts=[S.count_triangles(v, t, c_) for c_ in rungs])
    s = S.simplify(v, t, cell)
    lad.update(triangles_out=int(s.triangles.shape[0]), vertices_out=int(s.vertices.shape[0]), simplify_quadric=measure(lambda: S.simplify(v, t, cell)))
    out['ladder'] = lad
    say(f'ladder to {args.max_triangles}: cell {cell:g} after {len(rungs)} rungs, {lad["ms_median"]:.3f} ms; {lad["triangles_out"]} triangles')
    tdgp._lib.raise_on_device_fault('bench_mesh_simplify')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

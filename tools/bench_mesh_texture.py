#!/usr/bin/env python3
"""Time the mesh-texture bake and textured mesh frames on the GPU (mesh_texture.py) next to the same bake through stock tensor
ops on the same GPU and through numpy on a host copy, and next to vertex-colour and face-normal frames; writes profiles/mesh_texture_bench.json.

    python tools/bench_mesh_texture.py [--config c3] [--volume-res 256] [--samples 16] [--frames 8] [--reps 7] [--out profiles/mesh_texture_bench.json]

The scene is that of tools/bench_mesh_simplify.py: seeded weights, the level taken from the scene so that about half the rays hit, a
volume_res^3 grid over the whole field; the mesh is the sample whose triangle count is the median, simplified with `--cells` (2 and 4
voxels) and taken to world units; `--texels` (6 and 8) go with the cells in order.  Everything runs in this one process, after a warm-up
each; GPU time from events on the launch stream, min / median / max over the repetitions.
  device      per (cell, texels): tdgp_atlas_points, the field pass over every texel's point, tdgp_atlas_texels, `bake_field` as a whole, and the
              corner UVs it computes on the host (numpy) for the .obj writer
  torch       the same bake from stock tensor ops on the same GPU (integer ops for the owners, float64 for the points, clamp / round / to(uint8));
              the field pass is the same kernel in all three routes -- it has no other implementation
  host        mesh copied out, owners and points in numpy, points copied in, the field on the device, colours copied out, quantised in numpy,
              the image copied in: the route through host code, host clock
  frames      `--frames` views of the textured mesh (nearest and bilinear), of the same mesh with vertex colours and with face normals, per frame
  files       the .png of the atlas next to the binary .ply with vertex colours
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
def torch_points(v, t, atlas):
    """tdgp_atlas_points from stock tensor ops -> (points fp32 [H*W,3], owner int64 [H*W])."""
    import torch
    n, S, r, W, H = atlas
    dev = v.device
    T = int(t.shape[0])
    i = torch.arange(W * H, device=dev)
    row, col = i // W, i % W
    tx, ty = col // S, row // S
    px, py = col - tx * S, row - ty * S
    lower = px + py <= n
    k = 2 * (ty * r + tx) + (~lower).long()
    qx, qy = torch.where(lower, px, S - 1 - px), torch.where(lower, py, S - 1 - py)
    owned = k < T
    idx = t.long()[torch.where(owned, k, torch.zeros_like(k))]
    owned = owned & ((idx >= 0) & (idx < v.shape[0])).all(dim=1)
    P = v.double()[idx.clamp(0, v.shape[0] - 1)]
    b1, b2 = qx.double() / (n - 1), qy.double() / (n - 1)
    b0 = (1.0 - b1) - b2
    p = ((b0[:, None] * P[:, 0] + b1[:, None] * P[:, 1]) + b2[:, None] * P[:, 2]).float()
    return torch.where(owned[:, None], p, torch.zeros_like(p)), torch.where(owned, k, -torch.ones_like(k))


def torch_texels(rgb, owner, atlas):
    import torch
    k = (rgb[:, :3] * 0.5 + 0.5).clamp(0.0, 1.0)
    byte = torch.round(k * 255.0).to(torch.uint8)
    return torch.where((owner >= 0)[:, None], byte, torch.zeros_like(byte)).reshape(atlas.height, atlas.width, 3)


# ---- the host route ----------------------------------------------------------------------------------------------------------------------
def host_bake(v_dev, t_dev, atlas, colour_fn):
    import torch
    v, t = v_dev.cpu().numpy(), t_dev.cpu().numpy().astype(np.int64)
    n, S, r, W, H = atlas
    T = len(t)
    col, row = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    col, row = col.reshape(-1), row.reshape(-1)
    tx, ty = col // S, row // S
    px, py = col - tx * S, row - ty * S
    lower = px + py <= n
    k = 2 * (ty * r + tx) + np.where(lower, 0, 1)
    qx, qy = np.where(lower, px, S - 1 - px), np.where(lower, py, S - 1 - py)
    owned = k < T
    idx = t[np.where(owned, k, 0)]
    owned &= ((idx >= 0) & (idx < len(v))).all(axis=1)
    P = v[np.clip(idx, 0, len(v) - 1)].astype(np.float64)
    b1, b2 = qx / float(n - 1), qy / float(n - 1)
    b0 = (1.0 - b1) - b2
    p = np.where(owned[:, None], (b0[:, None] * P[:, 0] + b1[:, None] * P[:, 1]) + b2[:, None] * P[:, 2], 0.0).astype(np.float32)
    rgb = colour_fn(torch.as_tensor(p).to(v_dev.device))[:, :3].cpu().numpy()
    byte = np.rint(np.clip(rgb * np.float32(0.5) + np.float32(0.5), 0.0, 1.0) * np.float32(255)).astype(np.uint8)
    image = np.where(owned[:, None], byte, 0).astype(np.uint8).reshape(H, W, 3)
    return torch.as_tensor(image).to(v_dev.device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='c3', help='generator configuration (tdgp.config.config_<name>)')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--volume-res', type=int, default=256)
    ap.add_argument('--cells', type=float, nargs='+', default=[2.0, 4.0])
    ap.add_argument('--texels', type=int, nargs='+', default=[6, 8], help='one per cell')
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--commit', default=None, help='what the numbers were measured on (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mesh_texture_bench.json'))
    args = ap.parse_args(argv)
    if len(args.cells) != len(args.texels):
        ap.error('--cells and --texels go in pairs')
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_texture.py measures on a GPU; none found')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    I, Sh, S, Tx, M, g = tdgp.inference, tdgp.shapes, tdgp.mesh_simplify, tdgp.mesh_texture, tdgp.mesh, tdgp.geometry
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_mesh_texture] {msg}', file=sys.stderr, flush=True)               # noqa: E731
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
    cams1 = I.generate_camera_params(G, z, c, dict(I.SNAPSHOT_TRAJECTORY, num_frames=1)).to(dtype=torch.float32, device=dev)
    ray_field = Sh.field_functions(syn)[0]
    o0, d0 = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cams1[:1]), fov=cams1.fov[:1], resolution=(res, res), device=dev)
    t0 = Sh.coarse_depths(syn, R, Sr, dev)
    counts, level = [], None
    for b in range(n):
        planes = tdgp.renderer.HWCPlanes(syn.tri_planes(ws[b:b + 1], noise_mode='const').t)
        if level is None:
            level = float(ray_field(planes, o0, d0, t0.reshape(1, R, Sr), res).reshape(R, Sr, 4)[..., 3].max(dim=1).values.median())
        sigma = g.density_grid_from_planes(G, planes, vol, cube_size=box)[0]
        counts.append(int(g.marching_cubes(sigma, level)[1].shape[0]))
        del sigma, planes
    mid = sorted(range(n), key=lambda b: counts[b])[n // 2]
    planes = tdgp.renderer.HWCPlanes(syn.tri_planes(ws[mid:mid + 1], noise_mode='const').t)
    v0, t0_ = g.marching_cubes(g.density_grid_from_planes(G, planes, vol, cube_size=box)[0], level)
    say(f'{vol}^3, sample {mid}: {int(v0.shape[0])} vertices, {int(t0_.shape[0])} triangles')
    cams = I.generate_camera_params(G, z[mid:mid + 1], c[mid:mid + 1], dict(I.SNAPSHOT_TRAJECTORY, num_frames=args.frames)).to(dtype=torch.float32, device=dev)
    frames = int(cams.angles.shape[0])
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, commit=args.commit or commit_id(), config=args.config, samples=n,
               volume_res=vol, level=level, cube_size=box, sample=mid, vertices=int(v0.shape[0]), triangles=int(t0_.shape[0]), frames=frames,
               frame_resolution=res)
    reps = args.reps
    colour_fn = Tx.field_colour_fn(G, planes)

    def measure(fn, timer=timed_device, k=reps):
        fn()
        return stat([timer(fn) for _ in range(k)])

    out['cases'] = {}
    for cell, texels in zip(args.cells, args.texels):
        sv, st = S.simplify(v0, t0_, cell)[:2]
        world = g.grid_to_world(sv, vol, (0.0, 0.0, 0.0), box, None)
        T = int(st.shape[0])
        atlas = Tx.atlas_layout(T, texels)
        N = atlas.width * atlas.height
        row = dict(cell=cell, texels=texels, vertices=int(world.shape[0]), triangles=T, atlas=[atlas.width, atlas.height], atlas_texels=N,
                   texels_per_vertex=N / max(int(world.shape[0]), 1))
        points, owner = Tx.atlas_points(world, st, atlas)
        row['owned_texels'] = int((owner >= 0).sum())
        rgb = colour_fn(points)
        image = torch.empty([N, 3], dtype=torch.uint8, device=dev)
        tex = Tx.bake_field(G, planes, world, st, texels=texels)
        device = dict(points=measure(lambda: Tx.atlas_points(world, st, atlas)), field=measure(lambda: colour_fn(points)),
                      texels=measure(lambda: Tx.atlas_texels(rgb, owner, image)), bake=measure(lambda: Tx.bake_field(G, planes, world, st, texels=texels)))
        device['uvs_on_the_host'] = measure(lambda: Tx.atlas_uvs(T, atlas), timed_host)
        device['field_share_of_bake'] = device['field']['ms_median'] / device['bake']['ms_median']
        device['field_share_of_the_three_stages'] = device['field']['ms_median'] / (device['points']['ms_median'] + device['field']['ms_median'] + device['texels']['ms_median'])
        device['same_bytes_twice'] = bool(torch.equal(Tx.bake_field(G, planes, world, st, texels=texels).image, tex.image))
        row['device'] = device
        for k_, s_ in device.items():
            if isinstance(s_, dict):
                say(f'cell {cell:g} texels {texels} device {k_}: {s_["ms_median"]:.3f} ms (spread {s_["spread"]:.0%})')
        tp, to = torch_points(world, st, atlas)
        ti = torch_texels(rgb, to, atlas)
        tor = dict(points=measure(lambda: torch_points(world, st, atlas)), texels=measure(lambda: torch_texels(rgb, to, atlas)),
                   bake=measure(lambda: torch_texels(colour_fn(torch_points(world, st, atlas)[0]), to, atlas)),
                   same_points_as_device=bool(torch.equal(tp, points)), same_image_as_device=bool(torch.equal(ti, tex.image)),
                   image_bytes_that_differ=int((ti != tex.image).sum()))
        row['torch'] = tor
        say(f'cell {cell:g} torch: points {tor["points"]["ms_median"]:.3f} ms, texels {tor["texels"]["ms_median"]:.3f} ms, bake {tor["bake"]["ms_median"]:.3f} ms')
        hi = host_bake(world, st, atlas, colour_fn)
        host = dict(bake=measure(lambda: host_bake(world, st, atlas, colour_fn), timed_host, args.host_reps), same_image_as_device=bool(torch.equal(hi, tex.image)),
                    route='mesh out, numpy owners and points, points in, the field on the device, colours out, numpy quantisation, image in')
        row['host'] = host
        say(f'cell {cell:g} host bake: {host["bake"]["ms_median"]:.1f} ms')
        row['ratios'] = dict(torch_over_device_bake=tor['bake']['ms_median'] / device['bake']['ms_median'],
                             host_over_device_bake=host['bake']['ms_median'] / device['bake']['ms_median'],
                             torch_over_device_points_and_texels=(tor['points']['ms_median'] + tor['texels']['ms_median'])
                             / (device['points']['ms_median'] + device['texels']['ms_median']))
        # frames: unlit colour so that the four routes shade alike
        vc = M.vertex_colours(G, planes, world)
        kw = dict(G=G, ambient=1.0)
        fr = dict(
            texture_nearest=measure(lambda: M.render_mesh_views(world, st, cams, res, mode='colour', texture=tex, texture_filter='nearest', **kw)),
            texture_bilinear=measure(lambda: M.render_mesh_views(world, st, cams, res, mode='colour', texture=tex, texture_filter='bilinear', **kw)),
            vertex_colours=measure(lambda: M.render_mesh_views(world, st, cams, res, mode='colour', vertex_colours=vc, **kw)),
            face_normals=measure(lambda: M.render_mesh_views(world, st, cams, res, mode='shaded', **kw)))
        for s_ in fr.values():
            s_['ms_per_frame'] = s_['ms_median'] / frames
        tdgp._lib.profile_enable(True)
        M.render_mesh_views(world, st, cams, res, mode='colour', texture=tex, texture_filter='bilinear', **kw)
        Tx.bake_field(G, planes, world, st, texels=texels)
        rep = tdgp._lib.profile_report()
        tdgp._lib.profile_enable(False)
        fr['kernel_ms'] = {k: r['total_ms'] / r['launches'] for k, r in rep.items()}
        fr['hit_fraction'] = float(M.render_mesh_views(world, st, cams, res, mode='shaded', **kw).status.float().mean())
        row['frames'] = fr
        say(f'cell {cell:g} frames: ' + ', '.join(f'{k} {s_["ms_per_frame"]:.4f} ms' for k, s_ in fr.items() if isinstance(s_, dict) and 'ms_per_frame' in s_))
        with tempfile.TemporaryDirectory() as tmp:
            g.save_ply(os.path.join(tmp, 'a.ply'), world, st, colours=vc)
            g.save_obj(os.path.join(tmp, 'a.obj'), world, st, texture=tex)
            row['files'] = dict(ply_with_vertex_colours_bytes=os.path.getsize(os.path.join(tmp, 'a.ply')), png_bytes=os.path.getsize(os.path.join(tmp, 'a.png')),
                                obj_with_vt_bytes=os.path.getsize(os.path.join(tmp, 'a.obj')), raw_image_bytes=N * 3)
        out['cases'][f'cell {cell:g}, texels {texels}'] = row
    tdgp._lib.raise_on_device_fault('bench_mesh_texture')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

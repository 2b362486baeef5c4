#!/usr/bin/env python3
"""Time shape frames (shapes.render_shape_video_grid) against the RGB frames of the same cameras and against the mesh route, and write
profiles/shape_render_bench.json.

    python tools/bench_shapes.py [--config c3] [--samples 16] [--frames 32] [--reps 5] [--out profiles/shape_render_bench.json]

The workload is the snapshot video of tools/bench_trajectory.py: --samples samples x --frames `front_circle` frames around the mean camera, seeded
weights, plane batch 4; shape frames in shaded mode with the configuration's coarse steps and --num-refine fine ones.  The level is taken from the
scene (the median over the rays of sample 0's first frame of their largest coarse density), so that about half the rays hit.  All routes run in
this one process, alternating, after one warm-up each; GPU time from events on the launch stream; min / median / max over the repetitions.
  video     `render_shape_video_grid` against `render_video_grid` (the RGB frames: backbone, renderer, uint8 grid) on the same cameras
  frames    the frames alone, backbone included, no grid: `shapes._shape_batches` against `inference._plane_batches(ray_major=True)`
  mesh      `extract_geometry` at --volume-res^3 for the same samples (density grid + marching cubes), thresholded at the same level
  passes    one call's worth of rays (16 frames of 4 samples): the three field passes and the three new kernels, each timed on its own
  kernels   the new kernels' own times over a whole video from the library's per-launch events, with the bytes they move (from the shapes)
Nothing is asserted: this tool reports.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stat(times, **more):
    med = float(np.median(times))
    return dict(ms_min=min(times), ms_median=med, ms_max=max(times), reps=len(times), spread=(max(times) - min(times)) / med, **more)


def timed_device(fn):
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_bytes(rays, S, N):
    """Bytes each new kernel moves for `rays` rays, from the shapes.  sigma is one dword of every 16-byte row of the field's output, read in place: the
    cache lines of the whole rows are fetched, so the rows are counted whole (the bytes the loads themselves return are a quarter of that term)."""
    return dict(iso_bracket_kernel=rays * (S * 16 + 2 * 4 + 4 + N * 4),
                iso_locate_kernel=rays * (N * 16 + 4 + 16 + 4 * 4 + 24 + 4 + 4 + 21 * 4),
                iso_shade_kernel=rays * (7 * 16 + 4 + 12 + 12 + 12))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='c3', help='generator configuration (tdgp.config.config_<name>)')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--num-refine', type=int, default=16)
    ap.add_argument('--volume-res', type=int, default=256)
    ap.add_argument('--plane-batch', type=int, default=4)
    ap.add_argument('--skip', default='', help='comma-separated parts to leave out: video,frames,mesh,passes,kernels')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'shape_render_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_shapes.py measures on a GPU; none found')
    tdgp = importlib.import_module('3dgp_amd')
    I, Sh = tdgp.inference, tdgp.shapes
    skip = set(args.skip.split(','))
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_shapes] {msg}', file=sys.stderr, flush=True)                      # noqa: E731
    cfg = getattr(tdgp.config, f'config_{args.config}')()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=0))
    G = G.to(dev).eval()
    syn = G.synthesis
    n, V, res, pb = args.samples, args.frames, syn.test_resolution, args.plane_batch
    R, S, N = res * res, int(cfg.num_ray_steps), args.num_refine
    inp = tdgp.weights.synthetic_inputs(cfg, batch=n, seed=1)
    z, c = torch.as_tensor(inp['z']).to(dev), torch.as_tensor(inp['c']).to(dev)
    torch.manual_seed(0)
    np.random.seed(0)
    with torch.no_grad():
        ws = G.mapping(z, c)
        cams = I.generate_camera_params(G, z, c, dict(I.SNAPSHOT_TRAJECTORY, num_frames=V)).to(dtype=torch.float32, device=dev)
        # the level: from the scene's own coarse densities
        planes0 = syn.tri_planes(ws[:1], noise_mode='const')
        ray_field, point_field = Sh.field_functions(syn)
        o0, d0 = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cams[:1]), fov=cams.fov[:1], resolution=(res, res), device=dev)
        t0 = Sh.coarse_depths(syn, R, S, dev)
        level = float(ray_field(planes0, o0, d0, t0.reshape(1, R, S), res).reshape(R, S, 4)[..., 3].max(dim=1).values.median())
    kw = dict(level=level, mode='shaded', num_refine=N)
    res_json = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, config=args.config, samples=n, frames_per_sample=V, img_resolution=res,
                    ray_steps=S, num_refine=N, plane_batch=pb, mode='shaded', level=level, field_points_per_ray=dict(shape=S + N + Sh.STENCIL, rgb=2 * S))

    def shape_frames():
        for _ in Sh._shape_batches(G, ws, cams, pb, **kw):
            pass

    def rgb_frames():
        for _ in I._plane_batches(G, ws, cams, pb, ray_major=True):
            pass

    def compare(name, new, old, new_key, old_key):
        new(), old()                                                                                   # warm-up
        t_new, t_old = [], []
        for _ in range(args.reps):
            t_new.append(timed_device(new))
            t_old.append(timed_device(old))
        fps = lambda t: n * V / (float(np.median(t)) * 1e-3)                                           # noqa: E731
        res_json[name] = r = {new_key: stat(t_new, frames_per_s=fps(t_new)), old_key: stat(t_old, frames_per_s=fps(t_old)),
                              'shape_over_rgb_time': float(np.median(t_new)) / float(np.median(t_old))}
        say(f'{name}: shape {r[new_key]["ms_median"]:.1f} ms (spread {r[new_key]["spread"]:.3f}), rgb {r[old_key]["ms_median"]:.1f} ms '
            f'(spread {r[old_key]["spread"]:.3f}), ratio {r["shape_over_rgb_time"]:.3f}')

    with torch.no_grad():
        hit = float((next(iter(Sh._shape_batches(G, ws[:1], cams[:V], 1, **kw))).status != 0).float().mean())
        res_json['hit_share_sample_0'] = hit
        say(f'level {level:.4g}: {hit:.3f} of the rays of sample 0 hit')
        if 'video' not in skip:
            compare('video', lambda: Sh.render_shape_video_grid(G, ws, cams, plane_batch=pb, **kw), lambda: I.render_video_grid(G, ws, cams, plane_batch=pb),
                    'shape_video_grid', 'rgb_video_grid')
        if 'frames' not in skip:
            compare('frames', shape_frames, rgb_frames, 'shape_frames', 'rgb_frames')
        if 'mesh' not in skip:
            mesh = lambda: tdgp.geometry.extract_geometry(G, ws, volume_res=args.volume_res, cube_size=2.0 * cfg.cube_scale, thresh_value=level, crop=None)   # noqa: E731
            shapes = mesh()
            t_mesh = [timed_device(mesh) for _ in range(args.reps)]
            res_json['mesh'] = r = dict(extract_geometry=stat(t_mesh, samples_per_s=n / (float(np.median(t_mesh)) * 1e-3)), volume_res=args.volume_res,
                                        field_points_per_sample=args.volume_res ** 3, triangles_sample_0=int(shapes[0].triangles.shape[0]))
            if 'frames' in res_json:
                r['ms_per_sample'] = r['extract_geometry']['ms_median'] / n
                r['shape_frames_ms_per_sample'] = res_json['frames']['shape_frames']['ms_median'] / n
            say(f'mesh: extract_geometry {r["extract_geometry"]["ms_median"]:.0f} ms for {n} samples at {args.volume_res}^3')
        if 'passes' not in skip:
            nb = min(pb, n)
            nv = max(1, min(16 // nb, V))                                                              # what one call of render_shape_views holds by default
            planes = syn.tri_planes(ws[:nb], noise_mode='const')
            idx = torch.cat([torch.arange(nv) + b * V for b in range(nb)]).to(dev)
            o, d = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cams[idx]), fov=cams.fov[idx], resolution=(res, res), device=dev)
            o, d = o.reshape(nb, nv * R, 3).contiguous(), d.reshape(nb, nv * R, 3).contiguous()
            rays = nb * nv * R
            t = Sh.coarse_depths(syn, rays, S, dev)
            step = 2.0 * cfg.cube_scale / cfg.tri_plane_res
            st = {}
            f_c = lambda: ray_field(planes, o, d, t.reshape(nb, nv * R, S), res)                        # noqa: E731
            rgbs_c = f_c()
            sig_c = rgbs_c.reshape(rays, S, 4)[..., 3]
            k_b = lambda: Sh.iso_bracket(sig_c, t, N, level)                                           # noqa: E731
            i_, t_fine = k_b()
            f_f = lambda: ray_field(planes, o, d, t_fine.reshape(nb, nv * R, N), res)                   # noqa: E731
            rgbs_f = f_f()
            k_l = lambda: Sh.iso_locate(sig_c, t, i_, rgbs_f.reshape(rays, N, 4)[..., 3], t_fine, o, d, level, step, float(cfg.ray_end))   # noqa: E731
            _, status, points = k_l()
            f_s = lambda: point_field(planes, points.reshape(nb, nv * R * Sh.STENCIL, 3))               # noqa: E731
            stencil = f_s()
            k_s = lambda: Sh.iso_shade(stencil, status, d)                                             # noqa: E731
            k_s()
            u = torch.rand(rays, S, device=dev)
            rgb_call = lambda: syn.renderer(planes, syn.tri_plane_mlp, o, d, dict(syn.rendering_options(syn._default_render_options), ray_grid_w=res,   # noqa: E731
                                                                                   u_coarse=u, u_fine=u, n_coarse=None, n_fine=None))
            rgb_call()
            parts = dict(field_coarse=(f_c, rays * S), iso_bracket=(k_b, 0), field_fine=(f_f, rays * N), iso_locate=(k_l, 0),
                         field_stencil=(f_s, rays * Sh.STENCIL), iso_shade=(k_s, 0), rgb_renderer_call=(rgb_call, rays * 2 * S))
            times = {k: [] for k in parts}
            for _ in range(args.reps):
                for k, (fn, _) in parts.items():
                    times[k].append(timed_device(fn))
            for k, (fn, pts) in parts.items():
                st[k] = stat(times[k], **({'field_points': pts, 'ns_per_point': float(np.median(times[k])) * 1e6 / pts} if pts else {}))
            res_json['passes'] = dict(rays=rays, samples=nb, frames_per_sample=nv, **st)
            say('passes: ' + ', '.join(f'{k} {v["ms_median"]:.2f} ms' for k, v in st.items()))
        if 'kernels' not in skip:
            shape_frames()
            torch.cuda.synchronize()
            tdgp._lib.profile_enable(True)
            shape_frames()
            rep = tdgp._lib.profile_report()
            tdgp._lib.profile_enable(False)
            moved = kernel_bytes(n * V * R, S, N)
            out = {}
            for k, v in rep.items():
                if k.startswith('iso_'):
                    out[k] = dict(v, bytes=moved[k], gb_per_s=moved[k] / (v['total_ms'] * 1e-3) / 1e9)
                elif k in ('triplane_field_kernel', 'stratified_kernel'):
                    out[k] = v
            res_json['kernels'] = out
            say('kernels: ' + ', '.join(f'{k} {v["total_ms"]:.2f} ms' + (f' ({v["gb_per_s"]:.0f} GB/s)' if 'gb_per_s' in v else '') for k, v in out.items()))
    tdgp._lib.raise_on_device_fault('bench_shapes')

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res_json, f, indent=1)
    print(json.dumps(res_json))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Time mesh frames (mesh.render_mesh_views on the mesh extracted once per sample) against shape frames of the same cameras, and write
profiles/mesh_frames_bench.json.

    python tools/bench_mesh_frames.py [--config c3] [--samples 16] [--frames 32] [--volume-res 128,256] [--reps 5] [--out profiles/mesh_frames_bench.json]

The workload is the snapshot video of tools/bench_shapes.py: --samples samples x --frames `front_circle` frames around the mean camera, seeded
weights, the level taken from the scene so that about half the rays hit.  Everything runs in this one process, alternating, after one warm-up
each; GPU time from events on the launch stream; min / median / max over the repetitions.  The tri-planes of all samples are computed once,
outside every timed region (both routes need them and pay the same backbone).
  shape_frames   `shapes.render_shape_views` per sample on its planes: the yardstick, re-measured here
  per volume_res:
    extraction   per sample: `density_grid_from_planes` -> `marching_cubes` -> `grid_to_world`; triangles per sample
    face / field `render_mesh_views` per sample on its mesh (field: with its planes): ms per frame, and the kernels' own times per frame
                 from the library's per-launch events
    break_even   frames per sample from which extraction + mesh frames cost less than shape frames: extraction / (shape frame - mesh frame)
    video        `render_mesh_video_grid` (backbone, extraction, frames, uint8 grid) against `render_shape_video_grid`
Nothing is asserted: this tool reports.
"""
import argparse
import importlib
import json
import os
import subprocess
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


def commit_id():
    try:
        r = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else 'unknown'
    except OSError:
        return 'unknown'


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='c3', help='generator configuration (tdgp.config.config_<name>)')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--volume-res', default='128,256', help='comma-separated grid sizes')
    ap.add_argument('--commit', default=None, help='what the numbers were measured on (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mesh_frames_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_frames.py measures on a GPU; none found')
    tdgp = importlib.import_module('3dgp_amd')
    I, Sh, M, g = tdgp.inference, tdgp.shapes, tdgp.mesh, tdgp.geometry
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_mesh_frames] {msg}', file=sys.stderr, flush=True)                # noqa: E731
    cfg = getattr(tdgp.config, f'config_{args.config}')()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=0))
    G = G.to(dev).eval()
    syn = G.synthesis
    n, V, res = args.samples, args.frames, syn.test_resolution
    R, S, N = res * res, int(cfg.num_ray_steps), 16
    box = 2.0 * float(cfg.cube_scale)
    inp = tdgp.weights.synthetic_inputs(cfg, batch=n, seed=1)
    z, c = torch.as_tensor(inp['z']).to(dev), torch.as_tensor(inp['c']).to(dev)
    torch.manual_seed(0)
    np.random.seed(0)
    with torch.no_grad():
        ws = G.mapping(z, c)
        cams = I.generate_camera_params(G, z, c, dict(I.SNAPSHOT_TRAJECTORY, num_frames=V)).to(dtype=torch.float32, device=dev)
        planes = [tdgp.renderer.HWCPlanes(syn.tri_planes(ws[b:b + 1], noise_mode='const').t) for b in range(n)]
        ray_field = Sh.field_functions(syn)[0]
        o0, d0 = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cams[:1]), fov=cams.fov[:1], resolution=(res, res), device=dev)
        t0 = Sh.coarse_depths(syn, R, S, dev)
        level = float(ray_field(planes[0], o0, d0, t0.reshape(1, R, S), res).reshape(R, S, 4)[..., 3].max(dim=1).values.median())
    cam_of = lambda b: cams[b * V:(b + 1) * V]                                                          # noqa: E731
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, commit=args.commit or commit_id(), config=args.config, samples=n,
               frames_per_sample=V, img_resolution=res, ray_steps=S, num_refine=N, level=level, cube_size=box,
               field_points_per_ray=dict(shape=S + N + Sh.STENCIL, mesh_face=0, mesh_field=M.STENCIL))

    def shape_frames():
        for b in range(n):
            Sh.render_shape_views(G, planes[b], cam_of(b), level=level, num_refine=N)

    with torch.no_grad():
        shape_frames()
        t_shape = [timed_device(shape_frames) for _ in range(args.reps)]
        shape_ms = float(np.median(t_shape)) / (n * V)
        out['shape_frames'] = stat(t_shape, ms_per_frame=shape_ms)
        say(f'shape frames: {shape_ms:.4f} ms per frame')
        Sh.render_shape_video_grid(G, ws, cams, level=level, num_refine=N)
        t_shape_video = [timed_device(lambda: Sh.render_shape_video_grid(G, ws, cams, level=level, num_refine=N)) for _ in range(args.reps)]
        out['shape_video_grid'] = stat(t_shape_video)
        for vol in (int(v) for v in args.volume_res.split(',')):
            meshes = []

            def extract():
                meshes.clear()
                for b in range(n):
                    sigma = g.density_grid_from_planes(G, planes[b], vol, cube_size=box)[0]
                    verts, tris = g.marching_cubes(sigma, level)
                    meshes.append((g.grid_to_world(verts, vol, (0.0, 0.0, 0.0), box, crop=None), tris))

            extract()
            t_ext = [timed_device(extract) for _ in range(args.reps)]
            ext_ms = float(np.median(t_ext)) / n
            r = dict(extraction=stat(t_ext, ms_per_sample=ext_ms), triangles=[int(t.shape[0]) for _, t in meshes], vertices=[int(v.shape[0]) for v, _ in meshes])
            for normals in ('face', 'field'):
                def frames():
                    for b in range(n):
                        M.render_mesh_views(meshes[b][0], meshes[b][1], cam_of(b), res, normals=normals, planes=planes[b] if normals == 'field' else None, G=G)
                frames()
                t_f = [timed_device(frames) for _ in range(args.reps)]
                ms = float(np.median(t_f)) / (n * V)
                torch.cuda.synchronize()
                tdgp._lib.profile_enable(True)
                frames()
                rep = tdgp._lib.profile_report()
                tdgp._lib.profile_enable(False)
                hits = float(np.mean([float((M.render_mesh_views(meshes[b][0], meshes[b][1], cam_of(b), res, G=G).status == 1).float().mean()) for b in range(min(n, 2))]))
                r[normals] = dict(stat(t_f, ms_per_frame=ms), kernels_ms_per_frame={k: v['total_ms'] / (n * V) for k, v in rep.items()},
                                  hit_share_first_samples=hits,
                                  break_even_frames_per_sample=(ext_ms / (shape_ms - ms)) if shape_ms > ms else None)
                say(f'{vol}^3 {normals}: {ms:.4f} ms per frame, extraction {ext_ms:.3f} ms per sample, break-even {r[normals]["break_even_frames_per_sample"]}')
            kw = dict(level=level, volume_res=vol)
            M.render_mesh_video_grid(G, ws, cams, **kw)
            t_v = [timed_device(lambda: M.render_mesh_video_grid(G, ws, cams, **kw)) for _ in range(args.reps)]
            r['video_grid_face'] = stat(t_v, over_shape_video=float(np.median(t_v)) / float(np.median(t_shape_video)))
            out[f'volume_res_{vol}'] = r
            del meshes[:]
    tdgp._lib.raise_on_device_fault('bench_mesh_frames')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

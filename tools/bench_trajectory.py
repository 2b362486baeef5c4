#!/usr/bin/env python3
"""Time trajectory rendering with shared tri-planes against the per-frame route it replaces and write profiles/trajectory_bench.json.

    python tools/bench_trajectory.py [--config c3] [--samples 16] [--frames 32] [--reps 5] [--out profiles/trajectory_bench.json]

The workload is the training snapshots' video (inference_utils.py:63-77): --samples samples x --frames `front_circle` frames around the mean
camera, at batch sizes 4 (the reference's vis_cfg) and 16.  Three parts, both routes of a part in this one process, alternating:
  frames    GPU time of all frames on the device (events on the launch stream, no host copy): the per-frame route -- `ws` repeated per camera,
            the whole `G.synthesis` per chunk of `batch` frames, as `generate_trajectory` runs it by default -- against the shared route --
            `tri_planes` on `batch` samples, `render_views` on their cameras.  plane_batch = 1 (the sample loop outermost) is timed as well.
  end2end   host clock from `ws` to a uint8 [T, GH, GW, 3] host array of the video grid: fp32 frames to the host (`generate_trajectory`), then
            make_grid, `* 255`, `.to(uint8)`, permute in torch CPU ops, against `render_video_grid(as_numpy=True)`.
  grid      tdgp_frames_to_grid_u8 alone on the frames of the whole video, in GB/s (bytes read + written), against a plain `copy_` of an fp32
            buffer of the frames' size.
One warm-up of every route first; min / median / max over the repetitions; spread = (max - min) / median.  The one condition: the shared route's
frames are faster than the per-frame route's by more than the run-to-run spreads of the two (in ms, added); the script exits non-zero otherwise.
"""
import argparse
import importlib
import json
import os
import sys
import time

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


def timed_host(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    value = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, value


def make_grid_torch(frames, nrow, padding=2):
    """torchvision.utils.make_grid(frames [n,c,h,w], nrow, padding, pad_value=0) in torch ops (torchvision itself is not required)."""
    import torch
    n, c, h, w = frames.shape
    if n == 1:
        return frames[0]
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    grid = torch.zeros([c, (h + padding) * ymaps + padding, (w + padding) * xmaps + padding], dtype=frames.dtype)
    for k in range(n):
        y0, x0 = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        grid[:, y0:y0 + h, x0:x0 + w] = frames[k]
    return grid


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default='c3', help='generator configuration (tdgp.config.config_<name>)')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip', default='', help='comma-separated parts to leave out: frames,end2end,grid')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'trajectory_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_trajectory.py measures on a GPU; none found')
    tdgp = importlib.import_module('3dgp_amd')
    I = tdgp.inference
    skip = set(args.skip.split(','))
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_trajectory] {msg}', file=sys.stderr, flush=True)                  # noqa: E731
    cfg = getattr(tdgp.config, f'config_{args.config}')()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=0))
    G = G.to(dev)
    n, V, res = args.samples, args.frames, G.synthesis.test_resolution
    inp = tdgp.weights.synthetic_inputs(cfg, batch=n, seed=1)
    z, c = torch.as_tensor(inp['z']).to(dev), torch.as_tensor(inp['c']).to(dev)
    torch.manual_seed(0)
    np.random.seed(0)
    with torch.no_grad():
        ws = G.mapping(z, c)
        cams = I.generate_camera_params(G, z, c, dict(I.SNAPSHOT_TRAJECTORY, num_frames=V)).to(dtype=torch.float32, device=dev)
    ws_rep = ws.repeat_interleave(V, dim=0)
    planes_bytes = int(np.prod(G.synthesis.tri_planes(ws[:1], noise_mode='const').t.shape)) * 4
    res_json = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, config=args.config, samples=n, frames_per_sample=V, img_resolution=res,
                    ray_steps=cfg.num_ray_steps, planes_bytes_per_sample=planes_bytes)

    def per_frame(bs):
        for b0 in range(0, n * V, bs):
            G.synthesis(ws_rep[b0:b0 + bs], camera_params=cams[b0:b0 + bs], noise_mode='const')

    def shared(pb):
        for _ in I._plane_batches(G, ws, cams, pb):
            pass

    if 'frames' not in skip:
        res_json['frames'] = {}
        for bs in (4, 16):
            per_frame(bs), shared(bs), shared(1)                                                       # warm-up
            t_old, t_new, t_one = [], [], []
            for _ in range(args.reps):
                t_old.append(timed_device(lambda: per_frame(bs)))
                t_new.append(timed_device(lambda: shared(bs)))
                t_one.append(timed_device(lambda: shared(1)))
            gain = float(np.median(t_old)) - float(np.median(t_new))
            noise = (max(t_old) - min(t_old)) + (max(t_new) - min(t_new))
            res_json['frames'][f'batch_{bs}'] = r = dict(
                per_frame=stat(t_old, frames_per_s=n * V / (float(np.median(t_old)) * 1e-3)), shared=stat(t_new, frames_per_s=n * V / (float(np.median(t_new)) * 1e-3)),
                shared_plane_batch_1=stat(t_one, frames_per_s=n * V / (float(np.median(t_one)) * 1e-3)),
                shared_over_per_frame_time=float(np.median(t_new)) / float(np.median(t_old)), gain_ms=gain, spreads_added_ms=noise,
                shared_faster_beyond_spread=bool(gain > noise))
            say(f'frames batch={bs}: per frame {r["per_frame"]["ms_median"]:.1f} ms (spread {r["per_frame"]["spread"]:.3f}), shared {r["shared"]["ms_median"]:.1f} ms '
                f'(spread {r["shared"]["spread"]:.3f}), shared with plane_batch=1 {r["shared_plane_batch_1"]["ms_median"]:.1f} ms')

    nrow = int(np.ceil(n ** 0.5))
    if 'end2end' not in skip:
        res_json['end2end'] = {}

        def old_route(bs):
            frames = I.generate_trajectory(G, ws, cams, batch_size=bs)                                # [V, n, c, h, w] fp32 in [0, 1] on the host
            video = torch.stack([make_grid_torch(g, nrow) for g in frames])
            return (video * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()

        def new_route(pb):
            return I.render_video_grid(G, ws, cams, nrow='auto', plane_batch=pb, as_numpy=True)
        for bs in (4, 16):
            old_route(bs), new_route(bs)                                                               # warm-up
            t_old, t_new = [], []
            for _ in range(max(2, args.reps // 2)):
                t, a = timed_host(lambda: old_route(bs))
                t_old.append(t)
                t, b = timed_host(lambda: new_route(bs))
                t_new.append(t)
            assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (a.shape, b.shape)
            # (the two routes draw their stratified / importance samples in another order and run the backbone at another batch size: the
            #  videos agree up to that Monte-Carlo noise, not byte for byte -- byte equality on equal draws is tests/test_trajectory_gpu.py's)
            res_json['end2end'][f'batch_{bs}'] = r = dict(
                fp32_frames_to_host_then_cpu_chain=stat(t_old), device_grid_then_one_copy=stat(t_new), shape=list(b.shape),
                new_over_old_time=float(np.median(t_new)) / float(np.median(t_old)), mean_abs_byte_difference=float(np.abs(a.astype(np.int16) - b.astype(np.int16)).mean()))
            say(f'end2end batch={bs}: fp32 to host + CPU chain {r["fp32_frames_to_host_then_cpu_chain"]["ms_median"]:.0f} ms, device grid {r["device_grid_then_one_copy"]["ms_median"]:.0f} ms')

    if 'grid' not in skip:
        frames = torch.randn(n * V, res * res, 3, device=dev)
        dst = torch.empty_like(frames)
        grid = lambda: I.frames_to_grid(frames, res, res, tiles=n, images=V, stride_image=1, stride_tile=V, nrow=nrow)      # noqa: E731
        copy = lambda: dst.copy_(frames)                                                                                    # noqa: E731
        out = grid()
        copy()
        t_grid, t_copy = [], []
        for _ in range(max(args.reps, 10)):
            t_grid.append(timed_device(grid))
            t_copy.append(timed_device(copy))
        moved_grid = frames.numel() * 4 + out.numel()
        moved_copy = frames.numel() * 8
        res_json['grid'] = r = dict(frames_bytes=frames.numel() * 4, out_bytes=out.numel(), out_shape=list(out.shape),
                                    kernel=stat(t_grid, gb_per_s=moved_grid / (float(np.median(t_grid)) * 1e-3) / 1e9),
                                    copy_=stat(t_copy, gb_per_s=moved_copy / (float(np.median(t_copy)) * 1e-3) / 1e9))
        say(f'grid: kernel {r["kernel"]["ms_median"]:.3f} ms = {r["kernel"]["gb_per_s"]:.0f} GB/s, copy_ {r["copy_"]["ms_median"]:.3f} ms = {r["copy_"]["gb_per_s"]:.0f} GB/s')
    tdgp._lib.raise_on_device_fault('bench_trajectory')

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res_json, f, indent=1)
    print(json.dumps(res_json))
    slower = [k for k, v in res_json.get('frames', {}).items() if not v['shared_faster_beyond_spread']]
    if slower:
        raise SystemExit(f'bench_trajectory: the shared-planes route is not faster than the per-frame route beyond the spread: {slower} '
                         '(the planes of a batch may be evicting each other from the cache: compare shared_plane_batch_1)')


if __name__ == '__main__':
    main()

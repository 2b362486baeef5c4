#!/usr/bin/env python3
"""Measure the deep field kernels (3- and 4-layer tri-plane decoders) against the routes next to them.

    python tools/bench_field_deep.py [--reps 9] [--inner 8] [--out profiles/field_deep_bench.json]

Forward, one C3 ray chunk (B = 1, 256^2 rays of a camera on the unit sphere, S = 64 stratified depths, planes 512^2 x 96, F 32 / hid 64), for
n_layers 3 and 4: (1) tdgp_triplane_field_deep, (2) the eager route `renderer._field_eager` -- tdgp_triplane_features + the layers as tensor
ops, what these decoders ran through before the kernel existed --, (3) for scale, the two-layer kernel tdgp_triplane_field on the same rays.
Backward, the training shape (batch 8, 64^2 patch, 32 + 32 samples = 2.1 M points, planes 512^2 x 96 per sample): tdgp_triplane_field_deep_grad
for n_layers 3 and 4 next to the two-layer tdgp_triplane_field_grad (no eager baseline exists: the backward raised for these decoders).
Each figure is the median (and the minimum and maximum) over `--reps` windows of `--inner` calls, host clock around work that ends in a device
synchronise, after a warm-up of every route; the routes alternate inside a repetition so that drift hits them alike.  Peak device memory of
a forward route = torch's peak allocation above the inputs.  Outputs of the kernel and the eager route are compared at the timed size.
Seeded random weights and planes.  Needs a GPU; there is no fallback.
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
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=8)
    ap.add_argument('--plane-res', type=int, default=512)
    ap.add_argument('--rays', type=int, default=256, help='side of the ray image of the forward chunk')
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--train-batch', type=int, default=8)
    ap.add_argument('--train-patch', type=int, default=64)
    ap.add_argument('--train-steps', type=int, default=64, help='coarse + fine samples per ray in training')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'field_deep_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_field_deep needs a GPU')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    R = tdgp.renderer
    dev = 'cuda'
    sync = torch.cuda.synchronize
    F, hid, H = 32, 64, args.plane_res
    rs = np.random.RandomState(3)

    def T(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)

    def mlp_of(n):
        m = R.TriPlaneMLP(F, hid, 3, 'classical', n_layers=n)
        with torch.no_grad():
            for fc in m.model:
                fc.weight.copy_(torch.as_tensor(rs.randn(*fc.weight.shape).astype(np.float32)))
                fc.bias.copy_(torch.as_tensor(0.3 * rs.randn(*fc.bias.shape).astype(np.float32)))
        return m.to(dev)

    def window(fn):
        sync()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        sync()
        return (time.perf_counter() - t0) * 1e3 / args.inner

    def timed(routes):
        """routes: {name: fn} -> {name: dict(ms, min_ms, max_ms)}; the routes alternate inside every repetition."""
        for fn in routes.values():
            fn(); fn()
        sync()
        samples = {k: [] for k in routes}
        for _ in range(args.reps):
            for k, fn in routes.items():
                samples[k].append(window(fn))
        return {k: dict(ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in samples.items()}

    def peak_mb(fn):
        sync()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        sync()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return peak / 2 ** 20

    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, inner=args.inner, feat_dim=F, hid_dim=hid, plane_res=H,
                  note='seeded random weights and planes; times are per call, median over reps of windows of `inner` calls')
    mlps = {n: mlp_of(n) for n in (2, 3, 4)}
    # ---- forward: one ray chunk
    hw = R.planes_to_hwc(torch.randn([1, 3 * F, H, H], device=dev, generator=torch.Generator(device=dev).manual_seed(5)))
    side, S = args.rays, args.steps
    cam = dict(angles=T([[0.3, 1.4, 0.0]]), radius=T([1.0]), look_at=T([[0.0, 0.0, 0.0]]))
    ray_o, ray_d = R.sample_rays(R.compute_cam2world_matrix(cam), fov=18.0, resolution=(side, side))
    u = torch.rand([1, side * side, S], device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    t = 0.75 + 0.5 * (torch.arange(S, device=dev).float() + u) / S                      # stratified depths in [ray_start, ray_end]
    fwd = dict(points=side * side * S, rays=side * side, steps=S)
    packs = {2: R._mlp_params(mlps[2]), 3: R._mlp_params_deep(mlps[3]), 4: R._mlp_params_deep(mlps[4])}
    kernel = {n: (lambda n=n: R._field(hw, packs[n], 0.5, ray_o=ray_o, ray_d=ray_d, t=t, ray_w=side)) for n in (2, 3, 4)}
    eager = {n: (lambda n=n: R._field_eager(hw, mlps[n], 0.5, ray_o=ray_o, ray_d=ray_d, t=t)) for n in (3, 4)}
    times = timed({'two_layer_kernel': kernel[2], 'deep_kernel_n3': kernel[3], 'eager_n3': eager[3], 'deep_kernel_n4': kernel[4], 'eager_n4': eager[4]})
    fwd['times'] = times
    for n in (3, 4):
        a, b = kernel[n](), eager[n]()
        fwd[f'n{n}'] = dict(speedup_vs_eager=times[f'eager_n{n}']['ms'] / times[f'deep_kernel_n{n}']['ms'],
                            ratio_to_two_layer_kernel=times[f'deep_kernel_n{n}']['ms'] / times['two_layer_kernel']['ms'],
                            max_abs_diff_kernel_vs_eager=float((a - b).abs().max()), max_abs_output=float(b.abs().max()),
                            peak_mb_deep_kernel=peak_mb(kernel[n]), peak_mb_eager=peak_mb(eager[n]))
        del a, b
    result['forward'] = fwd
    del hw, ray_o, ray_d, t, u
    torch.cuda.empty_cache()
    # ---- backward: the training shape
    B, P = args.train_batch, args.train_patch ** 2 * args.train_steps
    gen = torch.Generator(device=dev).manual_seed(7)
    hwb = R.planes_to_hwc(torch.randn([B, 3 * F, H, H], device=dev, generator=gen))
    coords = (torch.rand([B, P, 3], device=dev, generator=gen) * 2 - 1) * 0.55
    d_rgb, d_sigma = torch.randn([B, P, 3], device=dev, generator=gen), torch.randn([B, P, 1], device=dev, generator=gen)
    grad = {n: (lambda n=n: R.simple_tri_plane_renderer_backward(hwb, coords, mlps[n], d_rgb, d_sigma, scale=0.5)) for n in (2, 3, 4)}
    result['backward'] = dict(points=B * P, batch=B, patch=args.train_patch, samples_per_ray=args.train_steps, includes='zeroing of the plane gradient (805 MB at the defaults)',
                              times=timed({'two_layer_grad': grad[2], 'deep_grad_n3': grad[3], 'deep_grad_n4': grad[4]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(result) + '\n')             # one JSON line
    print(json.dumps(result))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Time the ADA augmentation pipe on the HIP kernels against the eager chain (tests/augment_reference.py) on the same GPU.

Shapes [16,4,64,64] (the training patch) and [16,4,256,256]; the reference's default probability list at p = 1, random draws.  Timed:
  forward            pipe.apply(x, params)                 vs  the eager pad / upsample / grid_sample / downsample / colour chain
  forward + adjoint  the same plus dx for a given dy       vs  the eager chain's autograd backward
  Dmain + Dreg       one StyleGAN2Loss phase pair at the smallest discriminator of the loss tests, with and without the pipe
Both routes take the SAME parameters (the kernel route's `params()` launch is timed separately; the eager route's ~100 tiny parameter ops
are left out of its figure, in its favour).  Method: the two routes alternate inside one process, warmed up, device events around `--iters`
iterations, `--repeats` such blocks; median, minimum and maximum of the blocks are reported.  Launch counts and copies are not measured
here: they come from a `rocprofv3 --kernel-trace` run of their own (`--trace-only` runs each route once for that).

  python tools/bench_augment.py [--iters 100] [--repeats 5] [--out profiles/augment_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import augment_reference as R  # noqa: E402

tdgp = importlib.import_module('3dgp_amd')
DEV = 'cuda:0'


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def compare(routes, iters, repeats, warmup=10):
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():                              # alternated: both routes see the same clocks
            ms[k].append(timed(fn, iters))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def bench_shape(shape, iters, repeats):
    A = tdgp.augment
    pipe = A.AugmentPipe(**R.BASE).to(DEV)
    B, C, H, W = shape
    torch.manual_seed(1)
    x = torch.randn(shape, device=DEV)
    dy = torch.randn(shape, device=DEV)
    p = pipe.params(B, H, W, num_channels=C)
    f = pipe.Hz_geom
    xg = x.clone().requires_grad_(True)

    def hip_fwd():
        with torch.no_grad():
            return pipe.apply(x, p, 3)

    def eager_fwd():
        with torch.no_grad():
            return R.apply_reference(x, p, 3, f)

    def hip_both():
        return torch.autograd.grad(pipe.apply(xg, p, 3), xg, dy)

    def eager_both():
        return torch.autograd.grad(R.apply_reference(xg, p, 3, f), xg, dy)

    err = float((hip_fwd() - eager_fwd()).abs().max())
    out = dict(shape=list(shape), max_abs_difference_of_the_two_routes=err,
               params_launch=compare(dict(hip=lambda: pipe.params(B, H, W, num_channels=C)), iters, repeats),
               forward=compare(dict(hip=hip_fwd, eager=eager_fwd), iters, repeats),
               forward_adjoint=compare(dict(hip=hip_both, eager=eager_both), iters, repeats))
    for k in ('forward', 'forward_adjoint'):
        out[k]['eager_over_hip'] = out[k]['eager']['median_ms'] / out[k]['hip']['median_ms']
    return out


def bench_loss(iters, repeats):
    """Dmain + Dreg at the loss tests' generator / discriminator (tests/golden/loss.npz for the inputs), with and without the pipe."""
    g = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'loss.npz')))
    TR = tdgp.training
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)      # noqa: E731
    cfg = tdgp.config.config_tiny()
    cfg.use_noise = False
    cfg.patch_resolution = 16
    dcfg = tdgp.discriminator.DiscriminatorConfig(c_dim=0, cbase=256, cmax=16, patch_params_cond=True, hyper_mod=True, mbstd_group_size=2)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=201, exercise_all=True))
    G = G.to(DEV).train().requires_grad_(False)
    D = tdgp.discriminator.seeded_discriminator(dcfg, 16, 3, seed=202).to(DEV).train().requires_grad_(True)
    pcfg = TR.PatchConfig(enabled=True, distribution='uniform', resolution=16, min_scale_trg=0.5, max_scale=1.0, anneal_kimg=10, mbstd_group_size=2)
    kw = dict(r1_gamma=2.0, patch_cfg=pcfg, synthesis_kwargs=dict(u_coarse=T(g['u_coarse']), u_fine=T(g['u_fine'])))
    pipe = tdgp.augment.AugmentPipe(**R.BASE).to(DEV)
    c0 = torch.zeros(4, 0, device=DEV)
    real = tdgp.generator.TensorGroup(img=T(g['real']), c=c0, depth=torch.zeros(4, 1, 32, 32, device=DEV))
    gen = tdgp.generator.TensorGroup(z=T(g['z']), c=c0, camera_params=tdgp.generator.TensorGroup(**{k[4:]: T(v) for k, v in g.items() if k.startswith('cam_')}))

    def pair(loss):
        def fn():
            D.zero_grad(set_to_none=True)
            loss.accumulate_gradients('Dmain', real, gen, gain=1, cur_nimg=0)
            loss.accumulate_gradients('Dreg', real, gen, gain=16, cur_nimg=0)
            pipe.ada_stats = None
        return fn
    res = compare(dict(without_pipe=pair(TR.StyleGAN2Loss(G, D, DEV, **kw)), with_pipe=pair(TR.StyleGAN2Loss(G, D, DEV, augment_pipe=pipe, **kw))),
                  max(iters // 5, 10), repeats, warmup=3)
    res['pipe_cost_ms'] = res['with_pipe']['median_ms'] - res['without_pipe']['median_ms']
    res['note'] = 'batch 4, 16x16 patches, 3 channels: three pipe calls (two in Dmain, one in Dreg) and their adjoints, Dreg to second order'
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'augment_bench.json'))
    ap.add_argument('--trace-only', choices=['hip', 'eager'], help='run one forward + adjoint of one route at [16,4,64,64] and exit (for rocprofv3 --kernel-trace)')
    args = ap.parse_args()
    tdgp._lib.load()
    if args.trace_only:
        pipe = tdgp.augment.AugmentPipe(**R.BASE).to(DEV)
        torch.manual_seed(1)
        x = torch.randn(16, 4, 64, 64, device=DEV).requires_grad_(True)
        torch.cuda.synchronize()
        if args.trace_only == 'hip':
            y = pipe(x, 3)
        else:
            y = R.apply_reference(x, pipe.params(16, 64, 64, num_channels=4), 3, pipe.Hz_geom)
        torch.autograd.grad(y, x, torch.ones_like(y))
        torch.cuda.synchronize()
        return
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, repeats=args.repeats,
               shapes=[bench_shape(s, args.iters, args.repeats) for s in ((16, 4, 64, 64), (16, 4, 256, 256))], loss_pair=bench_loss(args.iters, args.repeats))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()

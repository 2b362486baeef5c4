#!/usr/bin/env python3
"""Time the step tail of a training phase -- eager (`training.optimizer_step`, `training.update_ema`) against fused
(`step_tail.FusedStepTail`, `step_tail.fused_update_ema`) -- on the parameter sets of the C3 generator and of its patch discriminator, and
one whole `training.train_iteration` at batch 32 / 64^2 patches with each.

Two figures per route, per the protocol of DESIGN.md section 8:
  device_ms   device events around `--iters` calls, i.e. the time the stream needs for one call INCLUDING the gaps in which it waits for
              the host to enqueue; when a route is bound by its launches this is its enqueue time
  enqueue_ms  host clock around the same calls without a synchronisation: what the Python thread spends before it can go on
The two routes alternate inside one process on the same gradients, warmed up; median, minimum and maximum of `--repeats` blocks.  The tail
runs on synthetic gradients (no forward is needed to time it): every call first points `p.grad` at the same pre-drawn tensors, in both routes.

  python tools/bench_train_step.py [--iters 20] [--repeats 5] [--out profiles/train_step_bench.json] [--skip-iteration]
"""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
tdgp = importlib.import_module('3dgp_amd')
DEV = 'cuda:0'


def timed(fn, iters):
    """-> (device ms per call, host enqueue ms per call)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    t1 = time.perf_counter()
    b.synchronize()
    return a.elapsed_time(b) / iters, (t1 - t0) * 1e3 / iters


def compare(routes, iters, repeats, warmup=3):
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    dev, enq = {k: [] for k in routes}, {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():                              # alternated: both routes see the same clocks
            d, e = timed(fn, iters)
            dev[k].append(d)
            enq[k].append(e)
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))      # noqa: E731
    out = {k: dict(device=stat(dev[k]), enqueue=stat(enq[k])) for k in routes}
    if 'eager' in out and 'fused' in out:
        out['eager_over_fused'] = dict(device=out['eager']['device']['median_ms'] / out['fused']['device']['median_ms'],
                                       enqueue=out['eager']['enqueue']['median_ms'] / out['fused']['enqueue']['median_ms'])
    return out


def networks(patch=64):
    cfg = tdgp.config.config_c3()
    cfg.patch_resolution = patch
    dcfg = tdgp.discriminator.DiscriminatorConfig(c_dim=cfg.c_dim, patch_params_cond=True, hyper_mod=True)
    G = tdgp.generator.Generator(cfg).to(DEV).train().requires_grad_(False)
    D = tdgp.discriminator.Discriminator(dcfg, input_resolution=patch, img_channels=3).to(DEV).train().requires_grad_(False)
    return cfg, G, D


def bench_tail(name, module, grad_clip, iters, repeats):
    mods = dict(eager=module, fused=copy.deepcopy(module))
    opts = {k: torch.optim.Adam(m.parameters(), lr=0.002, betas=(0.0, 0.99), eps=1e-8) for k, m in mods.items()}
    tail = tdgp.step_tail.FusedStepTail(mods['fused'], opts['fused'])
    torch.manual_seed(1)
    grads = [torch.randn_like(p) * 1e-3 for p in module.parameters()]

    def route(kind):
        params = list(mods[kind].parameters())

        def fn():
            for p, g in zip(params, grads):
                p.grad = g
            if kind == 'eager':
                tdgp.training.optimizer_step(mods[kind], opts[kind], world=1, grad_clip=grad_clip)
            else:
                tail.step(world=1, grad_clip=grad_clip)
        return fn
    out = compare(dict(eager=route('eager'), fused=route('fused')), iters, repeats)
    diff = max(float((a - b).abs().max()) for a, b in zip(mods['eager'].parameters(), mods['fused'].parameters()))
    n = sum(p.numel() for p in module.parameters())
    out.update(what=name, tensors=len(grads), elements=n, grad_clip=grad_clip, fused_launches=tail.record['launches'],
               bytes_moved_fused=n * 4 * (2 + 2 + 7), max_abs_difference_of_the_parameters_after_all_steps=diff)
    return out


def bench_ema(G, iters, repeats):
    ema = dict(eager=copy.deepcopy(G), fused=copy.deepcopy(G))
    kw = dict(cur_nimg=10 ** 7, batch_size=32)
    out = compare(dict(eager=lambda: tdgp.training.update_ema(ema['eager'], G, **kw), fused=lambda: tdgp.step_tail.fused_update_ema(ema['fused'], G, **kw)),
                  iters, repeats)
    out.update(tensors=len(list(G.parameters())) + len(list(G.buffers())), fused_launches=1)
    return out


def bench_iteration(cfg, G, D, batch, batch_gpu, iters, repeats):
    TR, TG = tdgp.training, tdgp.generator.TensorGroup
    pcfg = TR.PatchConfig(enabled=True, resolution=cfg.patch_resolution, mbstd_group_size=4)
    out = {}
    torch.manual_seed(2)
    np.random.seed(2)
    real = TG(img=torch.randn(batch, 3, cfg.img_resolution, cfg.img_resolution, device=DEV).clamp(-1, 1), c=TR.sample_random_c(batch, cfg.c_dim, DEV),
              depth=torch.zeros(batch, 1, cfg.img_resolution, cfg.img_resolution, device=DEV))
    routes = {}
    for kind in ('eager', 'fused'):
        g, d = copy.deepcopy(G), copy.deepcopy(D)
        loss = TR.StyleGAN2Loss(g, d, DEV, patch_cfg=copy.deepcopy(pcfg))
        phases = TR.setup_phases(g, d, dict(lr=0.0025, betas=[0.0, 0.99], eps=1e-8), dict(lr=0.002, betas=[0.0, 0.99], eps=1e-8), G_reg_interval=None, D_reg_interval=16)
        n = len(phases) * batch
        gen = TG(z=torch.randn(n, cfg.z_dim, device=DEV), c=TR.sample_random_c(n, cfg.c_dim, DEV),
                 camera_params=tdgp.metrics.sample_camera_params(tdgp.metrics.camera_base(), n, DEV))
        routes[kind] = (lambda loss=loss, phases=phases, gen=gen, kind=kind:
                        TR.train_iteration(loss, phases, real, gen, batch_idx=1, cur_nimg=0, batch_size=batch, batch_gpu=batch_gpu, world=1, step_tail=kind == 'fused'))
    out = compare(routes, iters, repeats, warmup=1)
    out.update(batch=batch, batch_gpu=batch_gpu, patch=cfg.patch_resolution, phases='Gall + Dmain (batch_idx 1: no Dreg)')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'train_step_bench.json'))
    ap.add_argument('--skip-iteration', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    cfg, G, D = networks()
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, repeats=args.repeats, chunk=tdgp.step_tail.CHUNK,
               tail_G=bench_tail('C3 generator, grad_clip 10', G, 10.0, args.iters, args.repeats),
               tail_D=bench_tail('C3 patch discriminator (64^2), no clipping', D, None, args.iters, args.repeats),
               ema_G=bench_ema(G, args.iters, args.repeats))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    if not args.skip_iteration:
        res['train_iteration'] = bench_iteration(cfg, G, D, 32, 4, max(args.iters // 10, 2), min(args.repeats, 3))
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    tdgp._lib.raise_on_device_fault('bench_train_step')
    print(json.dumps({k: (v.get('eager_over_fused') if isinstance(v, dict) else v) for k, v in res.items()}))


if __name__ == '__main__':
    main()

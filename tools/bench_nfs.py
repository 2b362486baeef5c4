#!/usr/bin/env python3
"""Measure the non-flatness score's device path against the route it replaces.

    python tools/bench_nfs.py [--config config_c3] [--reps 9] [--out profiles/nfs_bench.json]

1. tdgp_quantile_select against `renderer._quantile` (torch.quantile up to 2^24 elements, torch.sort above) + the read-back, on the same
   buffers: activated densities captured from a forward of the seeded random-weight generator (tiled to the larger sizes) and a buffer with
   60 % exact zeros; also the select's kernel time (the library's per-dispatch events) against its algorithmic bytes, 3 passes x 4 n.
2. One forward with cut_quantile = 0.5 at batch 4 and 16 with the threshold from the select and from `_quantile` -- the latter is, call for
   call, what the code before the select ran -- next to the plain forward.
3. `nfs256` against the earlier loop (compute_flattened_depth_maps with the sort route, then clamp + torch.histc + entropy on the host), and the
   bytes each moves to the host per image.
Times are medians over `--reps` runs after a warm-up, host clock around work that ends in a device synchronise.  The score's VALUE comes from
seeded random weights: it says nothing about quality.  Needs a GPU; there is no fallback.
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
sys.path.insert(0, os.path.join(REPO, 'tools'))
from calc_nfs import UniformLabels  # noqa: E402

QS_KERNELS = ('qs_zero_kernel', 'qs_hist_kernel', 'qs_pick_kernel')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='config_c3')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--sizes', type=int, nargs='*', default=[4 * 21845 * 64, 4 * 21845 * 128, 1 << 24, 1 << 25])
    ap.add_argument('--num-gen', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'nfs_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_nfs needs a GPU')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    R, M, _lib = tdgp.renderer, tdgp.metrics, tdgp._lib
    cfg = getattr(tdgp.config, args.config)()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=105, exercise_all=True))
    G = G.to('cuda').eval()
    sync = torch.cuda.synchronize
    dataset = UniformLabels(cfg.c_dim) if cfg.c_dim else None

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
        return statistics.median(out), min(out), r

    select_route = R._select_threshold
    sort_route = lambda d, q: float(R._quantile(d, q))                    # noqa: E731

    def batch(n, seed=7):
        torch.manual_seed(seed)
        np.random.seed(seed)
        return next(M._generator_batches(G, n, None, None, dataset, 'cuda', frontal_camera=True))

    result = dict(config=args.config, reps=args.reps, device=torch.cuda.get_device_name(0), resolution=cfg.img_resolution, num_ray_steps=cfg.num_ray_steps,
                  note='seeded random weights: the score is not a quality figure')
    # ---- the buffers the quantile is taken over in a real forward
    captured = []
    R._select_threshold = lambda d, q: captured.append(d.reshape(-1).clone()) or select_route(d, q)
    z, c, cam = batch(4)
    G(z, c, cam, render_opts=dict(return_depth=True, cut_quantile=0.5))
    R._select_threshold = select_route
    result['quantile_calls_per_forward_b4'] = len(captured)
    result['quantile_sizes_per_forward_b4'] = [int(t.numel()) for t in captured]
    dens = torch.cat(captured[:2])
    result['density_zero_fraction'] = float((dens == 0).float().mean())
    result['density_below_1e-3_fraction'] = float((dens < 1e-3).float().mean())

    def buffer(kind, n):
        if kind == 'density':
            return dens.repeat(-(-n // dens.numel()))[:n].contiguous()
        g = torch.Generator(device='cuda').manual_seed(n % 9973)
        x = torch.rand(n, device='cuda', generator=g) + 1e-3
        x[torch.rand(n, device='cuda', generator=g) < 0.6] = 0.0
        return x

    rows = []
    for kind in ('density', 'zeros60'):
        for n in args.sizes:
            x = buffer(kind, n)
            t_sel, t_sel_min, a = timed(lambda: select_route(x, 0.5))
            t_sort, t_sort_min, b = timed(lambda: sort_route(x, 0.5))
            _lib.profile_enable(True)
            for _ in range(args.reps):
                R.quantile_select(x, 0.5)
            rep = _lib.profile_report()
            _lib.profile_enable(False)
            per_call = {k: rep[k]['total_ms'] / args.reps for k in QS_KERNELS if k in rep}
            k_ms = sum(per_call.values())
            hist_ms = per_call.get('qs_hist_kernel', 0.0)
            rows.append(dict(buffer=kind, n=n, select_ms=t_sel, select_min_ms=t_sel_min, sort_route_ms=t_sort, sort_route_min_ms=t_sort_min,
                             speedup=t_sort / t_sel, same_float=bool(np.float32(a).tobytes() == np.float32(b).tobytes()), kernels_ms_per_call=per_call,
                             kernels_sum_ms=k_ms, algorithmic_bytes=3 * 4 * n, achieved_GBps_all_kernels=3 * 4 * n / (k_ms * 1e-3) / 1e9 if k_ms else None,
                             achieved_GBps_hist_kernels=3 * 4 * n / (hist_ms * 1e-3) / 1e9 if hist_ms else None))
            del x
    result['quantile_select'] = rows
    # ---- one forward
    fwd = {}
    for b in (4, 16):
        z, c, cam = batch(b)
        f = {}
        try:
            f['plain_ms'], f['plain_min_ms'], _ = timed(lambda: G(z, c, cam, render_opts=dict(return_depth=True)))
            R._select_threshold = select_route
            f['cut_select_ms'], f['cut_select_min_ms'], o1 = timed(lambda: G(z, c, cam, render_opts=dict(return_depth=True, cut_quantile=0.5)))
            R._select_threshold = sort_route
            f['cut_sort_route_ms'], f['cut_sort_route_min_ms'], o2 = timed(lambda: G(z, c, cam, render_opts=dict(return_depth=True, cut_quantile=0.5)))
            f['cut_overhead_select_ms'] = f['cut_select_ms'] - f['plain_ms']
            f['cut_overhead_sort_route_ms'] = f['cut_sort_route_ms'] - f['plain_ms']
        except torch.OutOfMemoryError as e:                               # nothing else is survivable: a device fault is a RuntimeError too, and ends the run
            f['error'] = str(e)[:300]
        finally:
            R._select_threshold = select_route
        fwd[f'batch_gen_{b}'] = f
    result['forward'] = fwd
    # ---- the metric
    lo, hi, px = cfg.ray_start, cfg.ray_end, cfg.img_resolution ** 2

    def earlier_loop(batch_gen):
        R._select_threshold = sort_route
        try:
            d = M.compute_flattened_depth_maps(G, args.num_gen, batch_gen=batch_gen, cut_quantile=0.5, dataset=dataset).clamp(lo, hi)
        finally:
            R._select_threshold = select_route
        h = torch.stack([torch.histc(r, 64, min=lo, max=hi) for r in d])
        return float(M.compute_histogram_entropy(h).exp().mean())

    def seeded(fn):
        def run():
            torch.manual_seed(11)
            np.random.seed(11)
            return fn()
        return run
    metric = {}
    for b in (4, 16):
        m = {}
        m['nfs_ms'], m['nfs_min_ms'], s_new = timed(seeded(lambda: M.compute_flatness_score(G, args.num_gen, lo, hi, batch_gen=b, dataset=dataset)), reps=max(3, args.reps // 3), warm=1)
        m['earlier_loop_ms'], m['earlier_loop_min_ms'], s_old = timed(seeded(lambda: earlier_loop(b)), reps=max(3, args.reps // 3), warm=1)
        m.update(score=s_new, score_earlier_loop=s_old, same_score=bool(s_new == s_old), speedup=m['earlier_loop_ms'] / m['nfs_ms'])
        metric[f'batch_gen_{b}'] = m
    metric['host_bytes_per_image'] = dict(histogram=64 * 4, depth_map=px * 4)
    result['nfs'] = dict(num_gen=args.num_gen, **metric)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()

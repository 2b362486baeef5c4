#!/usr/bin/env python3
"""Time FID's statistics on the device against what they replace and write profiles/fid_stats_bench.json.

    python tools/bench_fid_stats.py [--features 2048] [--rows 50000] [--reps 5] [--loop-images 512] [--config c3] [--out profiles/fid_stats_bench.json]

Four parts, every route of a part in this one process on the same rows:
  block     one feature block (n = 64 and n = 512): tdgp_moments_add | fp64 copies on the device, `s1 += r.sum(0); s2.addmm_(r.T, r)` (rocBLAS;
            timed with and without the widening copy) | `_RawMoments.add_block` on the host (the block's copy to the host included, as
            `append_torch` pays it)
  rows      one call over a saved row set (n = --rows): the same three routes; `tflops` counts the full 2 n F^2 of the Gram product for every
            route, so that the routes compare by it; the kernel computes the tiles on and above the diagonal only, and `executed_tflops` /
            `executed_share_of_fp64_matrix_peak` count just those; the peak is 78.6 TFLOP/s, the fp64 matrix rate of AMD's MI355X data sheet
  loop      compute_feature_stats_for_generator with host statistics (stats_device=None) and with device statistics, the stand-in detector
            widened to --features, batch_gen 4 and 16, eager forwards; three repetitions of each, alternating; img/s and the spread
  distance  frechet_distance_eigh on device tensors against frechet_distance (scipy sqrtm) on the host, both values recorded
Device routes are timed by events on the launch stream around `inner` back-to-back calls, host routes by a host clock around a call that ends
in a synchronise; one warm-up of every route first; min / median / max over the repetitions.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_MATRIX_PEAK = 78.6e12


def stat(times, **more):
    return dict(ms_min=min(times), ms_median=float(np.median(times)), ms_max=max(times), reps=len(times), **more)


def timed_device(fn, reps, inner=1):
    import torch
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return times


def timed_host(fn, reps):
    import torch
    times, value = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, value


def moment_routes(M, rows, reps, host_reps, inner):
    """The three routes on one [n, F] fp32 tensor on the device -> dict of timings; the kernel's totals are checked against rocBLAS's."""
    import torch
    n, F = rows.shape
    flop = 2.0 * n * F * F
    s1 = torch.zeros([F], dtype=torch.float64, device=rows.device)
    s2 = torch.zeros([F, F], dtype=torch.float64, device=rows.device)
    b1, b2 = torch.zeros_like(s1), torch.zeros_like(s2)
    r64 = rows.double()

    def kernel():
        M._moments_add(rows, s1, s2)

    def blas():
        r = rows.double()
        b1.add_(r.sum(0))
        b2.addmm_(r.T, r)

    def blas_no_copy():
        b2.addmm_(r64.T, r64)

    def host():
        m.add_block(rows.cpu().numpy())
    kernel(), blas(), blas_no_copy()
    rel = float(((s2 - b2 + r64.T @ r64).abs().max() / b2.abs().max()).item())      # b2 holds two products by now, s2 one
    out = dict(n=n, features=F, gram_flop=flop, kernel_vs_rocblas_max_rel=rel)
    tk, tb, tn = [], [], []
    for _ in range(reps):                                          # alternate, so that a drift of the machine shows in every route
        tk += timed_device(kernel, 1, inner)
        tb += timed_device(blas, 1, inner)
        tn += timed_device(blas_no_copy, 1, inner)
    for name, t in (('kernel', tk), ('rocblas_with_fp64_copy', tb), ('rocblas_addmm_only', tn)):
        ms = float(np.median(t))
        out[name] = stat(t, tflops=flop / (ms * 1e-3) / 1e12, share_of_fp64_matrix_peak=flop / (ms * 1e-3) / FP64_MATRIX_PEAK)
    # the kernel's own work: 64 x 64 tiles on and above the diagonal only (padded to whole tiles), about half of the full product
    t1 = -(-F // 64)
    out['kernel']['executed_flop'] = done = 2.0 * n * (t1 * (t1 + 1) // 2) * 64 * 64
    out['kernel']['executed_tflops'] = done / (out['kernel']['ms_median'] * 1e-3) / 1e12
    out['kernel']['executed_share_of_fp64_matrix_peak'] = done / (out['kernel']['ms_median'] * 1e-3) / FP64_MATRIX_PEAK
    if host_reps > 0:
        m = M._RawMoments(F)
        th, _ = timed_host(host, host_reps)
        out['host_numpy'] = stat(th, tflops=flop / (float(np.median(th)) * 1e-3) / 1e12)
    out['workspace_bytes'] = int(importlib.import_module('3dgp_amd._lib').load().tdgp_moments_workspace_bytes(n, F))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--features', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--loop-images', type=int, default=512)
    ap.add_argument('--config', default='c3', help='generator configuration of the loop (tdgp.config.config_<name>)')
    ap.add_argument('--skip', default='', help='comma-separated parts to leave out: block,rows,loop,distance')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'fid_stats_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_fid_stats.py measures on a GPU; none found')
    tdgp = importlib.import_module('3dgp_amd')
    M, D = tdgp.metrics, tdgp.distributed
    skip = set(args.skip.split(','))
    dev = torch.device('cuda:0')
    F = args.features
    say = lambda msg: print(f'[bench_fid_stats] {msg}', file=sys.stderr, flush=True)                # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, features=F, fp64_matrix_peak_tflops=FP64_MATRIX_PEAK / 1e12)
    g = torch.Generator(device=dev).manual_seed(0)

    if 'block' not in skip:
        res['block'] = {}
        for n in (64, 512):
            rows = torch.randn(n, F, device=dev, generator=g)
            res['block'][str(n)] = r = moment_routes(M, rows, args.reps, 3, inner=20)
            say(f'block n={n}: kernel {r["kernel"]["ms_median"]:.3f} ms, rocBLAS+copy {r["rocblas_with_fp64_copy"]["ms_median"]:.3f} ms, '
                f'addmm only {r["rocblas_addmm_only"]["ms_median"]:.3f} ms, host {r["host_numpy"]["ms_median"]:.1f} ms')
    if 'rows' not in skip:
        rows = torch.randn(args.rows, F, device=dev, generator=g)
        res['rows'] = r = moment_routes(M, rows, args.reps, 1, inner=1)
        say(f'rows n={args.rows}: kernel {r["kernel"]["ms_median"]:.2f} ms ({r["kernel"]["tflops"]:.1f} TFLOP/s), rocBLAS+copy '
            f'{r["rocblas_with_fp64_copy"]["ms_median"]:.2f} ms, addmm only {r["rocblas_addmm_only"]["ms_median"]:.2f} ms, host {r["host_numpy"]["ms_median"]:.0f} ms')
        del rows

    if 'loop' not in skip:
        cfg = getattr(tdgp.config, f'config_{args.config}')()
        G = tdgp.generator.Generator(cfg)
        G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=0))
        G = G.to(dev)
        det = lambda im: D.stand_in_features(im, F)                                                  # noqa: E731
        labels = None                                                                                # a conditional generator: random one-hot labels (datasets are out of scope)
        if G.c_dim:
            labels = lambda b: torch.nn.functional.one_hot(torch.randint(G.c_dim, (b,)), G.c_dim).float()      # noqa: E731
        res['loop'] = dict(config=args.config, images=args.loop_images, batch_size=64, launch='eager')

        def loop(batch_gen, stats_device):
            torch.manual_seed(1)
            np.random.seed(1)
            st = M.compute_feature_stats_for_generator(G, det, max_items=args.loop_images, batch_size=64, batch_gen=batch_gen, device=dev, capture_mean_cov=True,
                                                       c_sampler=labels, stats_device=stats_device)
            return st.get_mean_cov()
        for bg in (4, 16):
            loop(bg, None), loop(bg, dev)                                                            # warm-up
            th, td = [], []
            for _ in range(3):
                t, (mh, ch) = timed_host(lambda: loop(bg, None), 1)
                th += t
                t, (md, cd) = timed_host(lambda: loop(bg, dev), 1)
                td += t
            ips = lambda t: args.loop_images / (float(np.median(t)) * 1e-3)                         # noqa: E731
            spread = lambda t: (max(t) - min(t)) / float(np.median(t))                               # noqa: E731
            res['loop'][f'batch_gen_{bg}'] = r = dict(
                host_stats=stat(th, img_per_s=ips(th), spread=spread(th)), device_stats=stat(td, img_per_s=ips(td), spread=spread(td)),
                device_over_host_time=float(np.median(td)) / float(np.median(th)),
                device_not_slower_within_spread=bool(float(np.median(td)) <= float(np.median(th)) * (1.0 + max(spread(th), spread(td)))),
                cov_max_abs_diff=float(np.abs(cd - ch).max()), cov_max_abs=float(np.abs(ch).max()))
            say(f'loop batch_gen={bg}: host stats {r["host_stats"]["img_per_s"]:.1f} img/s (spread {r["host_stats"]["spread"]:.3f}), device stats '
                f'{r["device_stats"]["img_per_s"]:.1f} img/s (spread {r["device_stats"]["spread"]:.3f})')
        del G

    if 'distance' not in skip:
        rs = np.random.RandomState(0)
        a = rs.randn(3 * F, F)
        b = rs.randn(3 * F, F) @ (np.eye(F) + 0.05 * rs.randn(F, F)) + 0.1
        (mu_a, s_a), (mu_b, s_b) = ((x.mean(0), np.cov(x, rowvar=False)) for x in (a, b))
        on = [torch.from_numpy(x).to(dev) for x in (mu_a, s_a, mu_b, s_b)]
        M.frechet_distance_eigh(*on)                                                                 # warm-up (solver handles)
        te, ve = timed_host(lambda: M.frechet_distance_eigh(*on), 3)
        tc, vc = timed_host(lambda: M.frechet_distance_eigh(mu_a, s_a, mu_b, s_b), 1)
        ts, vs = timed_host(lambda: M.frechet_distance(mu_a, s_a, mu_b, s_b), 1)
        res['distance'] = dict(features=F, eigh_device=stat(te, value=ve), eigh_host=stat(tc, value=vc), sqrtm_host=stat(ts, value=vs),
                               rel_diff_device_vs_sqrtm=abs(ve - vs) / max(1.0, abs(vs)))
        say(f'distance: eigh on the device {np.median(te):.0f} ms ({ve!r}), eigh on the host {np.median(tc):.0f} ms, sqrtm on the host {np.median(ts):.0f} ms ({vs!r})')

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    # the one timing that must hold: device statistics may not slow the loop down by more than the run-to-run spread
    slower = [k for k, v in res.get('loop', {}).items() if isinstance(v, dict) and not v['device_not_slower_within_spread']]
    for k, v in res.get('loop', {}).items():
        if isinstance(v, dict):
            say(f'loop {k}: device / host time {v["device_over_host_time"]:.3f}, spreads {v["host_stats"]["spread"]:.3f} / {v["device_stats"]["spread"]:.3f}: '
                f'{"ok" if k not in slower else "DEVICE STATISTICS SLOWER THAN HOST STATISTICS BEYOND THE SPREAD"}')
    if slower:
        raise SystemExit(f'bench_fid_stats: the loop with device statistics is slower than with host statistics beyond the spread: {slower}')


if __name__ == '__main__':
    main()

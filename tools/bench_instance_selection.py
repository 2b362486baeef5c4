#!/usr/bin/env python3
"""Time instance selection's scores on the device against what they replace and write profiles/instance_selection_bench.json.

    python tools/bench_instance_selection.py [--shapes 1300x2048,50000x2048] [--reg-covar 1e-05] [--reps 5] [--torch-chunk 16384] [--out profiles/instance_selection_bench.json]

Per shape, every route in this one process on the same rows (rectified-Gaussian features made on the device, a fixed seed):
  kernel   the route of 3dgp_amd/instance_selection.py, stage by stage: moments (tdgp_moments_add), factorisation (covariance, cholesky_ex,
           solve_triangular, log-determinant, with its read-backs), scores (tdgp_gaussian_maha + the score's epilogue), sort (select_instances,
           keep ratio 0.5); `maha_kernel` is the kernel alone: its FLOP are the ones it executes (the K loop of column tile tj stops at
           64 (tj + 1), padded to whole tiles and K steps) and the peak is 78.6 TFLOP/s, the fp64 matrix rate of AMD's MI355X data sheet
  torch    the same factor L, then `solve_triangular(L, (X - mu)^T)` in fp64 over chunks of --torch-chunk rows and a square-sum; its peak
           memory above the resident rows is recorded next to the kernel route's
  sklearn  `GaussianMixture(1, reg_covar).fit(X).score_samples(X)` on the host, float32 as the reference calls it, where scikit-learn imports
Device stages are timed by events on the launch stream, routes that read back by a host clock around a call that ends in a synchronise; one
warm-up of every route, then --reps blocks in which the routes alternate; min / median / max and the spread (max - min) / median.
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
    med = float(np.median(times))
    return dict(ms_min=min(times), ms_median=med, ms_max=max(times), spread=(max(times) - min(times)) / med if med > 0 else 0.0, reps=len(times), **more)


def executed_flop(n, F):
    t1 = -(-F // 64)
    k_sum = sum(-(-min(F, 64 * (tj + 1)) // 32) * 32 for tj in range(t1))
    return 2.0 * (-(-n // 64) * 64) * 64 * k_sum


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--shapes', default='1300x2048,50000x2048')
    ap.add_argument('--reg-covar', type=float, default=1e-5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-chunk', type=int, default=16384)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'instance_selection_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_instance_selection.py measures on a GPU; none found')
    tdgp = importlib.import_module('3dgp_amd')
    M, S, L_ = tdgp.metrics, tdgp.instance_selection, tdgp._lib
    dev = torch.device('cuda:0')
    say = lambda msg: print(f'[bench_instance_selection] {msg}', file=sys.stderr, flush=True)      # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reg_covar=args.reg_covar, fp64_matrix_peak_tflops=FP64_MATRIX_PEAK / 1e12,
               torch_chunk=args.torch_chunk, shapes={})
    try:
        GaussianMixture = None if args.no_sklearn else importlib.import_module('sklearn.mixture').GaussianMixture
    except ImportError:
        GaussianMixture = None

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for shape in args.shapes.split(','):
        n, F = (int(v) for v in shape.split('x'))
        g = torch.Generator(device=dev).manual_seed(0)
        mix = torch.eye(F, device=dev) + 0.15 * torch.randn(F, F, device=dev, generator=g) / F ** 0.5
        rows = torch.clamp_min(torch.randn(n, F, device=dev, generator=g) @ mix + 0.6 * torch.rand(F, device=dev, generator=g), 0.0).contiguous()
        del mix
        log2pi = F * float(np.log(2.0 * np.pi))
        eye = torch.eye(F, dtype=torch.float64, device=dev)
        keep = n // 2

        def kernel_stages():
            """-> (stage times in ms, scores, (mu, L, P))"""
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            torch.cuda.synchronize()
            marks[0].record()
            m = M._DeviceMoments(F, dev)
            m.add_block(rows)
            marks[1].record()
            finite = bool((torch.isfinite(m.s1).all() & torch.isfinite(m.s2).all()).item())
            mu, cov = m.central(n)
            cov.diagonal().add_(args.reg_covar)
            L, info = torch.linalg.cholesky_ex(cov)
            assert finite and int(info.item()) == 0
            P = torch.linalg.solve_triangular(L, eye, upper=False).T.contiguous()
            log_det = torch.log(P.diagonal()).sum()
            marks[2].record()
            scores = -0.5 * (log2pi + S._maha_device(rows, mu, P)) + log_det
            marks[3].record()
            order = S.select_instances(scores, keep)
            marks[4].record()
            marks[4].synchronize()
            t = [marks[i].elapsed_time(marks[i + 1]) for i in range(4)]
            return dict(moments=t[0], factorisation=t[1], scores=t[2], sort=t[3], total=sum(t)), scores, (mu.contiguous(), L, P), order

        def torch_scores(mu, L):
            out = torch.empty([n], dtype=torch.float64, device=dev)
            for a in range(0, n, args.torch_chunk):
                y = torch.linalg.solve_triangular(L, (rows[a:a + args.torch_chunk].double() - mu).T, upper=False)
                out[a:a + args.torch_chunk] = (y * y).sum(0)
            return out

        def peak_of(fn):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - base, out

        # warm-up of every route; the factor is shared by the two maha routes
        _, scores, (mu, L, P), _ = kernel_stages()
        peak_kernel, maha_k = peak_of(lambda: S._maha_device(rows, mu, P))
        peak_torch, maha_t = peak_of(lambda: torch_scores(mu, L))
        rel = float(((maha_k - maha_t).abs() / maha_t.abs().clamp_min(1e-300)).max().item())
        whole = S.compute_gaussian_ll_scores(rows, reg_covar=args.reg_covar, device=dev)
        assert float((whole - scores).abs().max().item()) <= 1e-9

        stages = {k: [] for k in ('moments', 'factorisation', 'scores', 'sort', 'total')}
        tk, tt, tw = [], [], []
        for _ in range(args.reps):                                   # alternate, so that a drift of the machine shows in every route
            st, _, _, _ = kernel_stages()
            for k, v in st.items():
                stages[k].append(v)
            a, b = events()
            a.record()
            S._maha_device(rows, mu, P)
            b.record()
            b.synchronize()
            tk.append(a.elapsed_time(b))
            a, b = events()
            a.record()
            torch_scores(mu, L)
            b.record()
            b.synchronize()
            tt.append(a.elapsed_time(b))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.select_instances(S.compute_gaussian_ll_scores(rows, reg_covar=args.reg_covar, device=dev), keep)
            torch.cuda.synchronize()
            tw.append((time.perf_counter() - t0) * 1e3)
        flop = executed_flop(n, F)
        ms = float(np.median(tk))
        r = dict(n=n, features=F, mode={0: 'direct', 1: 'split'}[int(L_.load().tdgp_gaussian_maha_mode(n, F))],
                 workspace_bytes=int(L_.load().tdgp_gaussian_maha_workspace_bytes(n, F)),
                 kernel_route_stages={k: stat(v) for k, v in stages.items()},
                 kernel_route_whole_call=stat(tw),
                 maha_kernel=stat(tk, executed_flop=flop, executed_tflops=flop / (ms * 1e-3) / 1e12,
                                  executed_share_of_fp64_matrix_peak=flop / (ms * 1e-3) / FP64_MATRIX_PEAK, peak_bytes_above_rows=int(peak_kernel)),
                 maha_torch=stat(tt, peak_bytes_above_rows=int(peak_torch)),
                 kernel_over_torch_time=ms / float(np.median(tt)), kernel_vs_torch_max_rel=rel)
        say(f'{shape}: kernel {ms:.3f} ms ({r["maha_kernel"]["executed_tflops"]:.1f} TFLOP/s executed, {r["maha_kernel"]["executed_share_of_fp64_matrix_peak"]:.3f} of peak, '
            f'spread {r["maha_kernel"]["spread"]:.3f}), torch {np.median(tt):.3f} ms (peak {peak_torch / 2 ** 20:.0f} MiB vs {peak_kernel / 2 ** 20:.1f} MiB), '
            f'stages {", ".join(f"{k} {np.median(v):.2f}" for k, v in stages.items())} ms, whole call {np.median(tw):.2f} ms, max rel diff {rel:.2e}')
        if GaussianMixture is not None:
            x = rows.cpu().numpy()
            t0 = time.perf_counter()
            gmm = GaussianMixture(n_components=1, reg_covar=args.reg_covar)
            gmm.fit(x)
            ref = gmm.score_samples(x)
            r['sklearn_host_float32'] = dict(ms=(time.perf_counter() - t0) * 1e3, reps=1, max_abs_diff_to_device_scores=float(np.abs(ref - scores.cpu().numpy()).max()))
            say(f'{shape}: scikit-learn on the host {r["sklearn_host_float32"]["ms"]:.0f} ms, max |score difference| {r["sklearn_host_float32"]["max_abs_diff_to_device_scores"]:.2e}')
        res['shapes'][shape] = r
        del rows, eye, mu, L, P, scores, maha_k, maha_t, whole

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

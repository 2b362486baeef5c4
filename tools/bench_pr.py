#!/usr/bin/env python3
"""Time precision / recall at the 'pr50k3_full' shape (50 000 + 50 000 rows, F = 4096, k = 3; random features resident on the device) and
write profiles/pr_bench.json.

    python tools/bench_pr.py [--rows 50000] [--features 4096] [--reps 5] [--host-reps 1] [--out profiles/pr_bench.json]

Three routes on the same features:
  kernel        tdgp.metrics.compute_pr: pack + four tile passes on the fp16 matrix pipe + merges; nothing but two floats leaves the device
  torch_device  the reference's algorithm kept on the device: torch.cdist in fp16 over 10 000 x 10 000 blocks, kthvalue, <= (no host copies)
  torch_host    the reference as written (src/metrics/precision_recall.py): every distance block copied to the host, kthvalue / <= there
Wall times are device events on the launch stream around whole calls (the host route: a host clock around a call that ends in a
synchronise), after one warm-up of every route; min / median / max over the repetitions.  The per-kernel figures are the library's
per-dispatch events in a profiled run of their own.  FLOP = 2 N^2 F per pass; the share of peak is against 2.5 PFLOP/s dense fp16.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP16_PEAK = 2.5e15
BLOCK = 10000                           # the reference's row_batch_size / col_batch_size


def torch_route(real, gen, k, host):
    """precision_recall.py:49-59 with num_gpus = 1; `host` keeps its `.cpu()` on every distance block."""
    import torch
    out = []
    for manifold, probes in ((real, gen), (gen, real)):
        def distances(rows):
            blocks = [torch.cdist(rows.unsqueeze(0), cols.unsqueeze(0))[0] for cols in manifold.split(BLOCK)]
            return torch.cat([b.cpu() for b in blocks] if host else blocks, dim=1)
        kth = torch.cat([distances(rows).to(torch.float32).kthvalue(k + 1).values.to(torch.float16) for rows in manifold.split(BLOCK)])
        pred = torch.cat([(distances(rows) <= kth).any(dim=1) for rows in probes.split(BLOCK)])
        out.append(float(pred.to(torch.float32).mean()))
    return tuple(out)


def timed(fn, reps, host_clock=False):
    import torch
    times, value = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        if host_clock:
            t0 = time.perf_counter()
            value = fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            value = fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
    return dict(ms_min=min(times), ms_median=float(np.median(times)), ms_max=max(times), reps=reps), value


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--features', type=int, default=4096)
    ap.add_argument('--nhood-size', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=1, help='repetitions of the route with host copies (0 skips it)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pr_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_pr.py measures on a GPU; none found')
    tdgp = importlib.import_module('3dgp_amd')
    M, L = tdgp.metrics, tdgp._lib
    n, F, k = args.rows, args.features, args.nhood_size
    g = torch.Generator(device='cuda').manual_seed(0)
    real = torch.randn(n, F, device='cuda', generator=g)
    gen = torch.randn(n, F, device='cuda', generator=g) * 0.9 + 0.05
    real16, gen16 = real.to(torch.float16), gen.to(torch.float16)
    res = dict(shape=dict(rows=n, features=F, nhood_size=k), device=torch.cuda.get_device_name(0), torch=torch.__version__)

    kernel = lambda: M.compute_pr(real, gen, nhood_size=k)                                   # noqa: E731
    on_device = lambda: torch_route(real16, gen16, k, host=False)                            # noqa: E731
    say = lambda msg: print(f'[bench_pr] {msg}', file=sys.stderr, flush=True)                # noqa: E731
    kernel(), on_device()                                                                     # warm-up
    say('warm-up done')
    # alternate the two device routes, so that a drift of the machine shows in both
    tk, td = [], []
    for _ in range(args.reps):
        a, vk = timed(kernel, 1)
        b, vd = timed(on_device, 1)
        tk.append(a['ms_min'])
        td.append(b['ms_min'])
        say(f'kernel {tk[-1]:.1f} ms, torch on device {td[-1]:.1f} ms')
    stat = lambda t: dict(ms_min=min(t), ms_median=float(np.median(t)), ms_max=max(t), reps=len(t))      # noqa: E731
    res['kernel'] = dict(stat(tk), precision=vk[0], recall=vk[1])
    res['torch_device'] = dict(stat(td), precision=vd[0], recall=vd[1])
    if args.host_reps > 0:
        th, vh = timed(lambda: torch_route(real16, gen16, k, host=True), args.host_reps, host_clock=True)
        say(f'torch with host copies {th["ms_median"]:.0f} ms')
        res['torch_host'] = dict(th, precision=vh[0], recall=vh[1], bytes_to_host=4 * n * n * 2)

    # per-kernel figures: the library's per-dispatch events, one profiled call
    L.profile_enable(True)
    kernel()
    torch.cuda.synchronize()
    prof = L.profile_report()
    L.profile_enable(False)
    res['kernels'] = {name: dict(launches=v['launches'], total_ms=v['total_ms']) for name, v in prof.items() if name.startswith('pr_')}
    total = sum(v['total_ms'] for v in res['kernels'].values())
    tile = sum(v['total_ms'] for name, v in res['kernels'].items() if name.startswith('pr_tile_kernel'))
    flop = 4 * 2.0 * n * n * F
    res['summary'] = dict(kernel_ms_total=total, tile_ms=tile, pack_and_merge_share=(total - tile) / total if total else None,
                          tile_flop=flop, tile_tflops=flop / (tile * 1e-3) / 1e12 if tile else None,
                          tile_share_of_fp16_peak=flop / (tile * 1e-3) / FP16_PEAK if tile else None,
                          workspace_bytes=dict(kth=int(L.load().tdgp_pr_kth_workspace_bytes(n, n, k + 1)), member=int(L.load().tdgp_pr_member_workspace_bytes(n, n))),
                          speedup_vs_torch_device=res['torch_device']['ms_median'] / res['kernel']['ms_median'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Measure the perceptual path length's device path against an eager torch restatement of it.

    python tools/bench_ppl.py [--config config_c3] [--batch 2] [--reps 9] [--out profiles/ppl_bench.json]

1. One sampler iteration (`metrics.PPLSampler.__call__`: mapping, two renders of `--batch` images, image tail, detector, pair distance) with a
   stand-in detector of the LPIPS width -- 7 995 392 floats per image, the five VGG16 feature layers of a 256^2 image concatenated; the
   stand-in tiles the flattened image to that width, a cheap fixed map -- against the same iteration with none of the new kernels
   (`EagerSampler` below: `rays_to_image`, slicing, `mean`, `(x + 1) * 127.5`, `sub / square / sum`).  Peak device memory of both.  Also the
   iteration with both endpoints in one synthesis call of 2 * batch images (`OneCallSampler`): what the sampler's two calls cost.
2. The two kernels alone against their torch restatements on the same buffers: tdgp_ppl_frames at the metric's shape and on 512^2 frames
   with the crop and a 2 x 2 box; tdgp_pair_sqdist on [2 * batch, 7 995 392] rows, with its achieved bytes per second.
Times are medians over `--reps` windows after a warm-up, host clock around work that ends in a device synchronise; a kernel window holds
`--inner` calls.  Seeded random weights: the distances say nothing about quality.  Needs a GPU; there is no fallback.
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

LPIPS_WIDTH = 7995392            # 64*256^2 + 128*128^2 + 256*64^2 + 512*32^2 + 512*16^2 (VGG16 relu1_2 .. relu5_3 of a 256^2 image), not measured on the detector


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='config_c3')
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ppl_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_ppl needs a GPU')
    torch.set_grad_enabled(False)
    tdgp = importlib.import_module('3dgp_amd')
    R, M = tdgp.renderer, tdgp.metrics
    cfg = getattr(tdgp.config, args.config)()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=105, exercise_all=True))
    G = G.to('cuda').eval()
    sync = torch.cuda.synchronize
    B, W = args.batch, LPIPS_WIDTH

    def detector(img):
        flat = img.flatten(1) * (1.0 / 255.0)
        return flat.repeat(1, -(-W // flat.shape[1]))[:, :W].contiguous()

    class EagerSampler(M.PPLSampler):
        """The same iteration with none of the new kernels: the image from `synthesis` (rays_to_image inside), the torch tail, the torch distance."""

        def endpoint_images(self, d):
            kw = dict(camera_params=d.camera_params, noise_mode='const', u_coarse=d.u_coarse, u_fine=d.u_fine, **self.G_kwargs)
            return M.ppl_image_tail(torch.cat([self.G.synthesis(ws=ws, **kw) for ws in (d.ws0, d.ws1)]), self.crop, self.factor)

        def forward(self, c, camera_params=None):
            l0, l1 = self.detector(self.endpoint_images(self.draw(c, camera_params))).chunk(2)
            return (l0 - l1).square().sum(1) / self.epsilon ** 2

    class OneCallSampler(M.PPLSampler):
        """The alternative the sampler does not take: both endpoints of every pair in ONE synthesis call of 2B images (what that would save)."""

        def endpoint_images(self, d):
            cam = {k: torch.cat([d.camera_params[k]] * 2) for k in ('angles', 'fov', 'radius', 'look_at')}
            syn = self.G.synthesis
            rgb = syn(ws=torch.cat([d.ws0, d.ws1]), camera_params=cam, noise_mode='const', u_coarse=torch.cat([d.u_coarse] * 2),
                      u_fine=torch.cat([d.u_fine] * 2), ray_major=True, **self.G_kwargs).rgb
            return R.ppl_frames(rgb, syn.test_resolution, syn.test_resolution, crop=self.crop, factor=self.factor)

    def timed(fn, reps=args.reps, warm=2, inner=1):
        for _ in range(warm):
            fn()
        out = []
        for _ in range(reps):
            sync()
            t0 = time.perf_counter()
            for _ in range(inner):
                r = fn()
            sync()
            out.append((time.perf_counter() - t0) * 1e3 / inner)
        return statistics.median(out), min(out), r

    def peak_of(fn):
        sync()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        sync()
        return torch.cuda.max_memory_allocated() - base

    result = dict(config=args.config, batch=B, reps=args.reps, inner=args.inner, device=torch.cuda.get_device_name(0), resolution=cfg.img_resolution,
                  num_ray_steps=cfg.num_ray_steps, detector_width=W, note='seeded random weights, stand-in detector: the distances are not a quality figure')
    dataset = UniformLabels(cfg.c_dim) if cfg.c_dim else None

    # ---- one sampler iteration
    samplers = dict(kernels=M.PPLSampler(G, detector, 1e-4, 'w', 'end', crop=False), eager=EagerSampler(G, detector, 1e-4, 'w', 'end', crop=False),
                    one_call_of_2B=OneCallSampler(G, detector, 1e-4, 'w', 'end', crop=False))
    it = {}
    values = {}
    for name, s in samplers.items():
        s.eval().requires_grad_(False)

        def one(s=s):
            torch.manual_seed(11)
            np.random.seed(11)
            c, cam = next(M.iterate_random_conditioning(G, B, 'cuda', None, dataset))
            return s(c, cam)
        med, mn, dist = timed(one)
        values[name] = dist.double().cpu()
        it[name] = dict(iteration_ms=med, iteration_min_ms=mn, peak_bytes=peak_of(one), distances=values[name].tolist())
    it['speedup'] = it['eager']['iteration_ms'] / it['kernels']['iteration_ms']
    it['two_calls_over_one_call'] = it['kernels']['iteration_ms'] / it['one_call_of_2B']['iteration_ms']
    it['peak_bytes_saved'] = it['eager']['peak_bytes'] - it['kernels']['peak_bytes']
    it['max_relative_difference'] = float(((values['kernels'] - values['eager']).abs() / values['eager'].abs().clamp_min(1e-300)).max())
    result['sampler_iteration'] = it

    # ---- the image tail alone
    tails = []
    for h, crop, factor in ((cfg.img_resolution, False, max(cfg.img_resolution // 256, 1)), (512, True, 2)):
        frames = torch.rand([2 * B, h * h, 3], device='cuda') * 2 - 1
        k_ms, k_min, a = timed(lambda: R.ppl_frames(frames, h, h, crop=crop, factor=factor), inner=args.inner)
        t_ms, t_min, b = timed(lambda: M.ppl_image_tail(R.rays_to_image(frames, h, h), crop, factor), inner=args.inner)
        tails.append(dict(frames=2 * B, h=h, crop=crop, factor=factor, kernel_ms=k_ms, kernel_min_ms=k_min, torch_ms=t_ms, torch_min_ms=t_min, speedup=t_ms / k_ms,
                          kernel_peak_bytes=peak_of(lambda: R.ppl_frames(frames, h, h, crop=crop, factor=factor)),
                          torch_peak_bytes=peak_of(lambda: M.ppl_image_tail(R.rays_to_image(frames, h, h), crop, factor)),
                          max_abs_difference=float((a - b).abs().max())))
        del frames, a, b
    result['ppl_frames'] = tails

    # ---- the pair distance alone
    feats = torch.randn([2 * B, W], device='cuda')
    feats[B:] = feats[:B] + 1e-4 * torch.randn([B, W], device='cuda')
    inv = 1.0 / (1e-4 * 1e-4)
    k_ms, k_min, a = timed(lambda: M.pair_sqdist(feats, inv), inner=args.inner)

    def torch_dist():
        l0, l1 = feats.chunk(2)
        return (l0 - l1).square().sum(1) / 1e-4 ** 2
    t_ms, t_min, b = timed(torch_dist, inner=args.inner)
    exact = ((feats[:B].double() - feats[B:].double()).square().sum(1) * inv).cpu()
    nbytes = 2 * B * W * 4
    # the windows above read ONE buffer over and over: at 128 MB it stays in the 256 MB Infinity Cache, so theirs is a cache rate.  Cycling
    # through buffers of 5 x that size in total makes every call fetch its rows from HBM.
    ring = [feats] + [feats.clone() for _ in range(4)]
    turn = [0]

    def cycled(fn):
        def run():
            turn[0] = (turn[0] + 1) % len(ring)
            return fn(ring[turn[0]])
        return run
    kc_ms, kc_min, _ = timed(cycled(lambda f: M.pair_sqdist(f, inv)), inner=args.inner)
    tc_ms, tc_min, _ = timed(cycled(lambda f: (f[:B] - f[B:]).square().sum(1) / 1e-4 ** 2), inner=args.inner)
    del ring
    result['pair_sqdist'] = dict(n=B, W=W, kernel_ms=k_ms, kernel_min_ms=k_min, torch_ms=t_ms, torch_min_ms=t_min, speedup=t_ms / k_ms, algorithmic_bytes=nbytes,
                                 kernel_GBps=nbytes / (k_ms * 1e-3) / 1e9, torch_GBps_same_bytes=nbytes / (t_ms * 1e-3) / 1e9,
                                 note='kernel_ms / torch_ms re-read one 128 MB buffer (resident in the Infinity Cache); the *_from_hbm figures cycle through five',
                                 kernel_from_hbm_ms=kc_ms, kernel_from_hbm_min_ms=kc_min, torch_from_hbm_ms=tc_ms, torch_from_hbm_min_ms=tc_min,
                                 kernel_from_hbm_GBps=nbytes / (kc_ms * 1e-3) / 1e9, speedup_from_hbm=tc_ms / kc_ms,
                                 kernel_peak_bytes=peak_of(lambda: M.pair_sqdist(feats, inv)), torch_peak_bytes=peak_of(torch_dist),
                                 kernel_rel_err_vs_float64=float(((a.double().cpu() - exact).abs() / exact).max()),
                                 torch_rel_err_vs_float64=float(((b.double().cpu() - exact).abs() / exact).max()),
                                 same_bytes_on_a_second_run=bool(torch.equal(a, M.pair_sqdist(feats, inv))))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Time the Pillow-exact resampling kernels and the data tools against what they replace and write profiles/resample_bench.json.

    python tools/bench_resample.py [--reps 7] [--files 2000] [--skip-end-to-end] [--out profiles/resample_bench.json]

Yardsticks: (1) Pillow on the host with the 16 threads a job may use -- the reference's route; (2) `torch.nn.functional.interpolate(...,
mode='bicubic', antialias=True)` on the same GPU -- the obvious alternative, NOT bit-compatible (fp32 weights, no intermediate rounding).
Shapes:
  detector_input  [256, 256, 256, 3] uint8 -> fp32 [256, 3, 224, 224] (bicubic 256 -> 256 is skipped, centre crop, normalise) and the same
                  from 320 x 320 inputs, where both passes run; kernel time, GB/s on the bytes the contract must move (the uint8 input once,
                  the fp32 output once), the host chain (Pillow resize, crop, torch CPU normalise) on 16 threads
  lanczos         500 x 375 -> 256^2 (centre square first) and 1024^2 -> 256^2, one image and a batch of 64
  depth16         the 16-bit pass, 512^2 -> 256^2, one map and a batch of 64
  end_to_end      resize_dataset and extract_features (a stand-in detector: a fixed pooling) on a synthetic folder of --files JPEGs,
                  device='cuda' against device=None and against the Pillow route, with the decode / resample / encode / copy shares
Device work is timed by events on the launch stream (call) and by the library's per-kernel event pairs (kernels); host routes by a host clock.
One warm-up of every route, then --reps repetitions in which the routes alternate; min / median / max.
"""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = 16


def stat(times, **more):
    med = float(np.median(times))
    return dict(ms_min=float(min(times)), ms_median=med, ms_max=float(max(times)), reps=len(times), **more)


def pil_filter(name):
    import PIL.Image
    return dict(lanczos=PIL.Image.LANCZOS, bicubic=PIL.Image.BICUBIC, bilinear=PIL.Image.BILINEAR)[name]


def pillow_batch(arrays, fn, pool):
    """`fn` on every array of the batch in the pool (PIL releases the GIL while it resamples); -> ms."""
    t0 = time.perf_counter()
    list(pool.map(fn, arrays))
    return (time.perf_counter() - t0) * 1e3


def write_jpeg_folder(root, files, seed=0):
    """`files` RGB JPEGs of ImageNet-like sizes in 8 class folders plus one text file: smooth random fields, so that they compress like photos."""
    import PIL.Image
    sizes = [(375, 500), (500, 375), (333, 500), (500, 500), (480, 640)]

    def one(i):
        rs = np.random.RandomState(seed + i)
        h, w = sizes[i % len(sizes)]
        low = rs.randint(0, 256, size=(h // 16 + 2, w // 16 + 2, 3)).astype(np.uint8)
        img = PIL.Image.fromarray(low).resize((w, h), PIL.Image.BICUBIC)
        noise = rs.randint(-6, 7, size=(h, w, 3))
        a = np.clip(np.asarray(img).astype(np.int16) + noise, 0, 255).astype(np.uint8)
        d = os.path.join(root, f'n{i % 8:02d}')
        os.makedirs(d, exist_ok=True)
        PIL.Image.fromarray(a).save(os.path.join(d, f'{i:06d}.jpg'), quality=90)

    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(one, range(files)))
    with open(os.path.join(root, 'README.txt'), 'w') as f:
        f.write('synthetic\n')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--files', type=int, default=2000)
    ap.add_argument('--skip-end-to-end', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'resample_bench.json'))
    args = ap.parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import PIL
    import PIL.Image
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample.py measures on a GPU; none found')
    tdgp = importlib.import_module('3dgp_amd')
    M, T, L_ = tdgp.images, tdgp.data_tools, tdgp._lib
    dev = torch.device('cuda:0')
    torch.set_num_threads(THREADS)
    say = lambda msg: print(f'[bench_resample] {msg}', file=sys.stderr, flush=True)      # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, pillow=PIL.__version__, host_threads=THREADS)
    pool = ThreadPoolExecutor(THREADS)

    def timed_call(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def kernel_times(fn):
        """Per-kernel time of one call, from the event pairs the library attaches to its launches."""
        torch.cuda.synchronize()
        L_.profile_enable(True)
        fn()
        rep = L_.profile_report()
        L_.profile_enable(False)
        return {k: v['total_ms'] for k, v in rep.items()}

    def measure(routes, reps=args.reps):
        """routes: name -> callable returning ms.  One warm-up each, then alternating repetitions."""
        for fn in routes.values():
            fn()
        times = {k: [] for k in routes}
        for _ in range(reps):
            for k, fn in routes.items():
                times[k].append(fn())
        return {k: stat(v) for k, v in times.items()}

    # ------------------------------------------------------------------------------------------------ detector_input
    res['detector_input'] = {}
    for side in (256, 320):
        B = 256
        g = torch.Generator(device=dev).manual_seed(side)
        x = torch.randint(0, 256, (B, side, side, 3), dtype=torch.uint8, device=dev, generator=g)
        xh = x.cpu().numpy()
        mean, std = torch.tensor(M.DETECTOR_MEAN).view(1, 3, 1, 1), torch.tensor(M.DETECTOR_STD).view(1, 3, 1, 1)
        mean_d, std_d = mean.to(dev), std.to(dev)
        top, left = M.center_crop_box(256, 256, 224, 224)

        def host_chain():
            t0 = time.perf_counter()
            small = list(pool.map(lambda a: np.asarray(PIL.Image.fromarray(a).resize((256, 256), PIL.Image.BICUBIC))[top:top + 224, left:left + 224], xh))
            t = torch.from_numpy(np.stack(small)).permute(0, 3, 1, 2)
            t.float().div(255).sub(mean).div(std)
            return (time.perf_counter() - t0) * 1e3

        def torch_chain():
            def go():
                t = x.permute(0, 3, 1, 2).float()
                if side != 256:
                    t = torch.nn.functional.interpolate(t, size=(256, 256), mode='bicubic', antialias=True)
                t[:, :, top:top + 224, left:left + 224].div(255).sub(mean_d).div(std_d)
            return timed_call(go)

        r = measure(dict(kernels_call=lambda: timed_call(lambda: M.detector_input(x)), torch_interpolate_gpu=torch_chain, pillow_host_16_threads=host_chain),
                    reps=max(3, args.reps // 2))
        kt = kernel_times(lambda: M.detector_input(x))
        moved = B * side * side * 3 + B * 3 * 224 * 224 * 4
        ks = sum(kt.values())
        r.update(batch=B, source=f'{side}x{side}x3', kernels_ms=kt, kernels_total_ms=ks, contract_bytes=moved, achieved_gb_s=moved / (ks * 1e-3) / 1e9,
                 bit_exact_vs_host_path=bool(M.detector_input(x[:4]).cpu().numpy().tobytes() == M.detector_input(xh[:4]).tobytes()))
        res['detector_input'][str(side)] = r
        say(f'detector_input {side}: kernels {ks:.3f} ms ({r["achieved_gb_s"]:.0f} GB/s on {moved / 1e6:.0f} MB), call {r["kernels_call"]["ms_median"]:.3f} ms, '
            f'torch {r["torch_interpolate_gpu"]["ms_median"]:.3f} ms, Pillow chain on {THREADS} threads {r["pillow_host_16_threads"]["ms_median"]:.0f} ms')
        del x

    # ------------------------------------------------------------------------------------------------ lanczos, depth16
    def resize_case(name, bits, hw, box, out, filter, batches=(1, 64)):
        r = {}
        for B in batches:
            g = torch.Generator(device=dev).manual_seed(B)
            shape = (B,) + hw + ((3,) if bits == 8 else ())
            x = torch.randint(0, 256 if bits == 8 else 65536, shape, dtype=torch.int32, device=dev, generator=g)
            x = x.to(torch.uint8) if bits == 8 else x.to(torch.int16).view(torch.uint16)
            xh = x.cpu().numpy() if bits == 8 else x.view(torch.int16).cpu().numpy().view(np.uint16)
            x0, y0, w, h = box

            def pil_one(a):
                return np.asarray(PIL.Image.fromarray(a).crop((x0, y0, x0 + w, y0 + h)).resize((out, out), pil_filter(filter)))

            routes = dict(kernels_call=lambda: timed_call(lambda: M.resize(x, out, filter, box=box)), pillow_host_16_threads=lambda: pillow_batch(xh, pil_one, pool))
            if bits == 8:
                def torch_route():
                    def go():
                        t = x[:, y0:y0 + h, x0:x0 + w].permute(0, 3, 1, 2).float()
                        torch.nn.functional.interpolate(t, size=(out, out), mode='bicubic', antialias=True).round_().clamp_(0, 255).to(torch.uint8)
                    return timed_call(go)
                routes['torch_interpolate_bicubic_gpu'] = torch_route
            m = measure(routes)
            kt = kernel_times(lambda: M.resize(x, out, filter, box=box))
            got = M.resize(x[:2], out, filter, box=box)
            got = got.cpu().numpy() if bits == 8 else got.view(torch.int16).cpu().numpy().view(np.uint16)
            m.update(kernels_ms=kt, kernels_total_ms=sum(kt.values()), bit_exact_vs_pillow=bool(all(np.array_equal(got[i], pil_one(xh[i])) for i in range(min(2, B)))))
            r[f'batch_{B}'] = m
            say(f'{name} B={B}: kernels {m["kernels_total_ms"]:.3f} ms, call {m["kernels_call"]["ms_median"]:.3f} ms, Pillow on {THREADS} threads '
                f'{m["pillow_host_16_threads"]["ms_median"]:.2f} ms, exact {m["bit_exact_vs_pillow"]}')
        res[name] = r

    resize_case('lanczos_500x375_to_256', 8, (375, 500), (62, 0, 375, 375), 256, 'lanczos')
    resize_case('lanczos_1024_to_256', 8, (1024, 1024), (0, 0, 1024, 1024), 256, 'lanczos')
    resize_case('depth16_lanczos_512_to_256', 16, (512, 512), (0, 0, 512, 512), 256, 'lanczos')

    # ------------------------------------------------------------------------------------------------ end to end
    if not args.skip_end_to_end:
        tmp = tempfile.mkdtemp(prefix='bench_resample_')
        try:
            src = os.path.join(tmp, 'raw')
            t0 = time.perf_counter()
            write_jpeg_folder(src, args.files)
            say(f'{args.files} JPEGs written in {time.perf_counter() - t0:.1f} s')
            e2e = dict(files=args.files)

            def pillow_route():
                """The reference's route: Pillow decode, centre crop, Lanczos, save, on 16 threads."""
                out = os.path.join(tmp, 'pil')
                names = T.find_images_in_dir(src)
                for d in {os.path.dirname(n) for n in names}:
                    os.makedirs(os.path.join(out, d), exist_ok=True)

                def one(n):
                    img = PIL.Image.open(os.path.join(src, n))
                    img.load()
                    T.write_image(T._pillow_center_resize_crop(img, 256), os.path.join(out, n))
                t0 = time.perf_counter()
                list(pool.map(one, names))
                return time.perf_counter() - t0

            for tag, device in (('warm_up', 'cuda'), ('cuda', 'cuda'), ('host_path', None)):
                out = os.path.join(tmp, 'out_' + tag)
                r = T.resize_dataset(src, target_dir=out, size=256, device=device)
                if tag != 'warm_up':
                    e2e['resize_dataset_' + tag] = dict(seconds=r['seconds'], resized=r['resized'], note='stage seconds are summed over the threads; total is wall time')
                    say(f'resize_dataset {tag}: {r["seconds"]}')
            e2e['resize_dataset_pillow_16_threads_wall_s'] = pillow_route()
            say(f'resize_dataset Pillow route: {e2e["resize_dataset_pillow_16_threads_wall_s"]:.2f} s')
            same = all(open(os.path.join(tmp, 'out_cuda', n), 'rb').read() == open(os.path.join(tmp, 'pil', n), 'rb').read() for n in T.find_images_in_dir(src)[:50])
            e2e['resize_dataset_files_identical_to_pillow_route'] = bool(same)

            pooled = lambda t: torch.nn.functional.adaptive_avg_pool2d(t, (8, 8)).flatten(1)      # noqa: E731  (a stand-in: the detector is the caller's)
            data = os.path.join(tmp, 'out_cuda')
            for tag, device in (('warm_up', 'cuda'), ('cuda', 'cuda'), ('host_path', None)):
                r = T.extract_features(data, pooled, os.path.join(tmp, f'f_{tag}.memmap'), device=device)
                if tag != 'warm_up':
                    e2e['extract_features_' + tag] = dict(seconds=r['seconds'], images=r['num_images'])
                    say(f'extract_features {tag}: {r["seconds"]}')
            res['end_to_end'] = e2e
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    pool.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Perceptual path length of a generator (the reference's metric 'ppl2_wend', src/metrics/metric_main.py:105-108): one JSON line.

    python tools/calc_ppl.py --ckpt exported_dir/ --vgg16 vgg16.pt [--metric ppl2_wend]
    python tools/calc_ppl.py --ckpt exported_dir/ --vgg16 vgg16.pt --space w --sampling end --epsilon 1e-4 [--crop] --num-samples N --batch 2 [--seed 0]

`--ckpt` is a directory written by tools/export_reference_checkpoint.py.  `--vgg16` is a TorchScript detector loaded with torch.jit.load and
called as `vgg16(img, resize_images=False, return_lpips=True)` on [2B,3,H,W] fp32 images in [0, 255] (the reference fetches its own from a
URL; it stays the caller's).  A conditional generator draws its classes uniformly (the reference draws dataset items; datasets are out of
scope here).  The two endpoints of a pair share their camera and their renderer draws; nothing crosses to the host until the one number.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
from calc_nfs import UniformLabels  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--ckpt', required=True, metavar='DIR', help='directory written by tools/export_reference_checkpoint.py')
    p.add_argument('--vgg16', required=True, metavar='FILE', help='TorchScript LPIPS detector (torch.jit.load)')
    p.add_argument('--metric', choices=['ppl2_wend'], default=None, help='a registry entry: fixes every option below but --seed')
    p.add_argument('--space', choices=['z', 'w'], default='w')
    p.add_argument('--sampling', choices=['full', 'end'], default='end')
    p.add_argument('--epsilon', type=float, default=1e-4)
    p.add_argument('--crop', action='store_true')
    p.add_argument('--num-samples', type=int, default=50000)
    p.add_argument('--batch', type=int, default=2, help='pairs per sampler call')
    p.add_argument('--seed', type=int, default=0)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    tdgp = importlib.import_module('3dgp_amd')
    cfg, sd = tdgp.weights.load_exported(args.ckpt)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(sd)
    G = G.to('cuda').eval()
    vgg16 = torch.jit.load(args.vgg16).eval().to('cuda')
    detector = lambda img: vgg16(img, resize_images=False, return_lpips=True)      # noqa: E731
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    dataset = UniformLabels(cfg.c_dim) if cfg.c_dim else None
    if args.metric == 'ppl2_wend':
        out = tdgp.metrics.ppl2_wend(G, detector, dataset=dataset)
        opts = dict(num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, batch=2)
    else:
        opts = dict(num_samples=args.num_samples, epsilon=args.epsilon, space=args.space, sampling=args.sampling, crop=args.crop, batch=args.batch)
        name = f'ppl_{args.space}{args.sampling}'
        out = {name: tdgp.metrics.ppl_for_generator(G, detector, num_samples=args.num_samples, epsilon=args.epsilon, space=args.space,
                                                    sampling=args.sampling, crop=args.crop, batch_size=args.batch, dataset=dataset)}
    print(json.dumps(dict(out, **opts, seed=args.seed, ckpt=args.ckpt, vgg16=args.vgg16)))


if __name__ == '__main__':
    main()

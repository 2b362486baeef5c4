#!/usr/bin/env python3
"""Feature-space metrics from two saved feature sets (the reference's 'fid50k', 'pr50k3', 'kid50k', 'is50k', src/metrics/metric_main.py): one JSON line.

    python tools/calc_feature_metrics.py --real REAL.npz --gen GEN.npz --metrics pr,kid,is[,fid] [--nhood-size 3] [--seed 0]

`--real` / `--gen` are `FeatureStats.save` files written with capture_all (the detector that produced them is the caller's: the reference
fetches its own from a URL).  `pr` and `kid` compare the two sets; `is` reads `--gen` as class probabilities.  Precision / recall runs on the
GPU (its k-NN passes have no CPU path); KID and IS run where the features are put: on the GPU when there is one.  `fid` reads the raw
moments of files written with capture_mean_cov; from a file that holds only rows it accumulates them first (on the GPU: one call of the
moments kernel, `FeatureStats.add_rows`).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ('pr', 'kid', 'is', 'fid')


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--real', metavar='STATS.npz', help='FeatureStats.save file of the real features (pr, kid, fid)')
    p.add_argument('--gen', required=True, metavar='STATS.npz', help='FeatureStats.save file of the generated features (or probabilities, for is)')
    p.add_argument('--metrics', default='pr,kid,is', help='comma-separated subset of pr,kid,is,fid')
    p.add_argument('--nhood-size', type=int, default=3)
    p.add_argument('--num-subsets', type=int, default=100)
    p.add_argument('--max-subset-size', type=int, default=1000)
    p.add_argument('--num-splits', type=int, default=10)
    p.add_argument('--seed', type=int, default=0, help='numpy seed of the KID subsets')
    return p


def moments_of(M, stats, device, path):
    """A loaded FeatureStats -> one with raw moments: itself, or (a file that holds only rows) those rows accumulated where `device` says."""
    if stats.capture_mean_cov:
        return stats
    if not stats.capture_all:
        raise SystemExit(f'fid: {path} holds neither raw moments (capture_mean_cov) nor rows (capture_all)')
    import torch
    rows = stats.get_all()
    full = M.FeatureStats(capture_mean_cov=True, device=device if device != 'cpu' else None)
    if full.device is None:
        full.append(rows)
    else:
        full.add_rows(torch.from_numpy(rows).to(full.device))
    return full


def main(argv=None):
    args = build_parser().parse_args(argv)
    names = [m for m in args.metrics.split(',') if m]
    unknown = sorted(set(names) - set(METRICS))
    if unknown or not names:
        raise SystemExit(f'--metrics: unknown {unknown}; choose from {",".join(METRICS)}')
    if ({'pr', 'kid', 'fid'} & set(names)) and not args.real:
        raise SystemExit('--real is needed for pr, kid and fid')
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    tdgp = importlib.import_module('3dgp_amd')
    M = tdgp.metrics
    device = 'cuda' if torch.cuda.is_available() else 'cpu'
    gen_stats = M.FeatureStats.load(args.gen)
    real_stats = M.FeatureStats.load(args.real) if args.real else None
    rows_needed = bool({'pr', 'kid', 'is'} & set(names))
    gen = torch.from_numpy(gen_stats.get_all()).to(device) if rows_needed else None
    real = torch.from_numpy(real_stats.get_all()).to(device) if rows_needed and args.real else None
    out = {}
    if 'fid' in names:
        out['fid'] = M.compute_fid(moments_of(M, real_stats, device, args.real), moments_of(M, gen_stats, device, args.gen))
        if not rows_needed:
            out.update(num_real=real_stats.num_items, num_gen=gen_stats.num_items, seed=args.seed, real=args.real, gen=args.gen)
            print(json.dumps(out))
            return
    if 'pr' in names:
        out['precision'], out['recall'] = M.compute_pr(real, gen, nhood_size=args.nhood_size)
        out['nhood_size'] = args.nhood_size
    if 'kid' in names:
        np.random.seed(args.seed)
        out['kid'] = M.compute_kid(real, gen, num_subsets=args.num_subsets, max_subset_size=args.max_subset_size)
    if 'is' in names:
        out['is_mean'], out['is_std'] = M.compute_is(gen, num_splits=args.num_splits)
    out.update(num_real=None if real is None else int(real.shape[0]), num_gen=int(gen.shape[0]), seed=args.seed, real=args.real, gen=args.gen)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Non-flatness score of a generator (the reference's metric 'nfs256', src/metrics/metric_main.py:118-120): one JSON line.

    python tools/calc_nfs.py --ckpt exported_dir/ [--num-gen 256] [--batch-gen 4] [--seed 0]

`--ckpt` is a directory written by tools/export_reference_checkpoint.py.  The depth range is the generator's ray range, 64 bins, frontal
cameras, cut_quantile 0.5.  A conditional generator draws its classes uniformly (the reference draws dataset items; datasets are out of scope
here).  Depth maps are reduced to histograms on the GPU; 64 counts per image cross to the host.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class UniformLabels:
    """Dataset stand-in for `iterate_random_conditioning` when no dataset is at hand: `num_classes` items, item i carrying the one-hot label
    of class i, so that the loop's `np.random.randint(len(dataset))` draws classes uniformly (also used by tools/bench_nfs.py)."""

    def __init__(self, num_classes):
        self.num_classes = int(num_classes)

    def __len__(self):
        return self.num_classes

    def get_label(self, i):
        label = np.zeros(self.num_classes, dtype=np.float32)
        label[i] = 1.0
        return label

    def get_camera_angles(self, i):
        return np.array([0.0, np.pi / 2, 0.0], dtype=np.float32)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--ckpt', required=True, metavar='DIR', help='directory written by tools/export_reference_checkpoint.py')
    p.add_argument('--num-gen', type=int, default=256)
    p.add_argument('--batch-gen', type=int, default=4, help='images per forward (the reference\'s default is 4); must divide 64')
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
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    dataset = UniformLabels(cfg.c_dim) if cfg.c_dim else None
    with torch.no_grad():
        score = tdgp.metrics.compute_flatness_score(G, args.num_gen, cfg.ray_start, cfg.ray_end, batch_gen=args.batch_gen, dataset=dataset)
    key = f'nfs{args.num_gen}'
    print(json.dumps({key: score, 'num_gen': args.num_gen, 'batch_gen': args.batch_gen, 'seed': args.seed, 'ckpt': args.ckpt}))


if __name__ == '__main__':
    main()

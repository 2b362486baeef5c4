#!/usr/bin/env python3
"""Filter an image folder by Gaussian log-likelihood of its detector features (the reference's scripts/data_scripts/run_instance_selection.py): one JSON line.

    python tools/run_instance_selection.py -s SOURCE_DIR -o OUTPUT_DIR (-n NUM | -r RATIO) [--subdir_wise] [--reg_covar 1e-05] --embeddings FILE.npy

`--embeddings` is an [N, F] array whose row i belongs to the i-th image of SOURCE_DIR in sorted relative-path order (every file with an
extension PIL knows, as the reference discovers them); the detector that produced it is the caller's -- the reference fetches its own from a
URL.  The scores are computed on the GPU when there is one (fp64 moments and Mahalanobis kernels), on the host otherwise (`--device cpu`
forces that).  The kept files are copied to the same relative paths under OUTPUT_DIR.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('-s', '--source_dir', required=True, type=str, help='Source directory')
    p.add_argument('-o', '--output_dir', required=True, type=str, help='Target directory')
    p.add_argument('-n', '--num_imgs_to_keep', default=None, type=int, help='How many images to keep')
    p.add_argument('-r', '--keep_ratio', default=None, type=float, help='Which share of the images to keep')
    p.add_argument('--subdir_wise', action='store_true', help='Select inside each subdirectory separately (the ImageNet recipe does)')
    p.add_argument('--reg_covar', type=float, default=0.0, help='Covariance regularisation; needed when a folder has fewer images than features (ImageNet: 1e-05)')
    p.add_argument('--embeddings', required=True, metavar='FILE.npy', help='[N, F] features in discovery order')
    p.add_argument('--device', default=None, choices=('cuda', 'cpu'), help='default: cuda if a GPU is present')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    S = importlib.import_module('3dgp_amd').instance_selection
    device = args.device or ('cuda' if torch.cuda.is_available() else 'cpu')
    embeddings = np.load(args.embeddings)
    try:
        kept = S.run_instance_selection(args.source_dir, args.output_dir, num_imgs_to_keep=args.num_imgs_to_keep, keep_ratio=args.keep_ratio,
                                        subdir_wise=args.subdir_wise, reg_covar=args.reg_covar, embeddings=embeddings, verbose=False,
                                        device=None if device == 'cpu' else device)
    except ValueError as e:
        raise SystemExit(f'run_instance_selection: {e}')
    print(json.dumps(dict(source_dir=args.source_dir, output_dir=args.output_dir, num_images=int(embeddings.shape[0]), num_features=int(embeddings.shape[1]),
                          num_kept=len(kept), subdir_wise=bool(args.subdir_wise), reg_covar=args.reg_covar, device=device, kept=kept)))


if __name__ == '__main__':
    main()

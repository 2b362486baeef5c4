#!/usr/bin/env python3
"""Centre-crop and resize every image of a folder (the reference's scripts/data_scripts/resize_dataset.py): one JSON line.

    python tools/resize_dataset.py -d SOURCE_DIR -s SIZE [-t TARGET_DIR] [-f .jpg] [--images_only] [--rename_enum] [--device cpu]

Every image under SOURCE_DIR is cropped to its centre square and resized to SIZE x SIZE with Pillow's Lanczos arithmetic, bit for bit: `L`,
`RGB` and 16-bit `I;16` images on the GPU when there is one (`--device cpu` forces the host path, same bytes), every other mode (palette,
alpha, CMYK, ...) through Pillow on the host, counted as `host_fallback`.  Files that are not images are copied unless `--images_only`.
`.jpg` is written with quality 95.  Decoding and encoding run in a thread pool of at most 16 threads; the JSON line shows their share.
"""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('-d', '--source_dir', required=True, type=str, help='folder of raw images; sub-folders are walked')
    p.add_argument('-t', '--target_dir', default=None, type=str, help='where the resized tree goes; without it, SOURCE_DIR with _SIZE appended')
    p.add_argument('-s', '--size', required=True, type=int, help='side of the square output in pixels')
    p.add_argument('-f', '--format', type=str, default=None, help='write every image with this extension, e.g. .jpg; without it each keeps its own')
    p.add_argument('-j', '--num_jobs', type=int, default=16, help='decoder / encoder threads, 16 at the most')
    p.add_argument('--ignore_ext', type=str, default='.DS_Store', help='leave out files whose path ends like this')
    p.add_argument('--ignore_regex', type=str, default=None, help='leave out files whose whole relative path matches this expression')
    p.add_argument('--fname_prefix', type=str, default='', help='text put in front of every relative output name')
    p.add_argument('--images_only', action='store_true', help='do not carry files over that are not images')
    p.add_argument('--rename_enum', action='store_true', help='name the outputs by their eight-digit position in the sorted listing')
    p.add_argument('--ignore_grayscale', action='store_true', help='leave mode-L images out')
    p.add_argument('--ignore_broken', action='store_true', help='leave an image out when it does not decode, rather than stopping')
    p.add_argument('--ignore_existing', action='store_true', help='leave an image alone when its output file is already there')
    p.add_argument('--device', default=None, choices=('cuda', 'cpu'), help='default: cuda if a GPU is present')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    T = importlib.import_module('3dgp_amd').data_tools
    device = args.device or ('cuda' if torch.cuda.is_available() else 'cpu')
    res = T.resize_dataset(args.source_dir, target_dir=args.target_dir, size=args.size, format=args.format, ignore_ext=args.ignore_ext,
                           ignore_regex=args.ignore_regex, images_only=args.images_only, fname_prefix=args.fname_prefix, rename_enum=args.rename_enum,
                           ignore_grayscale=args.ignore_grayscale, ignore_broken=args.ignore_broken, ignore_existing=args.ignore_existing,
                           device=None if device == 'cpu' else device, threads=args.num_jobs)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

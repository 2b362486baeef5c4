#!/usr/bin/env python3
"""Merge a folder of images with a folder of depth maps (the reference's scripts/data_scripts/merge_depth_data.py): one JSON line.

    python tools/merge_depth_data.py -i IMAGES_DIR -d DEPTHS_DIR -t TARGET_DIR

Every `NAME.jpg` of IMAGES_DIR that has a `NAME.png` at the same relative path in DEPTHS_DIR is copied to TARGET_DIR next to its depth map,
renamed `NAME_depth.png`: the layout `ImageFolderDataset(use_depth=True)` and tools/train.py read.
"""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('-i', '--images_dir', required=True, type=str, help='folder holding NAME.jpg files')
    p.add_argument('-d', '--depths_dir', required=True, type=str, help='folder holding NAME.png depth maps under the same relative paths')
    p.add_argument('-t', '--target_dir', required=True, type=str, help='folder the pairs are written to')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    T = importlib.import_module('3dgp_amd').data_tools
    merged = T.merge_depth_data(args.images_dir, args.depths_dir, args.target_dir)
    print(json.dumps(dict(images_dir=args.images_dir, depths_dir=args.depths_dir, target_dir=args.target_dir, num_merged=len(merged))))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Detector features of every image of a folder (the reference's scripts/data_scripts/extract_features.py): one JSON line.

    python tools/extract_features.py --dataset DIR --detector FILE.pt --out FEATS.memmap [--npy FEATS.npy] [--batch_size 256] [--device cpu]

FILE.pt is a TorchScript module (`torch.jit.load`) taking fp32 [B, 3, 224, 224] batches and returning [B, F]; the detector is the caller's --
the reference fetches its own through timm.  Every image (depth maps `*_depth.png` left out) is converted to RGB and passed through the eval
transform timm resolves for the reference's default embedder -- bicubic resize of the shorter side to 256 with Pillow's bytes, centre crop to
224, / 255, normalise -- on the GPU when there is one.  Writes FEATS.memmap (float32 [N, F]) and FEATS_desc.json, which
`ImageFolderDataset(use_embeddings=True)` and tools/train.py open, and with `--npy` the same rows in discovery order for
tools/run_instance_selection.py --embeddings.
"""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--dataset', required=True, metavar='DIR', help='Image folder')
    p.add_argument('--detector', required=True, metavar='FILE.pt', help='TorchScript feature detector')
    p.add_argument('--out', required=True, metavar='FEATS.memmap', help='Output memmap (its descriptor is written next to it)')
    p.add_argument('--npy', default=None, metavar='FEATS.npy', help='Also write the [N, F] array in discovery order')
    p.add_argument('--batch_size', type=int, default=256)
    p.add_argument('--resize', type=int, default=256, help='Shorter side before the crop')
    p.add_argument('--crop', type=int, default=224, help='Centre crop handed to the detector')
    p.add_argument('--device', default=None, choices=('cuda', 'cpu'), help='default: cuda if a GPU is present')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    T = importlib.import_module('3dgp_amd').data_tools
    device = args.device or ('cuda' if torch.cuda.is_available() else 'cpu')
    detector = torch.jit.load(args.detector, map_location=device).eval()
    res = T.extract_features(args.dataset, detector, args.out, batch_size=args.batch_size, device=None if device == 'cpu' else device, npy_path=args.npy,
                             resize=args.resize, crop=args.crop)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

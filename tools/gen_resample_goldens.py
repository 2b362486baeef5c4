#!/usr/bin/env python3
"""Write tests/golden/resample.npz from live Pillow: what `PIL.Image.resize` gives on the shared resampling cases.

    python tools/gen_resample_goldens.py [--out tests/golden/resample.npz]

The cases and their seeded inputs are those of tests/pillow_resample_reference.py (CASES_U8, CASES_U16, make_input): 8-bit L / RGB images and
16-bit `I;16` maps, Lanczos / bicubic / bilinear.  The file holds Pillow's version string and, per case, Pillow's output; for an output larger
than GOLDEN_FULL_BYTES only its SHA-256 (32 bytes under `sha256:<case>`), so that the file stays a few hundred KB -- the bicubic 256 -> 224
RGB noise image (the detector shape) is kept in full.  Two crop-window cases (`box/...`) hold `.crop(box).resize(...)`.  The GPU tests compare
with this file, so they do not need Pillow where they run.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))

BOX_CASES = ((8, 'lanczos', (41, 57), 3, (5, 3, 31, 29), (16, 20)), (16, 'bicubic', (41, 57), 1, (7, 9, 33, 21), (12, 40)))      # bits, filter, (H, W), C, (x0, y0, w, h), (oh, ow)


def pil_filter(name):
    import PIL.Image
    return dict(lanczos=PIL.Image.LANCZOS, bicubic=PIL.Image.BICUBIC, bilinear=PIL.Image.BILINEAR)[name]


def pil_resize(x, out, filter, box=None):
    """x: uint8 [H, W, C] (C in {1, 3}) or uint16 [H, W] -> Pillow's resize of it (of its window box = (x0, y0, w, h), cropped first)."""
    import PIL.Image
    im = PIL.Image.fromarray(x[:, :, 0] if x.ndim == 3 and x.shape[2] == 1 else x)
    assert im.mode in ('L', 'RGB', 'I;16'), im.mode
    if box is not None:
        x0, y0, w, h = box
        im = im.crop((x0, y0, x0 + w, y0 + h))
    res = np.asarray(im.resize((out[1], out[0]), pil_filter(filter)))
    return res.reshape(out + (x.shape[2],)) if x.ndim == 3 else res


def main(argv=None):
    import PIL
    import pillow_resample_reference as R
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'resample.npz'))
    args = p.parse_args(argv)
    data = dict(pillow_version=np.array(PIL.__version__))
    cases = [(8,) + c for c in R.CASES_U8] + [(16, f, hw, out, 1, kind) for f, hw, out, kind in R.CASES_U16]
    for bits, f, hw, out, c, kind in cases:
        y = pil_resize(R.make_input(bits, hw, c, kind, key=f), out, f)
        key = R.case_key(bits, f, hw, out, c, kind)
        if R.golden_keeps_bytes(bits, f, hw, out, c, kind):
            data[key] = y
        else:
            data['sha256:' + key] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(y).tobytes()).digest(), dtype=np.uint8)
    for bits, f, hw, c, box, out in BOX_CASES:
        data[f'box/u{bits}'] = pil_resize(R.make_input(bits, hw, c, 'noise', key='box'), out, f, box=box)
    np.savez_compressed(args.out, **data)
    print(f'{args.out}: {len(data) - 1} cases from Pillow {PIL.__version__}, {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()

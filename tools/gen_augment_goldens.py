#!/usr/bin/env python3
"""Generate the augmentation goldens by importing the REFERENCE's AugmentPipe on the CPU (build container only).

Only arrays are written -- data, never reference source.  Per case (shape, colour channels, probabilities) and per `debug_percentile`:
the output and the gradient `dx` for a seeded `dy`, from the reference run in fp32 and run again in float64 (default dtype float64, the same
float32 input cast up, `Hz_geom` left float32 because the reference asserts it, `Hz_fbank` cast up).  First order only, through torch's own
`grid_sample` (`grid_sample_gradfix.enabled` stays False).  The tool asserts that both runs took the same integer decisions (the margins
handed to `pad`, every `round` and `floor`): a flip there would show as a distance thousands of times the rounding noise.

Layout (every file below the size limit of a committed file):
  tests/golden/augment.npz                    Hz_geom, Hz_fbank, percentiles, and per case <case>_x, <case>_dy
  tests/golden/augment/<case>_q<NN>.npz       y64, dx64 (float64) and y32_d16 / dx32_d16 + y32_scale / dx32_scale: the fp32 run as a float16
                                              difference from the float64 one in units of its own maximum (tests/augment_reference.py unpacks)

Run:  python tools/gen_augment_goldens.py     (needs the reference tree; TDGP_REFERENCE overrides its place)
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TDGP_REFERENCE', '/root/reference')
OUT = os.path.join(REPO, 'tests', 'golden')

BASE = dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1)    # configs/training/base.yaml
CASES = dict(rgbd=dict(shape=[3, 4, 24, 40], ncc=3, kw=BASE), rgb16=dict(shape=[2, 3, 16, 16], ncc=3, kw=BASE), luma16=dict(shape=[2, 1, 16, 16], ncc=1, kw=BASE),
             patch64=dict(shape=[2, 4, 64, 64], ncc=3, kw=BASE), filt=dict(shape=[2, 4, 24, 40], ncc=3, kw=dict(BASE, imgfilter=1, cutout=1)))
PERCENTILES = [0.02, 0.1, 0.35, 0.5, 0.7, 0.93, 0.98]


def _import_reference():
    om = types.ModuleType('omegaconf')
    om.DictConfig = type('DictConfig', (dict,), {})
    om.OmegaConf = object
    sys.modules.setdefault('omegaconf', om)
    tv = types.ModuleType('torchvision')
    tv.__path__ = []
    sys.modules.setdefault('torchvision', tv)
    for sub in ('torchvision.transforms', 'torchvision.transforms.functional', 'torchvision.utils', 'torchvision.io'):
        m = types.ModuleType(sub)
        m.__path__ = []
        sys.modules.setdefault(sub, m)
    sys.path.insert(0, REF)


_import_reference()
import torch  # noqa: E402
from src.training.augment import AugmentPipe  # noqa: E402
from src.torch_utils.ops import grid_sample_gradfix  # noqa: E402


class _Decisions:
    """Records the integers the pipe decides on: pad margins, round and floor results."""
    def __enter__(self):
        self.log = []
        self.saved = (torch.nn.functional.pad, torch.round, torch.floor)
        pad_fn, rnd, flr = self.saved

        def pad_(input, pad, *a, **k):                       # noqa: A002
            self.log.append(('pad', tuple(int(v) for v in pad)))
            return pad_fn(input, pad, *a, **k)

        def round_(t, *a, **k):
            r = rnd(t, *a, **k)
            self.log.append(('round', tuple(r.flatten().tolist())))
            return r

        def floor_(t, *a, **k):
            r = flr(t, *a, **k)
            if r.ndim == 0:                                  # the percentile's own floors; those of the (discarded) random draws are not decisions
                self.log.append(('floor', float(r)))
            return r
        torch.nn.functional.pad, torch.round, torch.floor = pad_, round_, floor_
        return self

    def __exit__(self, *exc):
        torch.nn.functional.pad, torch.round, torch.floor = self.saved


def run(case, q, x32, dy32, dtype):
    torch.set_default_dtype(dtype)
    try:
        pipe = AugmentPipe(**case['kw'])
        assert pipe.Hz_geom.dtype == torch.float32
        pipe.Hz_fbank = pipe.Hz_fbank.to(dtype)
        x = torch.from_numpy(x32).to(dtype).requires_grad_(True)
        with _Decisions() as d:
            y = pipe(x, num_color_channels=case['ncc'], debug_percentile=q)
        dx, = torch.autograd.grad(y, x, torch.from_numpy(dy32).to(dtype))
        return y.detach().numpy(), dx.numpy(), d.log, pipe
    finally:
        torch.set_default_dtype(torch.float32)


def pack_diff(a32, a64):
    d = a32.astype(np.float64) - a64
    scale = max(float(np.abs(d).max()), 1e-30)
    return (d / scale).astype(np.float16), np.float64(scale)


def main():
    assert grid_sample_gradfix.enabled is False
    os.makedirs(os.path.join(OUT, 'augment'), exist_ok=True)
    top = dict(percentiles=np.asarray(PERCENTILES))
    for ci, (name, case) in enumerate(CASES.items()):
        rs = np.random.RandomState(700 + ci)
        x = rs.randn(*case['shape']).astype(np.float32)
        dy = rs.randn(*case['shape']).astype(np.float32)
        top[name + '_x'], top[name + '_dy'] = x, dy
        for q in PERCENTILES:
            y32, dx32, log32, pipe = run(case, q, x, dy, torch.float32)
            y64, dx64, log64, _ = run(case, q, x, dy, torch.float64)
            assert y32.dtype == np.float32 and y64.dtype == np.float64
            # round / floor must agree.  A margin may differ by one: where the exact margin is an integer (q = 0.5: a flip and a half turn map
            # the frame onto itself, margin exactly 6) the two precisions land on either side of `ceil`.  One more row of reflect padding moves
            # nothing but texels the crop discards; the distance printed below stays at the rounding level, and is asserted to.
            strip = lambda log: [e for e in log if e[0] != 'pad']                        # noqa: E731
            pads32, pads64 = ([e[1] for e in log if e[0] == 'pad'] for log in (log32, log64))
            assert strip(log32) == strip(log64) and len(pads32) == len(pads64), f'{name} q={q}: the fp32 and float64 runs decided differently\n{log32}\n{log64}'
            assert all(abs(a - b) <= 1 for p32, p64 in zip(pads32, pads64) for a, b in zip(p32, p64)), (name, q, pads32, pads64)
            flipped = pads32 != pads64
            top.setdefault('Hz_geom', pipe.Hz_geom.numpy())
            top.setdefault('Hz_fbank', pipe.Hz_fbank.numpy().astype(np.float32))
            yd, ys = pack_diff(y32, y64)
            dd, ds = pack_diff(dx32, dx64)
            path = os.path.join(OUT, 'augment', f'{name}_q{int(round(q * 100)):02d}.npz')
            np.savez(path, y64=y64, dx64=dx64, y32_d16=yd, y32_scale=ys, dx32_d16=dd, dx32_scale=ds)
            rng = max(1.0, float(np.abs(y64).max())), max(1.0, float(np.abs(dx64).max()))
            assert max(ys / rng[0], ds / rng[1]) < 1e-4, (name, q, ys, ds)
            print(f'{name} q={q}:{" MARGIN FLIP" if flipped else ""} margins {[e[1] for e in log32 if e[0] == "pad"][:1]} fp32-vs-f64 y {ys / rng[0]:.2e} dx {ds / rng[1]:.2e}  '
                  f'{os.path.getsize(path) / 1024:.0f} KiB')
    np.savez(os.path.join(OUT, 'augment.npz'), **top)


if __name__ == '__main__':
    main()

"""tests/modconv_reference.py (the float64 reference of tests/test_modconv_training_gpu.py) against tests/golden/modconv_grad.npz: y, dx, dw, ds
of autograd through the original implementation's unfused modulated_conv2d, for the stride-1 3x3 and 1x1 forms and the x2 layer.  No GPU.

Bars: the ones these goldens are held to elsewhere -- y 1e-5 of max|ref| (test_modulated_conv2d_autograd), the gradients 1e-5
(test_modconv_grad_oracle; the GPU tests allow them 2e-5).  The goldens are fp32 results, so what is measured is their rounding.
"""
import numpy as np
import pytest
import torch

import modconv_reference as R
from conftest import assert_close, load_golden, max_rel, report_parity

CASES = [('c3', 1, True), ('rgb', 1, False), ('c3big', 1, True), ('up', 2, True), ('upbig', 2, True)]


@pytest.mark.parametrize('tag,up,demod', CASES, ids=[c[0] for c in CASES])
def test_reference_matches_the_original_autograd(tag, up, demod):
    g = load_golden('modconv_grad')
    got = R.modconv_grads(g[f'{tag}_x'], g[f'{tag}_w'], g[f'{tag}_s'], g[f'{tag}_dy'], up=up, demodulate=demod)
    report_parity(f'modconv float64 reference vs golden {tag}', **{n: max_rel(got[n], g[f'{tag}_{n}'], 1.0) for n in ('y', 'dx', 'dw', 'ds')})
    for n in ('y', 'dx', 'dw', 'ds'):
        assert got[n].dtype == np.float64
        assert_close(got[n], g[f'{tag}_{n}'], 1e-5, f'{tag} {n}', 1.0)


def test_reference_fp32_mode_and_filter():
    """dtype=float32 runs the same graph in fp32 (the yardstick the GPU tests report next to the HIP figures): close to, and not
    identical with, the float64 run.  The default filter is the normalised [1, 3, 3, 1] one, and a filter that is not symmetric is
    applied as a convolution (the flip convention of upfirdn2d with flip_filter=False)."""
    g = load_golden('modconv_grad')
    args = [g[f'up_{n}'] for n in ('x', 'w', 's', 'dy')]
    r64, r32 = R.modconv_grads(*args, up=2), R.modconv_grads(*args, up=2, dtype=torch.float32)
    for n in r64:
        assert r32[n].dtype == np.float32
        e = max_rel(r32[n], r64[n], 1.0)
        assert 0 < e < 2e-6, (n, e)
    f = R.setup_filter()
    assert f.shape == (4, 4) and abs(float(f.sum()) - 1) < 1e-15 and float(f[1, 2]) == 9 / 64 and float(f[0, 3]) == 1 / 64
    z = torch.zeros(1, 1, 5, 5, dtype=torch.float64)
    z[0, 0, 2, 2] = 1.0
    fa = torch.arange(16, dtype=torch.float64).reshape(4, 4)
    out = R.upfirdn_pad1(z, fa, gain=2.0)                      # the response to an impulse is the filter itself, not its mirror image
    assert out.shape == (1, 1, 4, 4) and torch.equal(out[0, 0], 2.0 * fa)

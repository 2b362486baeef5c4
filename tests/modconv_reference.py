"""Plain high-precision evaluation of the modulated convolution of the synthesis layers and its gradients: torch on the CPU, float64 by
default, written from the formulas alone (networks_stylegan2.py:60-80 unfused, conv2d_resample.py:108-125, upfirdn2d.py) -- it imports
neither the product nor `oracle/`.

    d = rsqrt(sum_{c,k} (w * s)^2 + 1e-8)                                              (demodulate; else d = 1)
    y = conv2d(x * s, w, padding k // 2) * d                                           (up 1)
    y = upfirdn(conv_transpose2d(x * s, w^T, stride 2), f, pad 1, gain 4) * d          (up 2; w^T = w as [Cin, Cout, 3, 3])

dx, dw and ds come from torch.autograd.grad through that graph.  `dtype=torch.float32` runs the very same graph in fp32: the yardstick of
what an fp32 evaluation of the unfused path is from the float64 one.  tests/test_modconv_reference.py ties it to the committed goldens of
the original implementation's autograd.
"""
import numpy as np
import torch


def setup_filter(taps=(1, 3, 3, 1)):
    """The separable, normalised resample filter (upfirdn2d.setup_filter): outer(taps, taps) / sum -> float64 [n, n]."""
    f = torch.as_tensor(taps, dtype=torch.float64)
    f = torch.outer(f, f)
    return f / f.sum()


def upfirdn_pad1(z, f, gain):
    """upfirdn2d(z, f, up 1, padding 1, flip_filter False): zero-pad by one pixel, then CONVOLVE every channel with f * gain (conv2d
    correlates, so the taps are flipped) -> [B, C, H + 2 - (n - 1), W + 2 - (n - 1)]."""
    C = z.shape[1]
    taps = (f.to(z.dtype) * gain).flip([0, 1])[None, None].repeat(C, 1, 1, 1)
    return torch.nn.functional.conv2d(torch.nn.functional.pad(z, [1, 1, 1, 1]), taps, groups=C)


def modconv(x, w, s, up=1, demodulate=True, f=None):
    """y [B, Cout, H * up, W * up] of x [B, Cin, H, W], w [Cout, Cin, k, k], s [B, Cin] in the dtype of its arguments."""
    B, cin, H, W = x.shape
    cout, cin_w, k, k2 = w.shape
    assert cin_w == cin and k == k2 and s.shape == (B, cin) and up in (1, 2)
    xs = x * s[:, :, None, None]
    if up == 1:
        y = torch.nn.functional.conv2d(xs, w, padding=k // 2)
    else:
        assert k == 3
        z = torch.nn.functional.conv_transpose2d(xs, w.transpose(0, 1), stride=2)                 # [B, Cout, 2H + 1, 2W + 1]
        y = upfirdn_pad1(z, setup_filter() if f is None else f, gain=4.0)
    if demodulate:
        d = ((w[None] * s[:, None, :, None, None]).square().sum([2, 3, 4]) + 1e-8).rsqrt()        # [B, Cout]
        y = y * d[:, :, None, None]
    return y


def modconv_grads(x, w, s, dy, up=1, demodulate=True, f=None, dtype=torch.float64):
    """dict(y, dx, dw, ds) as numpy arrays of `dtype`: the forward and torch.autograd.grad of <y, dy> through `modconv`."""
    cast = lambda t: torch.as_tensor(t).detach().cpu().to(dtype)              # noqa: E731
    x, w, s = (cast(t).clone().requires_grad_(True) for t in (x, w, s))
    y = modconv(x, w, s, up=up, demodulate=demodulate, f=None if f is None else cast(f))
    dx, dw, ds = torch.autograd.grad(y, [x, w, s], cast(dy))
    return {n: np.ascontiguousarray(t.detach().numpy()) for n, t in dict(y=y, dx=dx, dw=dw, ds=ds).items()}

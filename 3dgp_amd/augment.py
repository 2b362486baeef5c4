"""The ADA augmentation pipe (src/training/augment.py of the reference) on the HIP kernels of csrc/augment.hip.

`AugmentPipe` keeps the reference's constructor, buffers (`p`, `Hz_geom`, `Hz_fbank`) and `forward` signature, so a snapshot's
`augment_pipe` entry loads with `load_state_dict`.  One call is three launches and no host round trip:

  params()   tdgp_augment_params: every per-sample parameter (G_inv, C, band gains, noise sigma, cutout) from one `rand` and one `randn`
             block of torch's generator -- or from a fixed `debug_percentile` -- in the reference's order of fp32 operations;
  apply()    tdgp_augment_geom (margins, reflect pad, x2 sym6 upsampling, affine bilinear sampling, x2 downsampling in one kernel), then
             tdgp_augment_color (colour matrix, noise, cutout).

Given its parameters the operator is linear in the image (affine, counting the colour bias and the noise), so its gradient is its adjoint:
`_Geom` / `_GeomAdj` and `_Color` are `torch.autograd.Function`s whose `backward` is each other, parameters carry no gradient, and
`create_graph=True` works to any order (R1's double backward is the forward again).  Image-space filtering (off in the reference's default
list) runs as eager torch ops with torch's own gradients.  The draws are this module's own (no RNG parity with the reference is claimed);
the filter taps come from tools/gen_wavelets.py.
"""
import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .wavelet_taps import SYM2, SYM6

_CFG_FLOATS, _UNIFORMS, _NORMALS = 31, 29, 12          # TDGP_AUGMENT_* (include/tdgp.h)


def geom_filter():
    """upfirdn2d.setup_filter(sym6): the taps normalised to sum 1, float32, separable."""
    taps = torch.as_tensor(SYM6, dtype=torch.float32)
    return taps / taps.sum()


def filter_bank():
    """augment.py:175-184: the 4-band bank built from sym2, [4, 43] float32 (numpy.convolve only)."""
    lo = np.asarray(SYM2)                                   # H(z)
    hi = lo * ((-1) ** np.arange(lo.size))                  # H(-z)
    lo2 = np.convolve(lo, lo[::-1]) / 2                     # H(z) H(1/z) / 2
    hi2 = np.convolve(hi, hi[::-1]) / 2                     # H(-z) H(-1/z) / 2
    bank = np.eye(4, 1)
    for i in range(1, bank.shape[0]):
        up = np.zeros([bank.shape[0], bank.shape[1] * 2 - 1])
        up[:, ::2] = bank                                   # zero-stuffing
        bank = np.stack([np.convolve(row, lo2) for row in up])
        c = bank.shape[1]
        bank[i, (c - hi2.size) // 2: (c + hi2.size) // 2] += hi2
    return torch.as_tensor(bank, dtype=torch.float32)


@dataclass
class AugmentParams:
    """Per-sample parameters on the device; a stage whose entry is None is skipped."""
    G_inv: Optional[torch.Tensor] = None          # [B,3,3] pixel_out -> pixel_in
    C: Optional[torch.Tensor] = None              # [B,4,4] colour_in -> colour_out
    gains: Optional[torch.Tensor] = None          # [B,4] band gains of the image-space filter
    noise_sigma: Optional[torch.Tensor] = None    # [B]
    cutout: Optional[torch.Tensor] = None         # [B,4] size_x, size_y, centre_x, centre_y (relative)


def _check(x, what):
    _lib.require_cuda(x, what)
    if x.dtype != torch.float32:
        raise RuntimeError(f'{what} must be float32 (got {x.dtype})')


def _geom_launch(x, G_inv, f, adjoint):
    B, C, H, W = x.shape
    x, G, f = x.contiguous(), _lib.f32c(G_inv), _lib.f32c(f)
    if G.shape != (B, 3, 3) or f.numel() != 12:
        raise RuntimeError(f'augment geometry: G_inv {tuple(G.shape)} for a batch of {B}, {f.numel()} filter taps (12 expected)')
    y = torch.empty_like(x)
    if not adjoint:
        _lib.call('tdgp_augment_geom', _lib.ptr(x), _lib.ptr(G), _lib.ptr(f), _lib.ptr(y), B, C, H, W, _lib.stream_of(x))
    else:
        need = int(_lib.load().tdgp_augment_geom_adj_workspace_bytes(B, C, H, W))
        if need < 0:
            raise RuntimeError(f'augment geometry: shape {tuple(x.shape)} refused')
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
        _lib.call('tdgp_augment_geom_adj', _lib.ptr(x), _lib.ptr(G), _lib.ptr(f), _lib.ptr(y), B, C, H, W, _lib.ptr(ws), need, _lib.stream_of(x))
    return y


class _Geom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, G_inv, f):
        ctx.save_for_backward(G_inv, f)
        return _geom_launch(x, G_inv, f, adjoint=False)

    @staticmethod
    def backward(ctx, dy):
        G_inv, f = ctx.saved_tensors
        return _GeomAdj.apply(dy, G_inv, f), None, None


class _GeomAdj(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, G_inv, f):
        ctx.save_for_backward(G_inv, f)
        return _geom_launch(dy, G_inv, f, adjoint=True)

    @staticmethod
    def backward(ctx, v):
        G_inv, f = ctx.saved_tensors
        return _Geom.apply(v, G_inv, f), None, None


def _color_launch(x, Cm, transposed, use_bias, noise, sigma, cutout, ncc):
    B, C, H, W = x.shape
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.call('tdgp_augment_color', _lib.ptr(x), _lib.ptr(y), _lib.ptr(Cm), int(transposed), int(use_bias), _lib.ptr(noise), _lib.ptr(sigma),
              _lib.ptr(cutout), B, C, H, W, int(ncc), _lib.stream_of(x))
    return y


class _Color(torch.autograd.Function):
    """y = mask * (M x + bias + sigma * noise); its backward is itself with the transposed matrix, no bias and no noise."""
    @staticmethod
    def forward(ctx, x, Cm, transposed, use_bias, noise, sigma, cutout, ncc):
        ctx.save_for_backward(Cm, cutout)
        ctx.transposed, ctx.ncc = transposed, ncc
        return _color_launch(x, Cm, transposed, use_bias, noise, sigma, cutout, ncc)

    @staticmethod
    def backward(ctx, dy):
        Cm, cutout = ctx.saved_tensors
        return (_Color.apply(dy, Cm, not ctx.transposed, False, None, None, cutout, ctx.ncc),) + (None,) * 7


def _image_filter(images, gains, Hz_fbank):
    """augment.py:405-415: reflect pad, then two grouped conv2d with the per-sample g @ Hz_fbank (eager; gradients are torch's own)."""
    B, C, H, W = images.shape
    taps = (gains @ Hz_fbank).unsqueeze(1).repeat([1, C, 1]).reshape([B * C, 1, -1])
    p = Hz_fbank.shape[1] // 2
    x = images.reshape([1, B * C, H, W])
    x = torch.nn.functional.pad(x, [p, p, p, p], mode='reflect')
    x = torch.nn.functional.conv2d(x, taps.unsqueeze(2), groups=B * C)
    x = torch.nn.functional.conv2d(x, taps.unsqueeze(3), groups=B * C)
    return x.reshape([B, C, H, W])


class AugmentPipe(torch.nn.Module):
    def __init__(self,
                 xflip=0, rotate90=0, xint=0, xint_max=0.125,
                 scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2, xfrac_std=0.125,
                 brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1, saturation_std=1,
                 imgfilter=0, imgfilter_bands=[1, 1, 1, 1], imgfilter_std=1,
                 noise=0, cutout=0, noise_std=0.1, cutout_size=0.5):
        super().__init__()
        self.register_buffer('p', torch.ones([]))             # overall multiplier of every probability
        self.xflip, self.rotate90, self.xint, self.xint_max = float(xflip), float(rotate90), float(xint), float(xint_max)
        self.scale, self.rotate, self.aniso, self.xfrac = float(scale), float(rotate), float(aniso), float(xfrac)
        self.scale_std, self.rotate_max, self.aniso_std, self.xfrac_std = float(scale_std), float(rotate_max), float(aniso_std), float(xfrac_std)
        self.brightness, self.contrast, self.lumaflip, self.hue, self.saturation = float(brightness), float(contrast), float(lumaflip), float(hue), float(saturation)
        self.brightness_std, self.contrast_std, self.hue_max, self.saturation_std = float(brightness_std), float(contrast_std), float(hue_max), float(saturation_std)
        self.imgfilter, self.imgfilter_bands, self.imgfilter_std = float(imgfilter), list(imgfilter_bands), float(imgfilter_std)
        self.noise, self.cutout, self.noise_std, self.cutout_size = float(noise), float(cutout), float(noise_std), float(cutout_size)
        if len(self.imgfilter_bands) != 4:
            raise ValueError('imgfilter_bands must name 4 bands')
        self.ada_stats = None                                 # [sum of sign(real logits), count] on the device (training.AdaController); not a buffer
        self.register_buffer('Hz_geom', geom_filter())
        self.register_buffer('Hz_fbank', filter_bank())

    @torch.no_grad()
    def accumulate_signs(self, real_logits):
        """The controller's statistic (training_loop.py:355): adds sign(real logits) and their number to a device-side pair; no host read."""
        signs = real_logits.detach().sign().float()
        add = torch.stack([signs.sum(), signs.new_tensor(float(signs.numel()))])
        self.ada_stats = add if self.ada_stats is None else self.ada_stats + add

    def _cfg(self):
        vals = [self.xflip, self.rotate90, self.xint, self.xint_max, self.scale, self.rotate, self.aniso, self.xfrac, self.scale_std, self.rotate_max,
                self.aniso_std, self.xfrac_std, self.brightness, self.contrast, self.lumaflip, self.hue, self.saturation, self.brightness_std,
                self.contrast_std, self.hue_max, self.saturation_std, self.imgfilter, *[float(b) for b in self.imgfilter_bands], self.imgfilter_std,
                self.noise, self.cutout, self.noise_std, self.cutout_size]
        assert len(vals) == _CFG_FLOATS
        return (ctypes.c_float * _CFG_FLOATS)(*vals)

    def params(self, batch, height, width, debug_percentile=None, num_channels=3):
        """One launch -> AugmentParams.  Random draws: one `torch.rand` and one `torch.randn` block of the current generator.
        `num_channels`: the reference leaves hue and saturation out for one-channel images (augment.py:341, 349)."""
        _lib.require_cuda(self.p, 'AugmentPipe')
        dev = self.p.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
        geom = any(v > 0 for v in (self.xflip, self.rotate90, self.xint, self.scale, self.rotate, self.aniso, self.xfrac))
        color = any(v > 0 for v in (self.brightness, self.contrast, self.lumaflip)) or (num_channels > 1 and (self.hue > 0 or self.saturation > 0))
        out = AugmentParams(G_inv=new(batch, 3, 3) if geom else None, C=new(batch, 4, 4) if color else None,
                            gains=new(batch, 4) if self.imgfilter > 0 else None, noise_sigma=new(batch) if self.noise > 0 else None,
                            cutout=new(batch, 4) if self.cutout > 0 else None)
        if debug_percentile is None:
            u, n = torch.rand([batch, _UNIFORMS], device=dev), torch.randn([batch, _NORMALS], device=dev)
        else:
            u = n = None
        with torch.cuda.device(dev):
            _lib.call('tdgp_augment_params', self._cfg(), _lib.ptr(self.p), int(batch), int(height), int(width), int(num_channels), _lib.ptr(u), _lib.ptr(n),
                      int(debug_percentile is not None), float(0.0 if debug_percentile is None else debug_percentile), _lib.ptr(out.G_inv),
                      _lib.ptr(out.C), _lib.ptr(out.gains), _lib.ptr(out.noise_sigma), _lib.ptr(out.cutout), torch.cuda.current_stream(dev).cuda_stream)
        return out

    def apply(self, images, params=None, num_color_channels=None):
        """The pipe for given parameters: geometry, colour, image-space filter, noise, cutout -- each only when `params` carries it.
        (`torch.nn.Module.apply(fn)` keeps working: a callable first argument goes to it.)"""
        if callable(images) and params is None:
            return super().apply(images)
        _check(images, 'images')
        if images.ndim != 4:
            raise RuntimeError(f'images must be [B,C,H,W] (got {tuple(images.shape)})')
        C = images.shape[1]
        if params.C is not None and (num_color_channels not in (1, 3) or num_color_channels > C):
            raise ValueError('Image must be RGB (3 channels) or L (1 channel)')
        x = images
        if params.G_inv is not None:
            x = _Geom.apply(x, params.G_inv, self.Hz_geom)
        noise = torch.randn(images.shape, device=images.device) if params.noise_sigma is not None else None
        tail = noise is not None or params.cutout is not None
        if params.gains is None:
            if params.C is not None or tail:
                x = _Color.apply(x, params.C, False, True, noise, params.noise_sigma, params.cutout, num_color_channels)
        else:
            if params.C is not None:
                x = _Color.apply(x, params.C, False, True, None, None, None, num_color_channels)
            x = _image_filter(x, params.gains, self.Hz_fbank)
            if tail:
                x = _Color.apply(x, None, False, False, noise, params.noise_sigma, params.cutout, num_color_channels)
        return x

    def forward(self, images, num_color_channels, debug_percentile=None, num_frames=1):
        if num_frames != 1:
            raise NotImplementedError('AugmentPipe: num_frames != 1 (per-frame colour transforms of video batches) is not built')
        _check(images, 'images')
        B, C, H, W = images.shape
        return self.apply(images, self.params(B, H, W, debug_percentile=debug_percentile, num_channels=C), num_color_channels)

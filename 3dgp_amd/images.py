"""Anti-aliased resampling of 8-bit images and 16-bit depth maps with Pillow's arithmetic, on the device and on the host.

The reference prepares its datasets through Pillow (torchvision's `center_crop` / `resize` on PIL images): `center_resize_crop`
(`scripts/utils.py:116-120`, Lanczos) in `resize_dataset.py`, and the eval transform timm resolves for its embedder in `extract_features.py`
(bicubic resize of the shorter side to 256, centre crop to 224, `/255`, normalise).  Pillow's resampling is fully defined for 8-bit images and
for 16-bit `I;16` maps, so it is stated here as a contract (include/tdgp.h, tdgp_resample_*) and held bit for bit:

  * tables per (in_size, out_size, filter), built on the host in Python floats: `resample_tables`;
  * two separable passes, horizontal first, the horizontal one rounded to the sample type before the vertical one runs; a pass whose size
    does not change is skipped;
  * 8 bit: int32 coefficients on a 2^22 scale, `clip((2^21 + sum pixel * k) >> 22, 0, 255)`;
  * 16 bit: float64 coefficients, a rounded product and a rounded sum per tap, Pillow's byte pair on store (`overflow='pillow'`: a value
    above 65535 comes out as `0xFF00 | (v & 255)`) or a clamp of the last pass (`overflow='saturate'`).

A device tensor goes through the HIP kernels (csrc/resample.hip), a numpy array or CPU tensor through vectorised numpy with the same contract,
so every function here also works without a GPU.
"""
import collections
import functools
import math

import numpy as np
import torch

FILTER_SUPPORT = dict(lanczos=3.0, bicubic=2.0, bilinear=1.0)
PRECISION_BITS = 22           # 32 - 8 - 2: Pillow's fixed point for 8-bit coefficients
MAX_SIZE = 32768              # per axis (include/tdgp.h)
DETECTOR_MEAN = (0.485, 0.456, 0.406)
DETECTOR_STD = (0.229, 0.224, 0.225)


# ----------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


_FILTERS = dict(lanczos=_lanczos, bicubic=_bicubic, bilinear=_bilinear)


def _check_filter(filter):
    if filter not in _FILTERS:
        raise ValueError(f'filter {filter!r}: one of {sorted(_FILTERS)}')


@functools.lru_cache(maxsize=256)
def resample_tables(in_size, out_size, filter='lanczos', bits=8):
    """Pillow's coefficient tables of one axis -> (bounds int32 [out_size, 2] = (first source index, taps), coeffs [out_size, ksize]: int32 on
    the 2^22 scale for `bits=8`, float64 for `bits=16`).  Built in Python floats; cached; the arrays are read-only."""
    _check_filter(filter)
    in_size, out_size = int(in_size), int(out_size)
    if bits not in (8, 16):
        raise ValueError(f'bits = {bits!r}: 8 or 16')
    if not (1 <= in_size <= MAX_SIZE and 1 <= out_size <= MAX_SIZE):
        raise ValueError(f'resample_tables: {in_size} -> {out_size}: sizes lie in [1, {MAX_SIZE}]')
    fn = _FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale                  # Pillow multiplies by this rounded reciprocal; dividing instead moves 16-bit pixels by one unit
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, ksize), np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * inv) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        weights[xx, :xmax] = w
    if bits == 16:
        coeffs = weights
    else:
        coeffs = np.array([[int(v * (1 << PRECISION_BITS) + (0.5 if v >= 0 else -0.5)) for v in row] for row in weights.tolist()], dtype=np.int64)
        worst = int(np.abs(coeffs).sum(axis=1).max())
        assert 255 * worst + (1 << (PRECISION_BITS - 1)) < (1 << 31), f'resample_tables({in_size}, {out_size}, {filter!r}): the int32 sum can overflow'
        coeffs = coeffs.astype(np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


_DEVICE_TABLES = collections.OrderedDict()          # (in, out, filter, bits, device) -> (bounds, coeffs, stream they were uploaded on), least recently used first
DEVICE_TABLES_KEPT = 1024


def _device_tables(in_size, out_size, filter, bits, device):
    """The tables of one axis on `device`, uploaded once and kept while they are among the DEVICE_TABLES_KEPT most recently used.  A use on
    another stream than the one they were uploaded on is recorded with the allocator (`record_stream`), so that an evicted table's memory is not
    handed out again while a kernel launched there may still read it."""
    key = (in_size, out_size, filter, bits, str(device))
    stream = torch.cuda.current_stream(device)
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        bounds, coeffs = resample_tables(in_size, out_size, filter, bits)
        hit = _DEVICE_TABLES[key] = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coeffs.copy()).to(device), stream)
        if len(_DEVICE_TABLES) > DEVICE_TABLES_KEPT:
            _DEVICE_TABLES.popitem(last=False)
    else:
        _DEVICE_TABLES.move_to_end(key)
        if stream != hit[2]:
            hit[0].record_stream(stream)
            hit[1].record_stream(stream)
    return hit[0], hit[1]


# ----------------------------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------------------------
def center_crop_box(h, w, ch, cw):
    """(top, left) of torchvision's centre crop: Python's `round` (half to even) of half the margin."""
    if ch > h or cw > w:
        raise ValueError(f'center_crop_box: a {ch} x {cw} crop does not fit a {h} x {w} image')
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))


def resized_shape(h, w, size):
    """torchvision's rule for an int `size`: the shorter side becomes `size`, the longer one `int(size * long / short)`."""
    size = int(size)
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def _size_pair(size):
    if isinstance(size, (tuple, list)):
        oh, ow = size
        return int(oh), int(ow)
    return int(size), int(size)


# ----------------------------------------------------------------------------------------------------------------------
# host path
# ----------------------------------------------------------------------------------------------------------------------
def _pack16(ss, saturate):
    """float64 sums -> stored 16-bit values (include/tdgp.h): v = int(ss +- 0.5); Pillow's byte pair, or the clamp."""
    v = np.trunc(np.where(ss < 0.0, ss - 0.5, ss + 0.5)).astype(np.int64)
    over = (0xFF00 | (v & 255)) if not saturate else np.int64(65535)
    return np.where(v <= 0, 0, np.where(v > 65535, over, v)).astype(np.uint16)


def _pass_host(x, axis, out_size, filter, bits, saturate=False):
    """One pass along `axis` of a numpy array (uint8 or uint16)."""
    in_size = x.shape[axis]
    bounds, coeffs = resample_tables(in_size, out_size, filter, bits)
    ksize = coeffs.shape[1]
    x = np.moveaxis(x, axis, -1)
    first = bounds[:, 0].astype(np.int64)
    if bits == 8:
        acc = np.full(x.shape[:-1] + (out_size,), 1 << (PRECISION_BITS - 1), np.int32)
        for t in range(ksize):                              # coefficients past a row's taps are zero
            acc += x[..., np.minimum(first + t, in_size - 1)].astype(np.int32) * coeffs[:, t]
        out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    else:
        acc = np.zeros(x.shape[:-1] + (out_size,), np.float64)
        for t in range(ksize):
            acc = acc + x[..., np.minimum(first + t, in_size - 1)].astype(np.float64) * coeffs[:, t]
        out = _pack16(acc, saturate)
    return np.moveaxis(out, -1, axis)


def _resize_host(x, bits, box, oh, ow, filter, saturate):
    """x: numpy [B, H, W, C] uint8 or [B, H, W] uint16."""
    x0, y0, w, h = box
    x = x[:, y0:y0 + h, x0:x0 + w]
    if ow != w:
        x = _pass_host(x, 2, ow, filter, bits, saturate and oh == h)
    if oh != h:
        x = _pass_host(x, 1, oh, filter, bits, saturate)
    return np.ascontiguousarray(x)


# ----------------------------------------------------------------------------------------------------------------------
# device path
# ----------------------------------------------------------------------------------------------------------------------
def _axis_tables(in_size, out_size, filter, bits, device):
    if in_size == out_size:
        return None, None, 0
    bounds, coeffs = _device_tables(in_size, out_size, filter, bits, device)
    return bounds, coeffs, int(coeffs.shape[1])


def _resize_device(x, bits, box, oh, ow, filter, saturate, out):
    """x: device tensor [B, H, W, C] uint8 or [B, H, W] int16 (the bits of uint16), contiguous."""
    from . import _lib
    _lib.require_cuda(x, 'resample: x')
    _lib.require_cuda(out, 'resample: out')
    x0, y0, w, h = box
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    C = int(x.shape[3]) if bits == 8 else 1
    hb, hk, hks = _axis_tables(w, ow, filter, bits, x.device)
    vb, vk, vks = _axis_tables(h, oh, filter, bits, x.device)
    ws, need = _lib.byte_workspace('tdgp_resample_workspace_bytes', (B, h, w, oh, ow, C, bits // 8), x.device,
                                   RuntimeError(f'tdgp_resample refuses {B} x {h} x {w} -> {oh} x {ow}'))
    ws = ws if need else None                                          # bytes; torch's allocations are aligned far beyond a sample
    with torch.cuda.device(x.device):
        if bits == 8:
            _lib.call('tdgp_resample_u8', x.data_ptr(), B, H, W, C, x0, y0, w, h, _lib.ptr(hb), _lib.ptr(hk), hks, _lib.ptr(vb), _lib.ptr(vk), vks,
                      out.data_ptr(), oh, ow, _lib.ptr(ws), need, _lib.stream_of(x))
        else:
            _lib.call('tdgp_resample_u16', x.data_ptr(), B, H, W, x0, y0, w, h, _lib.ptr(hb), _lib.ptr(hk), hks, _lib.ptr(vb), _lib.ptr(vk), vks,
                      out.data_ptr(), oh, ow, int(saturate), _lib.ptr(ws), need, _lib.stream_of(x))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# public
# ----------------------------------------------------------------------------------------------------------------------
def _as_bits16(t):
    """A 16-bit-scale tensor (uint16 or int32 in [0, 65535]) as int16 carrying the same low 16 bits."""
    if t.dtype == torch.uint16:
        return t.view(torch.int16)
    return t.to(torch.int16)                      # wraps: the low 16 bits


def _check_box(box, H, W):
    if box is None:
        return 0, 0, W, H
    x0, y0, w, h = (int(v) for v in box)
    if not (w >= 1 and h >= 1 and 0 <= x0 <= W - w and 0 <= y0 <= H - h):
        raise ValueError(f'box (x0 {x0}, y0 {y0}, w {w}, h {h}) does not lie inside the {H} x {W} image')
    return x0, y0, w, h


def resize(x, size, filter='lanczos', box=None, overflow='pillow', out=None):
    """Pillow's `Image.resize(size, filter)` of `x`, or of its window `box = (x0, y0, w, h)` as if cropped first.

    x: uint8 [B, H, W, C] / [H, W, C] with C in {1, 3}, or a depth map on the 16-bit scale, uint16 or int32, [B, H, W] / [H, W].  `size`: an
    int (square) or (oh, ow).  `filter`: 'lanczos', 'bicubic' or 'bilinear'.  `overflow` (16 bit only): 'pillow' stores Pillow's bytes,
    'saturate' clamps what the last pass stores to 65535.  A GPU tensor runs the kernels and returns a GPU tensor (`out`: a contiguous tensor
    of the result's shape and dtype to write into, GPU route only); a numpy array or CPU tensor takes the host path and comes back as what it
    was.  The result has the input's dtype and rank.

    An int32 depth map must lie in [0, 65535].  The host path checks that and raises; the GPU route does NOT (a check would read the tensor back
    and synchronise): there a value outside the range is taken by its low 16 bits."""
    _check_filter(filter)
    if overflow not in ('pillow', 'saturate'):
        raise ValueError(f"overflow {overflow!r}: 'pillow' or 'saturate'")
    oh, ow = _size_pair(size)
    if not (1 <= oh <= MAX_SIZE and 1 <= ow <= MAX_SIZE):
        raise ValueError(f'resize: output {oh} x {ow}: sizes lie in [1, {MAX_SIZE}]')
    is_tensor = isinstance(x, torch.Tensor)
    dtype = x.dtype
    name = str(dtype).replace('torch.', '')
    if name == 'uint8':
        bits, full_rank = 8, 4
    elif name in ('uint16', 'int32'):
        bits, full_rank = 16, 3
    else:
        raise TypeError(f'resize takes uint8 images or uint16 / int32 depth maps, not {name}')
    if x.ndim not in (full_rank - 1, full_rank):
        raise ValueError(f'resize: expected {"[B, H, W, C] or [H, W, C]" if bits == 8 else "[B, H, W] or [H, W]"}, got shape {tuple(x.shape)}')
    single = x.ndim == full_rank - 1
    if single:
        x = x[None]
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if bits == 8 and int(x.shape[3]) not in (1, 3):
        raise ValueError(f'resize: C = {int(x.shape[3])} channels, 1 or 3 are supported')
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f'resize: input {H} x {W}: sizes lie in [1, {MAX_SIZE}]')
    box = _check_box(box, H, W)
    saturate = overflow == 'saturate'
    out_shape = (B, oh, ow) + ((int(x.shape[3]),) if bits == 8 else ())

    if is_tensor and x.is_cuda:
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == dtype and out.is_contiguous()
                    and tuple(out.shape) in (out_shape, out_shape[1:] if single else out_shape)):
                raise ValueError(f'resize: out must be a contiguous {name} tensor of shape {out_shape[1:] if single else out_shape} on {x.device}')
        x = x.contiguous()
        if bits == 8:
            res = torch.empty(out_shape, dtype=dtype, device=x.device) if out is None else out
            _resize_device(x, 8, box, oh, ow, filter, False, res)
        elif dtype == torch.uint16:
            res = torch.empty(out_shape, dtype=dtype, device=x.device) if out is None else out
            _resize_device(x.view(torch.int16), 16, box, oh, ow, filter, saturate, res)
        else:
            tmp = torch.empty(out_shape, dtype=torch.int16, device=x.device)
            _resize_device(_as_bits16(x), 16, box, oh, ow, filter, saturate, tmp)
            wide = tmp.to(torch.int32) & 0xFFFF
            res = wide if out is None else out.copy_(wide.reshape(out.shape))
        return res[0] if single and res.ndim == full_rank else res

    if out is not None:
        raise ValueError('resize: out= is for the GPU route')
    a = x.detach().numpy() if is_tensor and dtype != torch.uint16 else (x.view(torch.int16).numpy().view(np.uint16) if is_tensor else np.asarray(x))
    if bits == 16:
        if a.dtype != np.uint16 and (a.min(initial=0) < 0 or a.max(initial=0) > 65535):
            raise ValueError('resize: an int32 depth map must lie on the 16-bit scale, [0, 65535]')
        res = _resize_host(a.astype(np.uint16), 16, box, oh, ow, filter, saturate).astype(a.dtype)
    else:
        res = _resize_host(a, 8, box, oh, ow, filter, False)
    if single:
        res = res[0]
    if is_tensor:
        return torch.from_numpy(res.view(np.int16)).view(torch.uint16) if dtype == torch.uint16 else torch.from_numpy(res)
    return res


def center_resize_crop(x, size, filter='lanczos'):
    """The reference's `center_resize_crop` (`scripts/utils.py:116-120`): centre crop to min(h, w) square, then resize to `size`^2.  An input
    that is already `size`^2 is returned unchanged."""
    size = int(size)
    lead = x.ndim - (3 if str(x.dtype).replace('torch.', '') == 'uint8' else 2)
    if lead not in (0, 1):
        raise ValueError(f'center_resize_crop: unexpected shape {tuple(x.shape)}')
    h, w = int(x.shape[lead]), int(x.shape[lead + 1])
    if h == size and w == size:
        return x
    side = min(h, w)
    top, left = center_crop_box(h, w, side, side)
    return resize(x, size, filter=filter, box=(left, top, side, side))


def detector_input(x_u8, resize=256, crop=224, filter='bicubic', mean=DETECTOR_MEAN, std=DETECTOR_STD):
    """uint8 [B, H, W, C] (C in {1, 3}) -> fp32 [B, C, crop, crop]: the eval transform timm resolves for the reference's default embedder
    (`extract_features.py`): the shorter side resized to `resize` (bicubic, Pillow's bytes), centre crop, `/ 255`, `- mean`, `/ std`, every
    fp32 operation rounded on its own.  On a GPU tensor this is one horizontal and one fused vertical launch on the uint8 input (the resized
    image is never stored); on the host the same chain in numpy."""
    _check_filter(filter)
    is_tensor = isinstance(x_u8, torch.Tensor)
    if str(x_u8.dtype).replace('torch.', '') != 'uint8' or x_u8.ndim != 4 or int(x_u8.shape[3]) not in (1, 3):
        raise ValueError(f'detector_input takes uint8 [B, H, W, C] with C in (1, 3), got {x_u8.dtype} {tuple(x_u8.shape)}')
    B, H, W, C = (int(v) for v in x_u8.shape)
    crop = int(crop)
    oh, ow = resized_shape(H, W, resize)
    if not (1 <= oh <= MAX_SIZE and 1 <= ow <= MAX_SIZE):
        raise ValueError(f'detector_input: resized image {oh} x {ow}: sizes lie in [1, {MAX_SIZE}]')
    top, left = center_crop_box(oh, ow, crop, crop)
    mean32, std32 = np.asarray(mean, np.float32).reshape(-1), np.asarray(std, np.float32).reshape(-1)
    if len(mean32) != C or len(std32) != C or (std32 == 0).any():
        raise ValueError(f'detector_input: mean and std must hold {C} values, std non-zero')

    if is_tensor and x_u8.is_cuda:
        import ctypes
        from . import _lib
        x = x_u8.contiguous()
        hb, hk, hks = _axis_tables(W, ow, filter, 8, x.device)
        vb, vk, vks = _axis_tables(H, oh, filter, 8, x.device)
        ws, need = _lib.byte_workspace('tdgp_resample_u8_to_f32_workspace_bytes', (B, H, W, oh, ow, C, crop), x.device,
                                       RuntimeError(f'tdgp_resample_u8_to_f32 refuses {B} x {H} x {W} -> {oh} x {ow}'))
        ws = ws if need else None
        res = torch.empty([B, C, crop, crop], dtype=torch.float32, device=x.device)
        fl = ctypes.c_float * C
        with torch.cuda.device(x.device):
            _lib.call('tdgp_resample_u8_to_f32', x.data_ptr(), B, H, W, C, 0, 0, W, H, _lib.ptr(hb), _lib.ptr(hk), hks, _lib.ptr(vb), _lib.ptr(vk), vks,
                      oh, ow, left, top, crop, crop, fl(*mean32.tolist()), fl(*std32.tolist()), res.data_ptr(), _lib.ptr(ws), need, _lib.stream_of(x))
        return res

    a = x_u8.detach().numpy() if is_tensor else np.asarray(x_u8)
    # the whole resized image on the host; the crop cuts it afterwards (the bytes inside the window are the same either way)
    r = a
    if ow != W:
        r = _pass_host(r, 2, ow, filter, 8)
    if oh != H:
        r = _pass_host(r, 1, oh, filter, 8)
    r = r[:, top:top + crop, left:left + crop].transpose(0, 3, 1, 2)
    res = np.ascontiguousarray(((r.astype(np.float32) / np.float32(255.0)) - mean32[None, :, None, None]) / std32[None, :, None, None])
    return torch.from_numpy(res) if is_tensor else res

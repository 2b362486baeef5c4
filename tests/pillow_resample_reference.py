"""Plain-loop restatement of the resampling contract (include/tdgp.h, tdgp_resample_*; Pillow's Resample.c arithmetic) and the shared
test cases.  Written independently of 3dgp_amd/images.py: tables row by row in Python floats, one output row / column at a time, taps in
order.  Test infrastructure only -- the product never imports it.

Inputs regenerate from seeds (`make_input`); `CASES_U8` / `CASES_U16` are the cases tests/golden/resample.npz was generated for
(tools/gen_resample_goldens.py), the CPU tests compare with live Pillow and the GPU tests with the golden.
"""
import functools
import math
import zlib

import numpy as np

FILTERS = ('lanczos', 'bicubic', 'bilinear')
SUPPORT = {'lanczos': 3.0, 'bicubic': 2.0, 'bilinear': 1.0}
KINDS = ('noise', 'ramp', 'stripes')

# (H, W) -> (oh, ow)
SIZES_U8 = (((37, 53), (16, 16)), ((64, 64), (24, 24)), ((17, 17), (40, 40)), ((100, 75), (32, 24)), ((9, 300), (5, 7)), ((33, 33), (33, 20)),
            ((33, 33), (20, 33)), ((33, 33), (33, 33)), ((256, 256), (224, 224)))
SIZES_U16 = SIZES_U8[:4] + (((256, 256), (128, 128)),)
CASES_U8 = tuple((f, hw, out, c, kind) for f in FILTERS for hw, out in SIZES_U8 for c in (1, 3) for kind in KINDS)
CASES_U16 = tuple((f, hw, out, kind) for f in FILTERS for hw, out in SIZES_U16 for kind in KINDS)
# the golden holds Pillow's bytes for a case whose output is at most this many bytes, and their SHA-256 for a larger one
# (the file stays a few hundred KB); the bicubic 256 -> 224 noise image, the detector shape, is kept in full as well
GOLDEN_FULL_BYTES = 8192


def case_key(bits, filter, hw, out, c, kind):
    return f'u{bits}/{filter}/{hw[0]}x{hw[1]}-{out[0]}x{out[1]}/c{c}/{kind}'


def golden_keeps_bytes(bits, filter, hw, out, c, kind):
    return out[0] * out[1] * c * (bits // 8) <= GOLDEN_FULL_BYTES or (bits == 8 and filter == 'bicubic' and c == 3 and kind == 'noise')


def make_input(bits, hw, c, kind, key=''):
    """uint8 [H, W, c] or uint16 [H, W] (c = 1).  `key` seeds the noise."""
    h, w = hw
    top = 255 if bits == 8 else 65535
    i, j, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing='ij')
    if kind == 'noise':
        a = np.random.RandomState(zlib.crc32(f'{key}|{bits}|{h}|{w}|{c}'.encode())).randint(0, top + 1, size=(h, w, c))
    elif kind == 'ramp':
        a = (7 * i + 13 * j + 31 * ch) % 256 if bits == 8 else (311 * i + 173 * j) % 65536
    elif kind == 'stripes':
        a = (((i + j + ch) // 3) % 2) * top
    else:
        raise ValueError(kind)
    a = a.astype(np.uint8 if bits == 8 else np.uint16)
    return a if bits == 8 else a[:, :, 0]


# ----------------------------------------------------------------------------------------------------------------------
# the contract
# ----------------------------------------------------------------------------------------------------------------------
def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _weight(filter, x):
    if filter == 'lanczos':
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    if x < 0.0:
        x = -x
    if filter == 'bicubic':
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if filter == 'bilinear':
        return 1.0 - x if x < 1.0 else 0.0
    raise ValueError(filter)


@functools.lru_cache(maxsize=None)
def rows(in_size, out_size, filter):
    """((xmin, (w0, w1, ...)), ...) per output index: normalised float64 weights of the taps from xmin on; and ksize."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filter] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale                   # Pillow multiplies by the rounded reciprocal; a division moves 16-bit pixels by one unit
    table = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = _weight(filter, (x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        assert len(w) <= ksize
        table.append((xmin, tuple(w)))
    return tuple(table), ksize


def fixed_point(w):
    return int(w * (1 << 22) + 0.5) if w >= 0 else int(w * (1 << 22) - 0.5)


def _pass_u8(img, out_size, filter):
    """Resample axis 1 of uint8 [H, W, C]; returns (uint8 image, pre-clip int values)."""
    table, _ = rows(img.shape[1], out_size, filter)
    pre = np.zeros((img.shape[0], out_size, img.shape[2]), np.int64)
    for xx, (xmin, w) in enumerate(table):
        ss = np.full((img.shape[0], img.shape[2]), 1 << 21, np.int64)
        absk = 0
        for x, v in enumerate(w):
            k = fixed_point(v)
            absk += abs(k)
            ss = ss + img[:, xmin + x, :].astype(np.int64) * k
        assert 255 * absk + (1 << 21) < (1 << 31)            # int32 never overflows, so int64 here is the same arithmetic
        pre[:, xx, :] = ss >> 22
    return np.clip(pre, 0, 255).astype(np.uint8), pre


def _pass_u16(img, out_size, filter, saturate):
    """Resample axis 1 of uint16 [H, W]; returns (uint16 image, pre-clip int values)."""
    table, _ = rows(img.shape[1], out_size, filter)
    pre = np.zeros((img.shape[0], out_size), np.int64)
    for xx, (xmin, w) in enumerate(table):
        ss = np.zeros(img.shape[0], np.float64)
        for x, v in enumerate(w):
            ss = ss + img[:, xmin + x].astype(np.float64) * np.float64(v)        # a rounded product, then a rounded sum
        pre[:, xx] = np.trunc(np.where(ss >= 0.0, ss + 0.5, ss - 0.5)).astype(np.int64)
    v = pre
    hi = np.clip(v >> 8, 0, 255)
    lo = np.clip(np.fmod(v, 256), 0, 255)                      # fmod: C's sign of %
    out = hi * 256 + lo
    if saturate:
        out = np.clip(v, 0, 65535)
    return out.astype(np.uint16), pre


def resize_u8(img, out_hw, filter, box=None, with_preclip=False):
    """uint8 [H, W, C] -> [oh, ow, C].  `box` = (x0, y0, w, h) crops first.  with_preclip: also the pre-clip values of every pass that ran."""
    if box is not None:
        x0, y0, w, h = box
        img = img[y0:y0 + h, x0:x0 + w]
    oh, ow = out_hw
    pres = []
    if ow != img.shape[1]:
        img, pre = _pass_u8(img, ow, filter)
        pres.append(pre)
    if oh != img.shape[0]:
        t, pre = _pass_u8(img.transpose(1, 0, 2), oh, filter)
        img = t.transpose(1, 0, 2)
        pres.append(pre.transpose(1, 0, 2))
    img = np.ascontiguousarray(img)
    return (img, pres) if with_preclip else img


def resize_u16(img, out_hw, filter, overflow='pillow', box=None, with_preclip=False):
    """uint16 [H, W] -> [oh, ow].  overflow='saturate' clamps what the LAST pass stores; the rows between the passes are Pillow's bytes.
    with_preclip: also the pre-clip integer values of the last pass (None for a copy)."""
    assert overflow in ('pillow', 'saturate')
    if box is not None:
        x0, y0, w, h = box
        img = img[y0:y0 + h, x0:x0 + w]
    oh, ow = out_hw
    need_h, need_v = ow != img.shape[1], oh != img.shape[0]
    pre = None
    if need_h:
        img, pre = _pass_u16(img, ow, filter, overflow == 'saturate' and not need_v)
    if need_v:
        t, pre = _pass_u16(img.T, oh, filter, overflow == 'saturate')
        img, pre = t.T, pre.T
    img = np.ascontiguousarray(img)
    return (img, pre) if with_preclip else img


def detector_input(img, resize, crop, filter, mean, std):
    """uint8 [H, W, C] -> float32 [C, crop, crop]: shorter side to `resize`, centre crop, / 255, - mean, / std in fp32."""
    h, w = img.shape[:2]
    if w <= h:
        ow, oh = resize, int(resize * h / w)
    else:
        oh, ow = resize, int(resize * w / h)
    r = resize_u8(img, (oh, ow), filter)
    top, left = int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))
    r = r[top:top + crop, left:left + crop].transpose(2, 0, 1).astype(np.float32)
    out = np.empty_like(r)
    for c in range(r.shape[0]):
        out[c] = ((r[c] / np.float32(255.0)) - np.float32(mean[c])) / np.float32(std[c])
    return out


@functools.lru_cache(maxsize=None)
def expected(bits, filter, hw, out, c, kind):
    """The restatement's output of a shared case, computed once per process (read-only)."""
    x = make_input(bits, hw, c, kind, key=filter)
    y = resize_u8(x, out, filter) if bits == 8 else resize_u16(x, out, filter)
    y.setflags(write=False)
    return y

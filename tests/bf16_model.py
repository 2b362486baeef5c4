"""Float64 model of the reduced-precision (bf16) conv layers with the KERNELS' documented rounding points -- a test helper: no GPU code, no
import of the package's native library.

The rounding points are the contract text's (header of csrc/modconv_bf16.inc, the tdgp_modconv2d_bf16 comment of include/tdgp.h, the YBF comment
above fir_act_kernel), not the kernels' arithmetic:

    3x3 stride 1   a = sum bf16(W) * bf16(x * s)        the product x * s formed in fp32, then rounded; the sum exact (float64)
                   v = bf16(fp32(a) * d)                d: the fp32 demodulation coefficient, handed in as `dcoef`
                   v = bf16(v + n)                      if there is noise
                   y = bf16(clamp(act(v + bf16(bias)) * gain))          fp32 elementwise arithmetic
    3x3 x2         the same operands through conv_transpose2d (stride 2, unflipped weights) into an UNROUNDED intermediate, the 4x4 FIR with
                   gain 4, then * d and the same three roundings
    ToRGB          a = sum W * (x * s)                  fp32 weights and fp32 products x * s, neither rounded to bf16 (fp32 MFMA)
                   q = bf16(clamp((bf16(fp32(a)) + bf16(bias)) * gain)),   y = q + upsample2d(skip)   (fp32 skip, added unrounded)

`accum='f64'` sums exactly; `accum='seq32'` evaluates the SAME model with an fp32 accumulator, one term at a time, left to right over
(channel, tap) (bf16 x bf16 products are exact in fp32: only the additions round; a product that is not exact in fp32 -- FIR tap x
intermediate, fp32 weight x fp32 activation -- is added with one rounding, as a fused multiply-add does).  The outputs whose final bf16
bits differ between the two evaluations are the accumulation-noise yardstick of the GPU tests: `count_seq`.

The shape tables of tests/test_bf16_layers_gpu.py live here so that the CPU test measures the yardstick on exactly those cases."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SQRT2 = float(np.float32(np.sqrt(2.0)))


def bf16(x):
    """fp32 array -> nearest bfloat16 value (ties to even), kept as fp32.  Finite values and infinities."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def bits(v):
    """bf16 values held as fp32 -> their 16 bits."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    assert not (v.view(np.uint32) & np.uint32(0xFFFF)).any(), 'not bf16 values'
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def demod_coefficients(w, s):
    """d[b,o] = (sum_{c,taps} (w[o,c] s[b,c])^2 + 1e-8)^-1/2 of the fp32 weights and styles, in float64, cast to fp32."""
    w2 = np.square(np.asarray(w, np.float64)).sum(axis=(2, 3))                                       # [O,C]
    return (1.0 / np.sqrt(np.square(np.asarray(s, np.float64)) @ w2.T + 1e-8)).astype(np.float32)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _scaled(x, s):
    """x * s in fp32 (x holds bf16 values)."""
    x = np.asarray(x, np.float32)
    return x if s is None else x * np.asarray(s, np.float32)[:, :, None, None]


def fir_taps(f):
    """Taps of the x2 FIR as correlation weights: the flipped filter times the gain 4 (up^2), fp32 values."""
    return (np.asarray(f, np.float32)[::-1, ::-1] * np.float32(4)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ accumulators (fp32 values)
def acc_conv3(x, w, s, accum='f64'):
    xs, wb = bf16(_scaled(x, s)), bf16(w)
    B, cin, H, W = xs.shape
    if accum == 'f64':
        return F.conv2d(_t64(xs), _t64(wb), padding=1).numpy().astype(np.float32)
    xp = np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.zeros((B, wb.shape[0], H, W), np.float32)
    for c in range(cin):
        for ky in range(3):
            for kx in range(3):
                acc += wb[None, :, c, ky, kx, None, None] * xp[:, c, None, ky:ky + H, kx:kx + W]
    return acc


def acc_up2(x, w, s, f, accum='f64'):
    xs, wb, taps = bf16(_scaled(x, s)), bf16(w), fir_taps(f)
    B, cin, H, W = xs.shape
    cout = wb.shape[0]
    if accum == 'f64':
        z = F.conv_transpose2d(_t64(xs), _t64(wb).transpose(0, 1), stride=2)                          # z[2m + a, 2n + e] += x[m, n] w[a, e]
        zp = F.pad(z, (1, 1, 1, 1)).reshape(B * cout, 1, 2 * H + 3, 2 * W + 3)
        return F.conv2d(zp, _t64(taps)[None, None]).reshape(B, cout, 2 * H, 2 * W).numpy().astype(np.float32)
    z = np.zeros((B, cout, 2 * H + 1, 2 * W + 1), np.float32)
    for c in range(cin):
        for a in range(3):
            for e in range(3):
                z[:, :, a:a + 2 * H:2, e:e + 2 * W:2] += wb[None, :, c, a, e, None, None] * xs[:, c, None]
    zp = np.pad(z, ((0, 0), (0, 0), (1, 1), (1, 1))).astype(np.float64)
    acc = np.zeros((B, cout, 2 * H, 2 * W), np.float32)
    for ky in range(4):
        for kx in range(4):
            acc = (acc.astype(np.float64) + taps[ky, kx] * zp[:, :, ky:ky + 2 * H, kx:kx + 2 * W]).astype(np.float32)
    return acc


def acc_torgb(x, w, s, accum='f64'):
    xs, w2 = _scaled(x, s).astype(np.float64), np.asarray(w, np.float32).reshape(w.shape[0], w.shape[1]).astype(np.float64)
    if accum == 'f64':
        return np.einsum('oc,bchw->bohw', w2, xs).astype(np.float32)
    acc = np.zeros((xs.shape[0], w2.shape[0]) + xs.shape[2:], np.float32)
    for c in range(xs.shape[1]):
        acc = (acc.astype(np.float64) + w2[None, :, c, None, None] * xs[:, c, None]).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------ behind the accumulator
def _act_gain_clamp(t, act, alpha, gain, clamp):
    assert t.dtype == np.float32
    if act == 'lrelu':
        t = np.where(t > 0, t, t * np.float32(alpha))
    else:
        assert act == 'linear', act
    t = t * np.float32(gain)
    if clamp is not None and clamp >= 0:
        t = np.clip(t, -np.float32(clamp), np.float32(clamp))
    return t.astype(np.float32)


def layer_tail(acc, dcoef=None, noise=None, bias=None, act='lrelu', alpha=0.2, gain=SQRT2, clamp=None):
    """The three roundings of a 3x3 layer behind its fp32 accumulator `acc` [B,Cout,OH,OW]; noise [OH,OW] or [B,1,OH,OW]."""
    v = np.asarray(acc, np.float32)
    if dcoef is not None:
        v = v * np.asarray(dcoef, np.float32)[:, :, None, None]
    v = bf16(v)
    if noise is not None:
        n = np.asarray(noise, np.float32)
        v = bf16(v + (n[None, None] if n.ndim == 2 else n))
    if bias is not None:
        v = v + bf16(bias)[None, :, None, None]
    return bf16(_act_gain_clamp(v, act, alpha, gain, clamp))


def torgb_tail(acc, bias=None, gain=1.0, clamp=None):
    v = bf16(acc)
    if bias is not None:
        v = v + bf16(bias)[None, :, None, None]
    return bf16(_act_gain_clamp(v, 'linear', 0.0, gain, clamp))


def upsample2d_f64(x, f):
    """upsample2d(x, f) of the skip image (zero insertion, padding [2, 1, 2, 1], the filter times 4 applied as a convolution) in float64."""
    B, C, h, w = x.shape
    up = torch.zeros(B * C, 1, h, 2, w, 2, dtype=torch.float64)
    up[:, :, :, 0, :, 0] = _t64(x).reshape(B * C, 1, h, w)
    up = F.pad(up.reshape(B * C, 1, 2 * h, 2 * w), (2, 1, 2, 1))
    return F.conv2d(up, _t64(fir_taps(f))[None, None]).reshape(B, C, 2 * h, 2 * w).numpy()


# ------------------------------------------------------------------------------------------------ comparison
def count_differing(a, b):
    """(outputs whose bf16 bits differ, largest |a - b| / max|b| among them) of two bf16-valued tensors."""
    diff = bits(a) != bits(b)
    n = int(diff.sum())
    worst = float(np.abs(a.astype(np.float64) - b.astype(np.float64))[diff].max() / np.abs(b).max()) if n else 0.0
    return n, worst


MAX_ONE_OUTPUT = 2.0 ** -6          # of max|ref|: two bf16 ulps at the top of the range


# ------------------------------------------------------------------------------------------------ the cases
# stride 1 (W % 32 == 0), x2 (W even, Cin % 32 == 0): B, Cin, Cout, H, W
STRIDE1_SHAPES = [(2, 32, 64, 8, 32),          # smallest block that spans two samples
                  (3, 64, 40, 9, 32),          # ragged Cout; B (H + 1) not a multiple of 8
                  (2, 96, 130, 16, 64),        # three K chunks; three 64-channel slices with a ragged last
                  (5, 32, 32, 8, 96),          # three column tiles
                  (1, 2048, 32, 8, 32)]        # the Cin limit
UP2_SHAPES = [(8, 64, 32, 4, 4),               # six samples' styles in one block (GS = 32)
              (2, 32, 64, 3, 64),              # OW = 128, OH = 6: the 16 x 128 FIR tiles (lrelu form and, with act='linear', the general one), ragged row tile
              (1, 32, 130, 5, 66),             # OW = 132: ragged column tile; the Cout > 64 plan
              (2, 64, 32, 16, 6),              # 32 x 64 FIR tiles, narrow image
              (3, 32, 48, 7, 10)]              # odd H
NOISES = ['none', 'const', 'per_sample']
ACTS = [('lrelu', 256.0), ('linear', None), ('lrelu', 0.5)]          # (activation, clamp): the blocks' form; no clamp; a clamp that binds
# ToRGB (out_layout = 1): B, Cin, Cout, feat, H, W
TORGB_SHAPES = [(2, 32, 48, 16, 8, 8),         # two 32-row MFMA tiles of output channels
                (3, 24, 24, 8, 6, 10),         # P = 180: ragged 128-pixel tile, not a power of two
                (2, 30, 96, 32, 4, 8),         # Cin % 4 != 0: scalar style loads
                (1, 72, 12, 4, 16, 16),        # Cin > 64: streamed weights, ragged last 64-channel chunk
                (2, 200, 96, 32, 8, 12)]       # four K iterations
TORGB_FORMS = [(1.0, 256.0), (0.75, 0.5)]      # (gain, clamp)
FIR = (np.outer([1, 3, 3, 1], [1, 3, 3, 1]) / 64.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def conv_case(up, shape, styled=True):
    """Inputs and the two accumulators of one 3x3 case (computed once, shared by every noise / activation variant and by the CPU and GPU
    tests; treat as read-only)."""
    B, cin, cout, H, W = shape
    rs = np.random.RandomState(1000 * up + 7 * B + cin + cout + H + W)
    x = bf16(rs.randn(B, cin, H, W).astype(np.float32))
    w = rs.randn(cout, cin, 3, 3).astype(np.float32)
    s = (1.0 + 0.5 * rs.randn(B, cin)).astype(np.float32) if styled else None
    c = dict(x=x, w=w, s=s, dcoef=demod_coefficients(w, s) if styled else None, bias=rs.randn(cout).astype(np.float32),
             noise_const=(0.3 * rs.randn(H * up, W * up)).astype(np.float32), noise_per_sample=(0.3 * rs.randn(B, 1, H * up, W * up)).astype(np.float32))
    for accum in ('f64', 'seq32'):
        c['acc_' + accum] = acc_conv3(x, w, s, accum) if up == 1 else acc_up2(x, w, s, FIR, accum)
    return c


def conv_expect(c, noise, act, clamp):
    """(float64-accumulated model output, sequential-fp32 one) of a variant of `conv_case`."""
    kw = dict(dcoef=c['dcoef'], noise=None if noise == 'none' else c['noise_' + noise], bias=c['bias'], act=act, alpha=0.2 if act == 'lrelu' else 0.0,
              gain=SQRT2 if act == 'lrelu' else 1.0, clamp=clamp)
    return layer_tail(c['acc_f64'], **kw), layer_tail(c['acc_seq32'], **kw)


@functools.lru_cache(maxsize=None)
def torgb_case(shape):
    B, cin, cout, feat, H, W = shape
    rs = np.random.RandomState(3000 + 7 * B + cin + cout + H + W)
    x = bf16(rs.randn(B, cin, H, W).astype(np.float32))
    w = (rs.randn(cout, cin, 1, 1) / np.sqrt(cin)).astype(np.float32)
    s = (1.0 + 0.5 * rs.randn(B, cin)).astype(np.float32)
    prev = rs.randn(B, cout, H // 2, W // 2).astype(np.float32)
    c = dict(x=x, w=w, s=s, bias=rs.randn(cout).astype(np.float32), prev=prev, skip_up=upsample2d_f64(prev, FIR), skip_abs_up=upsample2d_f64(np.abs(prev), FIR))
    for accum in ('f64', 'seq32'):
        c['acc_' + accum] = acc_torgb(x, w, s, accum)
    return c


def torgb_expect(c, gain, clamp):
    return torgb_tail(c['acc_f64'], c['bias'], gain, clamp), torgb_tail(c['acc_seq32'], c['bias'], gain, clamp)

"""A plain-torch restatement of `AugmentPipe.apply` (3dgp_amd/augment.py) for arbitrary per-sample parameters: test infrastructure, the
yardstick where the goldens cannot reach (they give every sample of a batch the same transform) and the eager baseline of
tools/bench_augment.py.  Nothing under 3dgp_amd/ imports it.

Any dtype, any device: eager reflect pad / zero-stuffing upsampling (`upfirdn2d(impl='ref')`) / `affine_grid` / `grid_sample` / downsampling,
colour matrix, band filter, noise, cutout, in the order and with the expressions of the reference's pipe.  tests/test_augment.py pins it to
the reference's recorded float64 outputs and gradients on the CPU (same expression, same float32 taps: only float64 rounding apart).

Also here: the loader of the goldens tools/gen_augment_goldens.py writes, and the bound every augmentation test uses.
"""
import importlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = dict(rgbd=3, rgb16=3, luma16=1, patch64=3, filt=3)               # name -> colour channels (tools/gen_augment_goldens.py:CASES)
BASE = dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1)
CASE_KW = dict(rgbd=BASE, rgb16=BASE, luma16=BASE, patch64=BASE, filt=dict(BASE, imgfilter=1, cutout=1))
PERCENTILES = (0.02, 0.1, 0.35, 0.5, 0.7, 0.93, 0.98)

_top = None


def golden_top():
    global _top
    if _top is None:
        _top = dict(np.load(os.path.join(GOLDEN, 'augment.npz')))
    return _top


def load_case(name, q):
    """-> dict(x, dy, y64, dx64, y32, dx32) of one golden case at one percentile (the fp32 run unpacked from its float16 difference)."""
    top = golden_top()
    g = dict(np.load(os.path.join(GOLDEN, 'augment', f'{name}_q{int(round(q * 100)):02d}.npz')))
    out = dict(x=top[name + '_x'], dy=top[name + '_dy'], y64=g['y64'], dx64=g['dx64'])
    for k in ('y', 'dx'):
        out[k + '32'] = (g[k + '64'] + g[k + '32_d16'].astype(np.float64) * float(g[k + '32_scale'])).astype(np.float32)
    return out


def within_reference_noise(got, ref64, ref32, what, report=None):
    """The project's bound (tests/test_field_deep_gpu.py): e_ref = max |reference fp32 - reference float64|, e_hip = max |got - reference
    float64|, both over max(1, max |reference|); e_hip <= 2 max(e_ref, 2^-23)."""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, f'{what}: shapes {got.shape} {ref64.shape} {ref32.shape}'
    scale = max(1.0, float(np.abs(ref64).max()))
    e_ref, e_hip = float(np.abs(ref32 - ref64).max()) / scale, float(np.abs(got - ref64).max()) / scale
    if report is not None:
        report(what, e_ref=e_ref, e_hip=e_hip)
    print(f'{what}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}')
    assert e_hip <= 2 * max(e_ref, 2.0 ** -23), f'{what}: e_hip {e_hip:.3e} > 2 * max(e_ref {e_ref:.3e}, 2^-23)'


def _mat(rows, like):
    return torch.tensor(rows, dtype=like.dtype, device=like.device)


def _translate(tx, ty, like):
    return _mat([[1, 0, tx], [0, 1, ty], [0, 0, 1]], like)


def _scale(sx, sy, like):
    return _mat([[sx, 0, 0], [0, sy, 0], [0, 0, 1]], like)


def margins(G_inv, H, W):
    """[mx0, my0, mx1, my1] as python ints: the largest excursion of a frame corner over the whole batch, plus the filter's reach."""
    cx, cy = (W - 1) / 2, (H - 1) / 2
    cp = _mat([[-cx, -cy, 1], [cx, -cy, 1], [cx, cy, 1], [-cx, cy, 1]], G_inv)
    cp = G_inv @ cp.t()                                                      # [B, xyz, corner]
    m = cp[:, :2, :].permute(1, 0, 2).flatten(1)                            # [xy, B * corner]
    m = torch.cat([-m, m]).max(dim=1).values
    m = m + _mat([6 - cx, 6 - cy] * 2, G_inv)
    m = m.max(torch.zeros_like(m)).min(_mat([W - 1, H - 1] * 2, G_inv))
    return [int(v) for v in m.ceil().tolist()]


def geometry(images, G_inv, Hz_geom):
    up = importlib.import_module('3dgp_amd').ops.upfirdn2d
    B, C, H, W = images.shape
    G = G_inv.to(images.dtype)
    f = Hz_geom.to(device=images.device, dtype=torch.float32)
    mx0, my0, mx1, my1 = margins(G, H, W)
    x = torch.nn.functional.pad(images, [mx0, mx1, my0, my1], mode='reflect')
    G = _translate((mx0 - mx1) / 2, (my0 - my1) / 2, G) @ G
    x = up.upsample2d(x, f, up=2, impl='ref')
    G = _scale(2, 2, G) @ G @ _scale(1 / 2, 1 / 2, G)
    G = _translate(-0.5, -0.5, G) @ G @ _translate(0.5, 0.5, G)
    shape = [B, C, (H + 6) * 2, (W + 6) * 2]
    G = _scale(2 / x.shape[3], 2 / x.shape[2], G) @ G @ _scale(1 / (2 / shape[3]), 1 / (2 / shape[2]), G)
    grid = torch.nn.functional.affine_grid(theta=G[:, :2, :], size=shape, align_corners=False)
    x = torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    return up.downsample2d(x, f, down=2, padding=-6, flip_filter=True, impl='ref')


def color(images, Cm, ncc, bias=True):
    B, C, H, W = images.shape
    Cm = Cm.to(images.dtype)
    x = images.reshape(B, C, H * W)
    rest, x = x[:, ncc:], x[:, :ncc]
    if ncc == 3:
        x = Cm[:, :3, :3] @ x
        if bias:
            x = x + Cm[:, :3, 3:]
    elif ncc == 1:
        m = Cm[:, :3, :].mean(dim=1, keepdim=True)
        x = x * m[:, :, :3].sum(dim=2, keepdim=True)
        if bias:
            x = x + m[:, :, 3:]
    else:
        raise ValueError('Image must be RGB (3 channels) or L (1 channel)')
    return torch.cat([x, rest], dim=1).reshape(B, C, H, W)


def band_filter(images, gains, Hz_fbank):
    B, C, H, W = images.shape
    bank = Hz_fbank.to(device=images.device, dtype=images.dtype)
    taps = (gains.to(images.dtype) @ bank).unsqueeze(1).repeat([1, C, 1]).reshape([B * C, 1, -1])
    p = bank.shape[1] // 2
    x = torch.nn.functional.pad(images.reshape([1, B * C, H, W]), [p, p, p, p], mode='reflect')
    x = torch.nn.functional.conv2d(x, taps.unsqueeze(2), groups=B * C)
    x = torch.nn.functional.conv2d(x, taps.unsqueeze(3), groups=B * C)
    return x.reshape([B, C, H, W])


def cutout_mask(cutout, H, W, like):
    ct = cutout.to(like.dtype)
    xs = torch.arange(W, device=like.device).reshape(1, 1, 1, -1)
    ys = torch.arange(H, device=like.device).reshape(1, 1, -1, 1)
    mx = ((xs + 0.5) / W - ct[:, 2].reshape(-1, 1, 1, 1)).abs() >= ct[:, 0].reshape(-1, 1, 1, 1) / 2
    my = ((ys + 0.5) / H - ct[:, 3].reshape(-1, 1, 1, 1)).abs() >= ct[:, 1].reshape(-1, 1, 1, 1) / 2
    return torch.logical_or(mx, my).to(like.dtype)


def apply_reference(images, params, num_color_channels, Hz_geom, Hz_fbank=None, noise=None, color_bias=True):
    """`params`: anything with G_inv / C / gains / noise_sigma / cutout attributes (None = stage skipped), cast to the images' dtype.
    `noise`: the [B,C,H,W] normal draw to scale by noise_sigma (None: the noise stage adds nothing)."""
    x = images
    if params.G_inv is not None:
        x = geometry(x, params.G_inv.to(x.device), Hz_geom)
    if params.C is not None:
        x = color(x, params.C.to(x.device), num_color_channels, bias=color_bias)
    if params.gains is not None:
        x = band_filter(x, params.gains.to(x.device), Hz_fbank)
    if params.noise_sigma is not None and noise is not None:
        x = x + noise.to(x.dtype) * params.noise_sigma.to(device=x.device, dtype=x.dtype).reshape(-1, 1, 1, 1)
    if params.cutout is not None:
        x = x * cutout_mask(params.cutout.to(x.device), x.shape[2], x.shape[3], x)
    return x


class Params:
    def __init__(self, G_inv=None, C=None, gains=None, noise_sigma=None, cutout=None):
        self.G_inv, self.C, self.gains, self.noise_sigma, self.cutout = G_inv, C, gains, noise_sigma, cutout

    def to(self, device=None, dtype=None):
        return Params(*[None if t is None else t.to(device=device, dtype=dtype) for t in (self.G_inv, self.C, self.gains, self.noise_sigma, self.cutout)])


def _rot2(t):
    z, o = torch.zeros_like(t), torch.ones_like(t)
    return torch.stack([torch.cos(t), torch.sin(-t), z, torch.sin(t), torch.cos(t), z, z, z, o]).reshape(3, 3)


def percentile_params(kw, q, batch, H, W, num_channels, dtype):
    """The parameters the pipe takes under `debug_percentile=q`: every draw replaced by that quantile of its distribution.  As in the
    reference the quantile itself and the scalars derived from it are float32 whatever `dtype` is; the matrices are built in `dtype`."""
    a = dict(xflip=0, rotate90=0, xint=0, xint_max=0.125, scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2, xfrac_std=0.125,
             brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1, saturation_std=1,
             imgfilter=0, imgfilter_bands=[1, 1, 1, 1], imgfilter_std=1, noise=0, cutout=0, noise_std=0.1, cutout_size=0.5)
    a.update(kw)
    q = torch.as_tensor(q, dtype=torch.float32)
    e = torch.erfinv(q * 2 - 1)
    up = lambda t: t.to(dtype)                                             # noqa: E731
    like = torch.zeros([], dtype=dtype)
    out = Params()
    G = None
    eye3 = torch.eye(3, dtype=dtype)
    B3 = lambda M: M.expand(batch, 3, 3).contiguous()                       # noqa: E731  (batched factors, as the reference multiplies them)
    B4 = lambda M: M.expand(batch, 4, 4).contiguous()                       # noqa: E731
    if a['xflip'] > 0:
        i = up(torch.floor(q * 2))
        G = (eye3 if G is None else G) @ B3(_scale(float(1 / (1 - 2 * i)), 1 / 1, like))
    if a['rotate90'] > 0:
        i = up(torch.floor(q * 4))
        G = (eye3 if G is None else G) @ B3(_rot2(-(-np.pi / 2 * i)))
    if a['xint'] > 0:
        t = up((q * 2 - 1) * a['xint_max'])
        G = (eye3 if G is None else G) @ B3(_translate(-float(torch.round(t * W)), -float(torch.round(t * H)), like))
    if a['scale'] > 0:
        s = up(torch.exp2(e * a['scale_std']))
        G = (eye3 if G is None else G) @ B3(_scale(float(1 / s), float(1 / s), like))
    if a['rotate'] > 0:
        t = up((q * 2 - 1) * np.pi * a['rotate_max'])
        G = (eye3 if G is None else G) @ B3(_rot2(-(-t)))
    if a['aniso'] > 0:
        s = up(torch.exp2(e * a['aniso_std']))
        G = (eye3 if G is None else G) @ B3(_scale(float(1 / s), float(1 / (1 / s)), like))
    if a['xfrac'] > 0:
        t = up(e * a['xfrac_std'])
        G = (eye3 if G is None else G) @ B3(_translate(-float(t * W), -float(t * H), like))
    if G is not None:
        out.G_inv = G.contiguous()
    C = None
    eye4 = torch.eye(4, dtype=dtype)
    v = torch.as_tensor(np.asarray([1, 1, 1, 0]) / np.sqrt(3)).to(dtype)
    vv = v.ger(v)
    if a['brightness'] > 0:
        b = float(up(e * a['brightness_std']))
        T = eye4.clone()
        T[:3, 3] = b
        C = B4(T) @ (eye4 if C is None else C)
    if a['contrast'] > 0:
        c = float(up(torch.exp2(e * a['contrast_std'])))
        C = B4(torch.diag(torch.tensor([c, c, c, 1], dtype=dtype))) @ (eye4 if C is None else C)
    if a['lumaflip'] > 0:
        i = up(torch.floor(q * 2))
        C = B4((eye4 - 2 * vv * i)) @ (eye4 if C is None else C)
    if a['hue'] > 0 and num_channels > 1:
        t = up((q * 2 - 1) * np.pi * a['hue_max'])
        s, c = torch.sin(t), torch.cos(t)
        cc = 1 - c
        vx, vy, vz = v[0], v[1], v[2]
        z, o = torch.zeros_like(t), torch.ones_like(t)
        R = torch.stack([vx * vx * cc + c, vx * vy * cc - vz * s, vx * vz * cc + vy * s, z,
                         vy * vx * cc + vz * s, vy * vy * cc + c, vy * vz * cc - vx * s, z,
                         vz * vx * cc - vy * s, vz * vy * cc + vx * s, vz * vz * cc + c, z, z, z, z, o]).reshape(4, 4)
        C = B4(R) @ (eye4 if C is None else C)
    if a['saturation'] > 0 and num_channels > 1:
        s = up(torch.exp2(e * a['saturation_std']))
        C = B4((vv + (eye4 - vv) * s)) @ (eye4 if C is None else C)
    if C is not None:
        out.C = C.contiguous()
    if a['imgfilter'] > 0:
        power = torch.as_tensor(np.array([10, 1, 1, 1]) / 13).to(dtype)
        g = torch.ones(4, dtype=dtype)
        for i, strength in enumerate(a['imgfilter_bands']):
            t = torch.ones(4, dtype=dtype)
            t[i] = up(torch.exp2(e * a['imgfilter_std'])) if strength > 0 else 1.0
            g = g * (t / (power * t.square()).sum().sqrt())
        out.gains = g.expand(batch, 4).contiguous()
    if a['noise'] > 0:
        out.noise_sigma = up(torch.erfinv(q) * a['noise_std']).expand(batch).contiguous()
    if a['cutout'] > 0:
        out.cutout = torch.stack([like + a['cutout_size'], like + a['cutout_size'], up(q), up(q)]).expand(batch, 4).contiguous()
    return out

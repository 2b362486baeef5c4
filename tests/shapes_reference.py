"""The yardstick of the shape-frame tests: the contracts of tdgp_iso_bracket / tdgp_iso_locate / tdgp_iso_shade (include/tdgp.h) restated in
numpy float32, operation for operation -- every array below is float32 and numpy rounds each operation once, never fusing a multiply into
an add, and its float32 `/` and `sqrt` are correctly rounded -- plus the chain that strings them together around two field callbacks and an
analytic ray / sphere helper.  Written from the contract, for these tests."""
import numpy as np

F = np.float32
STATUS_MISS, STATUS_HIT, STATUS_NEAR = 0, 1, 2
MODES = {'shaded': 0, 'normals': 1, 'colour': 2}


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _first_at_least(sigma, level, none):
    """Per row: the first k with sigma[k] >= level (ordered comparison: a NaN is not), or `none`."""
    with np.errstate(invalid='ignore'):
        ge = sigma >= F(level)
    return np.where(ge.any(axis=1), ge.argmax(axis=1), none).astype(np.int32)


def bracket(sigma, t, N, level):
    """sigma, t [rays,S] -> (idx int32 [rays], t_fine [rays,N])."""
    sigma, t = _f(sigma), _f(t)
    rays, S = t.shape
    idx = _first_at_least(sigma, level, S)
    r = np.arange(rays)
    lo = t[r, np.clip(idx - 1, 0, S - 1)]                  # idx == 0: lo = hi = t[0]; idx == S: lo = hi = t[S-1]
    hi = t[r, np.clip(idx, 0, S - 1)]
    frac = np.arange(1, N + 1).astype(np.float32) / F(N)
    with np.errstate(invalid='ignore', over='ignore'):
        fine = lo[:, None] + (hi - lo)[:, None] * frac[None, :]
    inside = (idx >= 1) & (idx <= S - 1)
    fine = np.where(inside[:, None], fine, hi[:, None]).astype(np.float32)
    fine[:, N - 1] = hi
    return idx, fine


def locate(sigma, t, idx, sigma_fine, t_fine, ray_o, ray_d, level, h, t_miss):
    """-> (t_hit [rays], status int32 [rays], points [rays,7,3])."""
    sigma, t, sigma_fine, t_fine, ray_o, ray_d = (_f(a) for a in (sigma, t, sigma_fine, t_fine, ray_o, ray_d))
    rays, S = t.shape
    N = t_fine.shape[1]
    level, h = F(level), F(h)
    idx = np.clip(np.asarray(idx, np.int64), 0, S)
    r = np.arange(rays)
    j = _first_at_least(sigma_fine, level, N - 1).astype(np.int64)
    s_hi, t_hi = sigma_fine[r, j], t_fine[r, j]
    jm, im = np.maximum(j - 1, 0), np.clip(idx - 1, 0, S - 1)
    s_lo = np.where(j == 0, sigma[r, im], sigma_fine[r, jm])
    t_lo = np.where(j == 0, t[r, im], t_fine[r, jm])
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        a = (level - s_lo) / (s_hi - s_lo)
        a = np.where((a >= 0) & (a <= 1), a, F(1)).astype(np.float32)
        th = t_lo + (t_hi - t_lo) * a
    status = np.where(idx == S, STATUS_MISS, np.where(idx == 0, STATUS_NEAR, STATUS_HIT)).astype(np.int32)
    th = np.where(idx == S, F(t_miss), np.where(idx == 0, t[:, 0], th)).astype(np.float32)
    x = ray_o + ray_d * th[:, None]
    points = np.repeat(x[:, None, :], 7, axis=1)
    for i in range(3):
        points[:, 1 + 2 * i, i] = x[:, i] + h
        points[:, 2 + 2 * i, i] = x[:, i] - h
    return th, status, points


def shade(stencil, status, ray_d, mode, light=None, ambient=0.2, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0)):
    """stencil [rays,7,4] -> (rgb [rays,3], normal [rays,3])."""
    s, d = _f(stencil), _f(ray_d)
    status = np.asarray(status)
    ambient, albedo, background = F(ambient), _f(albedo), _f(background)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        g = np.stack([s[:, 1, 3] - s[:, 2, 3], s[:, 3, 3] - s[:, 4, 3], s[:, 5, 3] - s[:, 6, 3]], axis=1)
        q = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        toward = (-d) / dn[:, None]
        ok = (q > 0) & (q < np.inf)
        n = np.where(ok[:, None], (-g) / np.sqrt(q)[:, None], toward).astype(np.float32)
        l = toward if light is None else np.broadcast_to(_f(light), toward.shape)
        c = (n[:, 0] * l[:, 0] + n[:, 1] * l[:, 1]) + n[:, 2] * l[:, 2]
        c = np.where(c > 0, c, F(0)).astype(np.float32)
        v = ambient + (F(1) - ambient) * c
        if MODES[mode] == 0:
            out = (albedo[None, :] * v[:, None]) * F(2) - F(1)
        elif MODES[mode] == 1:
            out = n
        else:
            k = s[:, 0, :3] * F(0.5) + F(0.5)
            k = np.where(k > 0, k, F(0)).astype(np.float32)
            k = np.where(k > 1, F(1), k).astype(np.float32)
            out = (k * v[:, None]) * F(2) - F(1)
    miss = (status == STATUS_MISS)[:, None]
    rgb = np.where(miss, background[None, :], out).astype(np.float32)
    normal = np.where(miss, F(0), n).astype(np.float32)
    return rgb, normal


def chain(ray_field, point_field, t, ray_o, ray_d, N, level, h, t_miss, mode='shaded', **shade_kw):
    """The whole tail around two field callbacks: ray_field(t [rays,n]) -> rgbs [rays,n,4] at ray_o + t * ray_d, point_field(points
    [rays,7,3]) -> rgbs [rays,7,4].  -> dict(idx, t_fine, depth, status, points, rgb, normal)."""
    t = _f(t)
    sig_c = _f(ray_field(t))[..., 3]
    idx, t_fine = bracket(sig_c, t, N, level)
    sig_f = _f(ray_field(t_fine))[..., 3]
    depth, status, points = locate(sig_c, t, idx, sig_f, t_fine, ray_o, ray_d, level, h, t_miss)
    rgb, normal = shade(point_field(points), status, ray_d, mode, **shade_kw)
    return dict(idx=idx, t_fine=t_fine, depth=depth, status=status, points=points, rgb=rgb, normal=normal)


def ray_sphere(ray_o, ray_d, radius):
    """Float64: per ray (hit mask, entry depth t, chord length in t) of the sphere |x| = radius around the origin."""
    o, d = np.asarray(ray_o, np.float64), np.asarray(ray_d, np.float64)
    a, b, c = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - radius ** 2
    disc = b * b - a * c
    hit = disc > 0
    root = np.sqrt(np.where(hit, disc, 0.0))
    return hit, (-b - root) / a, 2.0 * root / a


def pinhole_rays(res, fov_deg, radius=1.0):
    """res x res rays of a camera at (0, 0, radius) looking at the origin: float32 origins and unit directions [res*res, 3]."""
    xs = np.linspace(-1.0, 1.0, res)
    x, y = np.meshgrid(xs, -xs)
    z = -np.ones_like(x) / np.tan(np.deg2rad(fov_deg) / 2.0)
    d = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.array([0.0, 0.0, radius]), d.shape)
    return _f(o), _f(d)

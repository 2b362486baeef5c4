"""The plain reference of the tri-plane field that the field tests share: torch CPU ops in any dtype (grid_sample, plane mean, the decoder's
layers), the bound the kernels are held to, and the inputs that take every branch of the bilinear addressing.  No GPU code is imported here.

The bound ("the reference's own noise"): with e_ref = max |reference fp32 - reference float64| and e_hip = max |kernel - reference float64|, both
divided by max(1, max |reference|), require e_hip <= 2 * max(e_ref, 2^-23) -- both computations make the same number of fp32 roundings in a
different order (README, parity paragraph)."""
import math

import numpy as np
import torch

from conftest import report_parity


def random_mlp_weights(rs, F, hid, n):
    """Weights [out, in] and biases of an n-layer decoder F -> hid x (n - 1) -> 4, drawn from `rs`: all weights first, then all biases."""
    dims = [F] + [hid] * (n - 1) + [4]
    ws = [rs.randn(o, i).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(0.3 * rs.randn(o)).astype(np.float32) for o in dims[1:]]
    return ws, bs


def _within_reference_noise(got, ref64, ref32, what):
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, f'{what}: shapes {got.shape} {ref64.shape} {ref32.shape}'
    scale = max(1.0, float(np.abs(ref64).max()))
    e_ref, e_hip = float(np.abs(ref32 - ref64).max()) / scale, float(np.abs(got - ref64).max()) / scale
    report_parity(what, e_ref=e_ref, e_hip=e_hip)
    print(f'{what}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}')
    assert e_hip <= 2 * max(e_ref, 2.0 ** -23), f'{what}: e_hip {e_hip:.3e} > 2 * max(e_ref {e_ref:.3e}, 2^-23)'


def _reference(planes, coords, ws, bs, marcher, scale, dtype, nearest_kink=None):
    """simple_tri_plane_renderer + TriPlaneMLP with torch CPU ops in `dtype`: grid_sample, plane mean, the layers.  -> [B,P,4] with the graph attached."""
    B, C, H, W = planes.shape
    F, P = C // 3, coords.shape[1]
    c = coords / scale
    c2d = torch.stack([c[..., [0, 1]], c[..., [0, 2]], c[..., [1, 2]]], dim=1).reshape(B * 3, 1, P, 2)
    feats = torch.nn.functional.grid_sample(planes.reshape(B * 3, F, H, W), c2d, mode='bilinear', align_corners=True).reshape(B, 3, F, P)
    h = feats.permute(0, 1, 3, 2).mean(dim=1).reshape(B * P, F)
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = torch.addmm(b.unsqueeze(0), h, (w * (1.0 / math.sqrt(w.shape[1]))).t())
        if i + 1 < len(ws):
            if nearest_kink is not None:                      # per point: the smallest |pre-activation| of any hidden unit so far
                nearest_kink.append(h.detach().abs().amin(dim=1).reshape(B, P))
            h = torch.nn.functional.leaky_relu(h, 0.2) * math.sqrt(2.0)
    out = h.reshape(B, P, 4)
    if marcher == 'mip':
        out = torch.cat([torch.sigmoid(out[..., :3]) * (1 + 2 * 0.001) - 0.001, out[..., 3:]], dim=-1)
    return out


def _cpu(arrays, dtype, grad=False):
    return [torch.as_tensor(np.ascontiguousarray(a)).to(dtype).requires_grad_(grad) for a in arrays]


def kink_mask(planes, coords, ws, bs, scale, threshold):
    """[B,P] bool: the points that have a hidden pre-activation within `threshold` of zero in the float64 run.  lrelu has a kink there: two correct
    fp32 evaluations may take different slopes (1 against 0.2) at such a point and then differ by its whole contribution to a gradient, so the
    gradient tests give these points a zero incoming gradient; every remaining point has the same slopes in any evaluation."""
    kink = []
    with torch.no_grad():
        _reference(*_cpu([planes, coords], torch.float64), _cpu(ws, torch.float64), _cpu(bs, torch.float64), 'classical', scale, torch.float64, nearest_kink=kink)
    return (torch.stack(kink).amin(dim=0) < threshold).numpy()


def _addressing_coords(scale):
    """[37, 3] positions that take every branch of the bilinear geometry the kernels share (csrc/field_body.inc, csrc/field_grad.inc), as
    normalised values q = c / scale per axis: the corners -1 and +1, 2^-20 inside and outside of each, beyond -2 texels and beyond W / H (the
    clamps).  Every such value stands on one axis at a time next to two interior ones -- so a cell's +1 neighbour is out of range on x only, on
    y only, on z only -- and then on all three axes at once.  All of them, and scale = 2^-1, are exact in fp32, so fp32 and float64 agree on the cell."""
    e = 2.0 ** -20
    special = [-1.0, 1.0, -1.0 + e, -1.0 - e, 1.0 - e, 1.0 + e, -2.5, 2.5]
    inner = [0.13, -0.41, 0.62]
    pts = []
    for axis in range(3):
        for v in special:
            p = [inner[(axis + 1) % 3], inner[(axis + 2) % 3], inner[axis]]
            p[axis] = v
            pts.append(p)
    pts += [[v, v, v] for v in special] + [[-1.0, 1.0, -2.5], [1.0 + e, -1.0 - e, 2.5], [2.5, -2.5, 1.0], inner, [-0.77, 0.05, 0.99]]
    q = np.asarray(pts, np.float32)
    assert q.shape == (37, 3)
    return q * np.float32(scale)


def _expected_cells(coords, scale, H, W):
    """[.., 3, 2] the (x0, y0) tap rows of the three planes in the kernels' own fp32 steps (divide, add, multiply, floor, clamp to [-2, size])."""
    q = coords.astype(np.float32) / np.float32(scale)
    out = np.empty(coords.shape[:-1] + (3, 2), np.int32)
    for pl, (u, v) in enumerate(((0, 1), (0, 2), (1, 2))):                         # planes (x,y), (x,z), (y,z): width <- first coordinate
        for k, (a, n) in enumerate(((u, W), (v, H))):
            i = (q[..., a] + np.float32(1.0)) * np.float32((n - 1) / 2.0)
            out[..., pl, k] = np.clip(np.floor(i), -2, n).astype(np.int32)
    return out

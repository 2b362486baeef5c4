"""tests/field_reference.py pinned without a GPU: the plain torch reference of the tri-plane field against an independent implementation (the C
oracle), forward and all six gradients, and the kink masks of tests/test_field_pairs_gpu.py held to the caps that file relies on."""
import numpy as np
import pytest
import torch

import test_field_pairs_gpu as cases
from conftest import report_parity
from field_reference import _cpu, _reference, kink_mask

B, H, W, P, SCALE = 2, 20, 28, 101, 0.5                               # planes not square: an H / W swap shows
PAIRS = [(24, 20), (8, 1), (32, 33), (16, 48), (32, 64), (64, 128)]
# The oracle returns fp32 and keeps the kernels' fp32 geometry chain (coords / scale, + 1, * (size - 1) / 2 in fp32), so the two agree to fp32 rounding
# of the geometry, not to double.  Measured with the seeds below, worst of the 12 cases, as a share of max(1, max |reference|): forward 2.30e-6
# ((64,128) mip), d_planes 1.23e-6, d_w0 2.08e-6, d_b0 8.6e-8, d_w1 1.68e-6, d_b1 1.2e-7, d_coords 1.41e-6.  The bound is twice the largest.
MEASURED_WORST = 2.30e-6
BOUND = 2 * MEASURED_WORST


@pytest.mark.parametrize('marcher', ['classical', 'mip'])
@pytest.mark.parametrize('F,hid', PAIRS)
def test_reference_agrees_with_the_oracle(oracle, F, hid, marcher):
    rs = np.random.RandomState(300 + 7 * F + hid + (50 if marcher == 'mip' else 0))
    planes = rs.randn(B, 3 * F, H, W).astype(np.float32)
    coords = rs.uniform(-0.64, 0.64, (B, P, 3)).astype(np.float32)   # the cube is [-0.5, 0.5]^3: a third of the points leave it
    assert 0.2 < (np.abs(coords).max(-1) > 0.5).mean() < 0.6
    w0, b0 = rs.randn(hid, F).astype(np.float32), (0.3 * rs.randn(hid)).astype(np.float32)
    w1, b1 = rs.randn(4, hid).astype(np.float32), (0.3 * rs.randn(4)).astype(np.float32)
    d_out = rs.randn(B, P, 4).astype(np.float32)
    x, c = _cpu([planes, coords], torch.float64, grad=True)
    ws, bs = _cpu([w0, w1], torch.float64, grad=True), _cpu([b0, b1], torch.float64, grad=True)
    out = _reference(x, c, ws, bs, marcher, SCALE, torch.float64)
    grads = torch.autograd.grad(out, [x, ws[0], bs[0], ws[1], bs[1], c], torch.as_tensor(d_out).to(torch.float64))
    ref = dict(zip(('d_planes', 'd_w0', 'd_b0', 'd_w1', 'd_b1', 'd_coords'), [g.numpy() for g in grads]), out=out.detach().numpy())
    fwd = oracle.triplane_field(planes, coords, w0, b0, w1, b1, SCALE, mlp_mode=marcher)
    got = dict(zip(('d_planes', 'd_w0', 'd_b0', 'd_w1', 'd_b1', 'd_coords'),
                   oracle.triplane_field_grad(planes, coords, w0, b0, w1, b1, d_out[..., :3], d_out[..., 3:], scale=SCALE, mlp_mode=marcher, return_coords=True)),
               out=np.concatenate([fwd['rgb'], fwd['sigma']], axis=-1))
    errs = {}
    for name, r in ref.items():
        assert got[name].shape == r.shape, name
        errs[name] = float(np.abs(got[name].astype(np.float64) - r).max()) / max(1.0, float(np.abs(r).max()))
    print(f'reference vs oracle F {F} hid {hid} {marcher}: ' + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    report_parity(f'field reference vs oracle F {F} hid {hid} {marcher}', **errs)
    for name, e in errs.items():
        assert e <= BOUND, f'{name}: {e:.3e} of max(1, max |reference|) from the oracle (> {BOUND:.1e})'


@pytest.mark.parametrize('F,hid,n,marcher', cases.SMALL_GRAD_CASES)
def test_kink_mask_caps_of_the_small_gradient_cases(F, hid, n, marcher):
    """Conditions of the gradient tests, not measurements: at most 3 % of a case's points get a zero incoming gradient, and of the five points of
    the ragged last tile at least one is kept.  (Measured over these cases: at most 2 of the 202 points masked.)"""
    planes, coords, ws, bs, _ = cases.small_case(F, hid, n, marcher)
    assert coords.shape == (2, 101, 3) and len(ws) == n and ws[0].shape == (hid, F)
    mask = kink_mask(planes, coords, ws, bs, cases.SCALE, cases.KINK)
    assert mask.shape == (2, 101) and mask.dtype == bool
    print(f'kink mask F {F} hid {hid} n {n} {marcher}: {mask.mean():.4f} of the points')
    assert mask.mean() <= 0.03 and not mask[-1, -5:].all()


@pytest.mark.parametrize('F,hid', cases.MANY_BLOCK_CASES)
def test_kink_mask_caps_of_the_many_block_cases(F, hid):
    planes, coords, ws, bs, _ = cases.many_block_case(hid)
    assert coords.shape == (2, 33333, 3) and ws[0].shape == (hid, F)
    mask = kink_mask(planes, coords, ws, bs, cases.SCALE, cases.KINK_MANY)
    print(f'kink mask 2 x 33333 points F {F} hid {hid}: {mask.mean():.4f} of the points')
    assert 0 < mask.mean() < 0.03 and not mask[-1, -10:].all()


def test_kink_mask_is_the_nearest_hidden_pre_activation():
    """`kink_mask` against its definition written out: a two-layer decoder whose first bias puts one chosen hidden unit of one chosen point at zero."""
    rs = np.random.RandomState(11)
    F, hid = 8, 5
    planes, coords = rs.randn(1, 3 * F, 6, 7), rs.uniform(-0.4, 0.4, (1, 9, 3))
    w0, b0, w1, b1 = rs.randn(hid, F), rs.randn(hid) + 3.0, rs.randn(4, hid), rs.randn(4)
    pre = []
    with torch.no_grad():
        _reference(*_cpu([planes, coords], torch.float64), _cpu([w0, w1], torch.float64), _cpu([b0, b1], torch.float64), 'classical', 0.5, torch.float64, nearest_kink=pre)
    assert not kink_mask(planes, coords, [w0, w1], [b0, b1], 0.5, float(pre[0].min()) * 0.5).any()
    feats = torch.nn.functional.grid_sample(
        torch.as_tensor(planes).reshape(3, F, 6, 7),
        torch.stack([torch.as_tensor(coords / 0.5)[..., [a, b]] for a, b in ((0, 1), (0, 2), (1, 2))], dim=1).reshape(3, 1, 9, 2),
        mode='bilinear', align_corners=True).reshape(3, F, 9).mean(dim=0).numpy()
    b0[2] = -float(w0[2] @ feats[:, 4]) / np.sqrt(F)                   # unit 2 of point 4 now sits at zero
    mask = kink_mask(planes, coords, [w0, w1], [b0, b1], 0.5, 1e-9)
    assert mask.shape == (1, 9) and mask[0, 4] and mask.sum() == 1

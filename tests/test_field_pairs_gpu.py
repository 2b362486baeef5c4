"""Every width and walk form of the tri-plane field kernels against the plain float64 reference (tests/field_reference.py).

Forward, two layers (csrc/field.hip): the 12 (feat_dim, hid_dim) pairs of FIELD_CASE in points mode and in the three ray forms.  The profile
report names all three forward kernels `triplane_field_kernel`; which case reaches which one follows from launch_field_t's conditions:
  * F = 8 (FQ = 2): `triplane_field_kernel` always, image mode included;
  * F = 16 / 32, image walk, S = 20 (S % 4 == 0, S >= 16): `triplane_walk2_kernel` -- but for hid 16, (32,16) and (16,16), which launch_field_t
    keeps on the table walk (their walk2 instantiations would read a scalar offset too soon after the vector instruction that writes it, a memory
    fault; 3dgp_amd/isa_check.py looks for that in every build);
  * F = 16 / 32, image walk, S = 18 (S % 4 != 0) and S = 12 (S < 16), and F = 64 at every S: `triplane_walk_kernel`, with its operands in
    registers for MT * FQ <= 32 (every F = 16 pair, (32,16), (32,32), (32,64)) and in LDS for (32,128), (64,64), (64,128);
  * linear ray order and points mode: `triplane_field_kernel`.
Forward, 4 layers (csrc/field_deep.hip, NH = 2): the 10 deep pairs.
Gradient, two layers (csrc/render_grad.hip): F in {8,16,24,32} x hid <= 64 as include/tdgp.h states them -- the MT = 1 block of 4 waves
(hid <= 32) and the MT = 2 block of 2 waves, full and zero-padded panels -- and the same for the four deep-gradient instantiations
(MT 1 / 2 x NH 1 / 2).  Widths outside the Python wrapper's table go through the C entry points directly.

Every comparison is held to `_within_reference_noise`; gradient cases give a zero incoming gradient to the points at an lrelu kink
(`kink_mask`; tests/test_field_reference.py asserts, without a GPU, that this masks at most 3 % of any case and never the whole ragged tail).

Measured on an MI355X, worst e_hip / max(e_ref, 2^-23) per group (the bound is 2): a. 1.10 ((64,128) mip), b. 1.07 ((16,16) S 12), c. 1.10 ((8,16)),
d. 2.00 ((32,48) d_b1 through the C entry point: e_hip 2.38e-7 where e_ref 9.7e-8 lies under the 2^-23 floor; deterministic, fixed reduction order),
e. 1.48 ((8,32) n 4 d_b2), f. 1.14 ((32,32) d_w0).  f. with field_grad_reduce_kernel summing in fp32, as it did: 2.99 ((32,32) d_b1, 4.18e-7
against 1.40e-7), a failure; the kernel now sums in fp64.
That the tests bite, checked with two value-only changes to a copy of the sources: field_grad_reduce_kernel summing nblocks - 1 blocks fails both
cases of f. (d_w0 off by 4.7e-2 and 3.7e-2); `/ 3.0001f` for `/ 3.0f` in field_body's a0s fill for MT = 2 alone fails a. for (32,32), (16,32),
(8,32) and (8,32) mip, the four hid 32 cases, and for nothing else."""
import ctypes

import numpy as np
import pytest
import torch

from field_reference import _cpu, _expected_cells, _reference, _within_reference_noise, kink_mask, random_mlp_weights

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B, H, W, P, SCALE = 2, 20, 28, 32 * 3 + 5, 0.5                        # planes not square (an H / W swap shows); P no multiple of 16 or 32
KINK, KINK_MANY = 1e-5, 1e-4                                          # fp32 evaluations of these O(1) sums differ by ~1e-6

FWD2_PAIRS = [(32, 64), (32, 32), (32, 128), (32, 16), (16, 64), (16, 32), (16, 16), (8, 64), (8, 32), (8, 16), (64, 64), (64, 128)]      # FIELD_CASE
DEEP_PAIRS = [(32, 64), (32, 32), (32, 16), (16, 64), (16, 32), (16, 16), (8, 64), (8, 32), (8, 16), (64, 64)]
FWD2_POINT_CASES = [(F, hid, 'classical') for F, hid in FWD2_PAIRS] + [(8, 32, 'mip'), (64, 128, 'mip')]
RAY_S = [20, 18, 12]

# gradient cases (F, hid, n_layers, marcher)
GRAD2_WRAPPER_CASES = [(F, hid, 2, 'classical') for F in (8, 16, 32) for hid in (16, 32, 64)]
GRAD2_ABI_CASES = [(F, hid, 2, 'classical') for F, hid in ((24, 16), (24, 64), (8, 1), (16, 20), (32, 33), (32, 48), (24, 40))] + \
                  [(24, 40, 2, 'mip'), (32, 33, 2, 'mip')]
DEEP_WRAPPER_CASES = [(F, hid, n, 'classical') for F, hid in DEEP_PAIRS if F <= 32 for n in (3, 4)]
DEEP_ABI_CASES = [(24, 32, 3, 'classical'), (16, 20, 4, 'classical'), (32, 33, 3, 'classical'), (32, 48, 4, 'classical')]
SMALL_GRAD_CASES = GRAD2_WRAPPER_CASES + GRAD2_ABI_CASES + DEEP_WRAPPER_CASES + DEEP_ABI_CASES
MANY_BLOCK_CASES = [(32, 64), (32, 32)]                               # the MT = 2 form; the MT = 1 form with 4 waves


def small_case(F, hid, n, marcher):
    """The common small shape of this file, drawn from the case's own seed: planes [B,3F,H,W], coords [B,P,3] uniform in +-0.64 (the cube is
    [-0.5, 0.5]^3: a third of the points leave it), n layers of weights and biases, an incoming gradient [B,P,4].  No GPU."""
    rs = np.random.RandomState(1000 + 7 * F + hid + 1000 * n + (500 if marcher == 'mip' else 0))
    planes = rs.randn(B, 3 * F, H, W).astype(np.float32)
    coords = rs.uniform(-0.64, 0.64, (B, P, 3)).astype(np.float32)
    ws, bs = random_mlp_weights(rs, F, hid, n)
    d_out = rs.randn(B, P, 4).astype(np.float32)
    return planes, coords, ws, bs, d_out


def many_block_case(hid):
    """The shape of test_field_grad_large -- 2 x 33333 points on 32 x 32 planes, 521 blocks -- built like test_gradient_many_tiles_vs_float64."""
    rs = np.random.RandomState(77 + hid)
    Bm, F, Hm, Pm = 2, 32, 32, 33333
    planes = rs.randn(Bm, 3 * F, Hm, Hm).astype(np.float32)
    coords = rs.uniform(-0.6, 0.6, (Bm, Pm, 3)).astype(np.float32)
    d_out = rs.randn(Bm, Pm, 4).astype(np.float32)
    ws, bs = random_mlp_weights(rs, F, hid, 2)
    return planes, coords, ws, bs, d_out


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()


def _module(tdgp, ws, bs, marcher):
    m = tdgp.renderer.TriPlaneMLP(ws[0].shape[1], ws[0].shape[0], 3, marcher, n_layers=len(ws)).to(DEV)
    with torch.no_grad():
        for fc, w, b in zip(m.model, ws, bs):
            fc.weight.copy_(T(w)); fc.bias.copy_(T(b))
    return m


def _forward_references(planes, coords, ws, bs, marcher):
    with torch.no_grad():
        return [_reference(*_cpu([planes, coords], dt), _cpu(ws, dt), _cpu(bs, dt), marcher, SCALE, dt).numpy() for dt in (torch.float64, torch.float32)]


def _grad_names(n):
    return ['d_planes', 'd_coords'] + [f'd_w{i}' for i in range(n)] + [f'd_b{i}' for i in range(n)]


def _grad_references(planes, coords, ws, bs, d_out, marcher):
    """{float64, float32} -> {name: gradient} by autograd through `_reference`."""
    refs = {}
    for dtype in (torch.float64, torch.float32):
        x, c = _cpu([planes, coords], dtype, grad=True)
        w_, b_ = _cpu(ws, dtype, grad=True), _cpu(bs, dtype, grad=True)
        out = _reference(x, c, w_, b_, marcher, SCALE, dtype)
        grads = torch.autograd.grad(out, [x, c] + w_ + b_, torch.as_tensor(d_out).to(dtype))
        refs[dtype] = dict(zip(_grad_names(len(ws)), [t.numpy() for t in grads]))
    return refs


def _masked_small_case(F, hid, n, marcher):
    planes, coords, ws, bs, d_out = small_case(F, hid, n, marcher)
    d_out[kink_mask(planes, coords, ws, bs, SCALE, KINK)] = 0.0
    return planes, coords, ws, bs, d_out


def _hold_gradients(got, refs, what):
    assert sorted(got) == sorted(refs[torch.float64])
    for name in refs[torch.float64]:
        _within_reference_noise(N(got[name]), refs[torch.float64][name], refs[torch.float32][name], f'{what} {name}')


# ------------------------------------------------------------------------------------------------ a. two-layer forward, points mode
@pytest.mark.parametrize('F,hid,marcher', FWD2_POINT_CASES)
def test_two_layer_forward_points_every_pair(tdgp, F, hid, marcher):
    R = tdgp.renderer
    planes, coords, ws, bs, _ = small_case(F, hid, 2, marcher)
    mlp = _module(tdgp, ws, bs, marcher)
    assert R.fused_form(mlp)
    hw, pack = R.planes_to_hwc(T(planes)), R._mlp_params(mlp)
    plain = R._field(hw, pack, SCALE, coords=T(coords))
    taps = torch.full([B, P, 3, 2], -7, dtype=torch.int32, device=DEV)
    tapped = R._field(hw, pack, SCALE, coords=T(coords), tap_idx=taps)
    assert torch.equal(plain, tapped)                                              # the instantiations with and without tap rows
    assert np.array_equal(N(taps), _expected_cells(coords, SCALE, H, W))
    ref64, ref32 = _forward_references(planes, coords, ws, bs, marcher)
    _within_reference_noise(N(plain), ref64, ref32, f'field pairs a. forward points F {F} hid {hid} {marcher}')


# ------------------------------------------------------------------------------------------------ b. two-layer forward, ray forms
@pytest.mark.parametrize('S', RAY_S)
@pytest.mark.parametrize('F,hid', FWD2_PAIRS)
def test_two_layer_forward_ray_forms_every_pair(tdgp, F, hid, S):
    R = tdgp.renderer
    h, w, marcher = 9, 17, 'classical'                                             # not whole 8 x 8 patches
    rs = np.random.RandomState(2000 + 7 * F + hid + 100 * S)
    planes = rs.randn(B, 3 * F, H, W).astype(np.float32)
    ws, bs = random_mlp_weights(rs, F, hid, 2)
    cam = dict(angles=T(np.stack([rs.uniform(-1, 1, B), rs.uniform(1.0, 2.0, B), np.zeros(B)], 1)), radius=T(np.ones(B)), look_at=T(np.zeros((B, 3))))
    ray_o, ray_d = R.sample_rays(R.compute_cam2world_matrix(cam), T(rs.uniform(15, 45, B)), (w, h))
    Rn = h * w
    assert ray_o.shape == (B, Rn, 3)
    t = T(np.sort(rs.uniform(0.4, 1.6, (B, Rn, S)).astype(np.float32), axis=2))     # beyond the cube at both ends
    noise = T(rs.randn(B, Rn * S).astype(np.float32))
    coords = (ray_o.unsqueeze(-2) + t.unsqueeze(-1) * ray_d.unsqueeze(-2)).reshape(B, Rn * S, 3)      # torch, fp32: multiply, then add
    outside = (coords.abs().amax(-1) > 0.5).reshape(B, Rn, S)                       # the cube is [-0.5, 0.5]^3
    assert outside[..., 0].any() and outside[..., -1].any() and not outside.all(dim=-1).all()
    mlp = _module(tdgp, ws, bs, marcher)
    hw, pack = R.planes_to_hwc(T(planes)), R._mlp_params(mlp)
    modes = (dict(ray_o=ray_o, ray_d=ray_d, t=t, ray_w=w), dict(ray_o=ray_o, ray_d=ray_d, t=t, ray_w=0), dict(coords=coords))
    outs, taps = [], []
    for mode in modes:
        tp = torch.full([B, Rn * S, 3, 2], -7, dtype=torch.int32, device=DEV)
        outs.append(R._field(hw, pack, SCALE, **mode))
        assert torch.equal(R._field(hw, pack, SCALE, tap_idx=tp, **mode), outs[-1])
        assert int((tp == -7).sum()) == 0
        taps.append(tp)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])           # image walk, linear ray order, coords mode: identical bytes
    assert torch.equal(taps[0], taps[1]) and torch.equal(taps[0], taps[2])
    assert np.array_equal(N(taps[2]), _expected_cells(N(coords), SCALE, H, W))
    ref64, ref32 = _forward_references(planes, N(coords), ws, bs, marcher)
    _within_reference_noise(N(outs[0]), ref64, ref32, f'field pairs b. forward image walk F {F} hid {hid} S {S}')
    if S == RAY_S[0]:                                                              # once per pair: the density noise of every form
        for mode in modes:
            noisy = R._field(hw, pack, SCALE, sigma_noise=noise, density_noise=0.8, **mode)
            assert torch.equal(noisy[..., :3], outs[0][..., :3])
            assert torch.equal(noisy[..., 3], outs[0][..., 3] + noise * 0.8)


# ------------------------------------------------------------------------------------------------ c. deep forward at n = 4
@pytest.mark.parametrize('F,hid', DEEP_PAIRS)
def test_four_layer_forward_points_every_pair(tdgp, F, hid):
    R = tdgp.renderer
    planes, coords, ws, bs, _ = small_case(F, hid, 4, 'classical')
    mlp = _module(tdgp, ws, bs, 'classical')
    assert R.deep_form(mlp)
    got = R._field(R.planes_to_hwc(T(planes)), R._mlp_params_deep(mlp), SCALE, coords=T(coords))
    ref64, ref32 = _forward_references(planes, coords, ws, bs, 'classical')
    _within_reference_noise(N(got), ref64, ref32, f'field pairs c. deep forward n 4 F {F} hid {hid}')


# ------------------------------------------------------------------------------------------------ d. two-layer gradient
def _nan_like(t):
    return torch.full_like(t, float('nan'))                                        # an element the kernel leaves unwritten shows


def _field_grad_abi(tdgp, planes, coords, ws, bs, d_out, marcher):
    """tdgp_triplane_field_grad / tdgp_triplane_field_deep_grad through the C ABI, allocating as `simple_tri_plane_renderer_backward` does (zeroed
    d_planes, workspace from the entry point's own query): the wrapper refuses widths outside the forward table by design."""
    R, L = tdgp.renderer, tdgp._lib
    p = R.planes_to_hwc(T(planes)).t
    Bq, _, Hq, Wq, F = p.shape
    c, do = T(coords), T(d_out)
    Pq, hid, n = c.shape[1], ws[0].shape[0], len(ws)
    w, b = [T(a) for a in ws], [T(a) for a in bs]
    d_planes, d_coords = torch.zeros_like(p), _nan_like(c)
    d_w, d_b = [_nan_like(t) for t in w], [_nan_like(t) for t in b]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])    # noqa: E731  (as renderer._ptr_array)
    with torch.cuda.device(p.device):
        if n == 2:
            nbytes = int(L.load().tdgp_triplane_field_grad_workspace_bytes(Bq, Pq, F, hid))
            assert nbytes > 0
            buf = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
            L.call('tdgp_triplane_field_grad', p.data_ptr(), c.data_ptr(), w[0].data_ptr(), b[0].data_ptr(), w[1].data_ptr(), b[1].data_ptr(), do.data_ptr(),
                   d_planes.data_ptr(), d_w[0].data_ptr(), d_b[0].data_ptr(), d_w[1].data_ptr(), d_b[1].data_ptr(), d_coords.data_ptr(), buf.data_ptr(), nbytes,
                   Bq, Pq, F, Hq, Wq, hid, SCALE, R.MARCHER_IDS[marcher], L.stream_of(p))
        else:
            nbytes = int(L.load().tdgp_triplane_field_deep_grad_workspace_bytes(Bq, Pq, F, hid, n))
            assert nbytes > 0
            buf = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
            L.call('tdgp_triplane_field_deep_grad', p.data_ptr(), c.data_ptr(), ptrs(w), ptrs(b), n, do.data_ptr(), d_planes.data_ptr(), ptrs(d_w), ptrs(d_b),
                   d_coords.data_ptr(), buf.data_ptr(), nbytes, Bq, Pq, F, Hq, Wq, hid, SCALE, R.MARCHER_IDS[marcher], L.stream_of(p))
        torch.cuda.synchronize()
    got = dict(d_planes=R.planes_from_hwc(d_planes), d_coords=d_coords)
    for i in range(n):
        got[f'd_w{i}'], got[f'd_b{i}'] = d_w[i], d_b[i]
    return got


def _field_grad_wrapper(tdgp, planes, coords, ws, bs, d_out, marcher):
    R = tdgp.renderer
    n = len(ws)
    mlp = _module(tdgp, ws, bs, marcher)
    assert R.fused_form(mlp) if n == 2 else R.deep_form(mlp)
    res = R.simple_tri_plane_renderer_backward(T(planes), T(coords), mlp, T(d_out[..., :3]), T(d_out[..., 3:]), scale=SCALE, coords_grad=True)
    if n == 2:
        return dict(d_planes=R.planes_from_hwc(res[0]), d_w0=res[1], d_b0=res[2], d_w1=res[3], d_b1=res[4], d_coords=res[5])
    got = dict(d_planes=R.planes_from_hwc(res[0]), d_coords=res[3])
    for i in range(n):
        got[f'd_w{i}'], got[f'd_b{i}'] = res[1][i], res[2][i]
    return got


def _gradient_case(tdgp, call, F, hid, n, marcher, what):
    planes, coords, ws, bs, d_out = _masked_small_case(F, hid, n, marcher)
    got = call(tdgp, planes, coords, ws, bs, d_out, marcher)
    _hold_gradients(got, _grad_references(planes, coords, ws, bs, d_out, marcher), f'{what} F {F} hid {hid} n {n} {marcher}')
    if n == 2 and hid in (32, 33):                                                 # the fixed reduction order of both block shapes: identical bytes run to run
        again = call(tdgp, planes, coords, ws, bs, d_out, marcher)
        for name in ('d_w0', 'd_b0', 'd_w1', 'd_b1'):
            assert torch.equal(got[name], again[name]), name


@pytest.mark.parametrize('F,hid,n,marcher', GRAD2_WRAPPER_CASES)
def test_two_layer_gradient_table_pairs(tdgp, F, hid, n, marcher):
    _gradient_case(tdgp, _field_grad_wrapper, F, hid, n, marcher, 'field pairs d. grad')


@pytest.mark.parametrize('F,hid,n,marcher', GRAD2_ABI_CASES)
def test_two_layer_gradient_widths_of_the_header(tdgp, F, hid, n, marcher):
    _gradient_case(tdgp, _field_grad_abi, F, hid, n, marcher, 'field pairs d. grad (C ABI)')


# ------------------------------------------------------------------------------------------------ e. deep gradient
@pytest.mark.parametrize('F,hid,n,marcher', DEEP_WRAPPER_CASES)
def test_deep_gradient_table_pairs(tdgp, F, hid, n, marcher):
    _gradient_case(tdgp, _field_grad_wrapper, F, hid, n, marcher, 'field pairs e. deep grad')


@pytest.mark.parametrize('F,hid,n,marcher', DEEP_ABI_CASES)
def test_deep_gradient_widths_of_the_header(tdgp, F, hid, n, marcher):
    _gradient_case(tdgp, _field_grad_abi, F, hid, n, marcher, 'field pairs e. deep grad (C ABI)')


# ------------------------------------------------------------------------------------------------ f. two-layer gradient at many blocks
@pytest.mark.parametrize('F,hid', MANY_BLOCK_CASES)
def test_two_layer_gradient_many_blocks_vs_float64(tdgp, F, hid):
    """521 blocks of partial sums per weight / bias gradient element, held to the bound the deep kernel is held to at this shape."""
    planes, coords, ws, bs, d_out = many_block_case(hid)
    ambiguous = kink_mask(planes, coords, ws, bs, SCALE, KINK_MANY)
    assert 0 < ambiguous.mean() < 0.03 and not ambiguous[-1, -10:].all()           # the ten points of the ragged last tile are (mostly) kept
    d_out[ambiguous] = 0.0
    got = _field_grad_wrapper(tdgp, planes, coords, ws, bs, d_out, 'classical')
    _hold_gradients(got, _grad_references(planes, coords, ws, bs, d_out, 'classical'), f'field pairs f. grad 2 x 33333 points F {F} hid {hid}')


# ------------------------------------------------------------------------------------------------ g. forward-only widths say so up front
@pytest.mark.parametrize('F,hid', [(32, 128), (64, 64), (64, 128)])
def test_wide_two_layer_decoder_is_forward_only_and_says_so_up_front(tdgp, F, hid):
    """In the forward table, not in the gradient kernel's (F <= 32, hid <= 64): `render_autograd` refuses before anything is launched."""
    R = tdgp.renderer
    mlp = R.TriPlaneMLP(F, hid, 3, 'classical').to(DEV)
    assert R.fused_form(mlp)
    opts = dict(box_size=1.0, num_proposal_steps=8, num_fine_steps=8, clamp_mode='softplus', use_inf_depth=True, ray_start=0.75, ray_end=1.25)
    planes = torch.randn([1, 3 * F, 16, 16], device=DEV, requires_grad=True)
    rays = torch.zeros([1, 16, 3], device=DEV)
    tdgp._lib.profile_enable(True)
    try:
        with pytest.raises(NotImplementedError, match='forward-only'):
            R.render_autograd(R.ImportanceRenderer('classical'), planes, mlp, rays, rays, opts)
        torch.cuda.synchronize()
        assert not tdgp._lib.profile_report()                                      # refused before any launch
    finally:
        tdgp._lib.profile_enable(False)

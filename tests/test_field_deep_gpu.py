"""tdgp_triplane_field_deep / tdgp_triplane_field_deep_grad (csrc/field_deep.hip): the field of 3- and 4-layer tri-plane decoders, forward and
gradient, on the GPU.

The bound used throughout ("the reference's own noise"): with e_ref = max |reference fp32 - reference float64| and e_hip = max |kernel - reference
float64|, both divided by max(1, max |reference|), require e_hip <= 2 * max(e_ref, 2^-23) -- both computations make the same number of fp32
roundings in a different order (README, parity paragraph)."""
import numpy as np
import pytest
import torch

from conftest import assert_close, load_golden, report_parity
from field_reference import _addressing_coords, _cpu, _expected_cells, _reference, _within_reference_noise, random_mlp_weights

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAIRS = [(32, 64), (32, 32), (32, 16), (16, 64), (16, 32), (16, 16), (8, 64), (8, 32), (8, 16), (64, 64)]      # the fused table's pairs with hid <= 64


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()


def _deep_mlp(tdgp, ws, bs, marcher):
    m = tdgp.renderer.TriPlaneMLP(ws[0].shape[1], ws[0].shape[0], 3, marcher, n_layers=len(ws)).to(DEV)
    with torch.no_grad():
        for fc, w, b in zip(m.model, ws, bs):
            fc.weight.copy_(T(w)); fc.bias.copy_(T(b))
    return m


def _random_mlp(tdgp, rs, F, hid, n, marcher):
    ws, bs = random_mlp_weights(rs, F, hid, n)
    return _deep_mlp(tdgp, ws, bs, marcher), ws, bs


# ------------------------------------------------------------------------------------------------ 1. reference goldens through the kernel
@pytest.mark.parametrize('tag,n,marcher', [('n3', 3, 'classical'), ('n4mip', 4, 'mip')])
def test_mlp_variants_go_through_the_kernel(tdgp, tag, n, marcher):
    g = load_golden('mlp_variants')
    R = tdgp.renderer
    mlp = _deep_mlp(tdgp, [g[f'{tag}_w{i}'] for i in range(n)], [g[f'{tag}_b{i}'] for i in range(n)], marcher)
    assert R.deep_form(mlp)
    planes, coords = T(g[f'{tag}_planes']), T(g['coords'])
    out = R.simple_tri_plane_renderer(planes, coords, mlp, scale=0.5)
    direct = R._field(R.planes_to_hwc(planes), R._mlp_params_deep(mlp), 0.5, coords=coords)
    assert torch.equal(torch.cat([out['rgb'], out['sigma']], dim=-1), direct)
    for key in ('rgb', 'sigma'):
        ref = g[f'{tag}_{key}']
        assert_close(N(out[key]), ref, 5e-6, f'{tag} {key} (deep kernel)', max(1.0, float(np.abs(ref).max())))


def _fixture_case(tdgp, g, tag, marcher):
    n = 3 if tag == 'small_n3' else 4
    mlp = _deep_mlp(tdgp, [g[f'{tag}_w{i}'] for i in range(n)], [g[f'{tag}_b{i}'] for i in range(n)], marcher)
    k = f'{tag}_{marcher}_'
    ref32 = lambda name: g[k + name]                                                          # noqa: E731
    ref64 = lambda name: g[k + name].astype(np.float64) + g[k + name + '_f64m32'].astype(np.float64)      # noqa: E731  (tools/gen_goldens.py: gen_field_deep)
    return mlp, n, ref32, ref64


@pytest.mark.parametrize('tag', ['small_n3', 'hot_n4'])
@pytest.mark.parametrize('marcher', ['classical', 'mip'])
def test_forward_vs_reference_fixture(tdgp, tag, marcher):
    g = load_golden('field_deep')
    R = tdgp.renderer
    mlp, n, ref32, ref64 = _fixture_case(tdgp, g, tag, marcher)
    assert R.deep_form(mlp)
    planes, coords = T(g[f'{tag}_planes']), T(g[f'{tag}_coords'])
    out = R.simple_tri_plane_renderer(planes, coords, mlp, scale=0.5)
    direct = R._field(R.planes_to_hwc(planes), R._mlp_params_deep(mlp), 0.5, coords=coords)
    assert torch.equal(torch.cat([out['rgb'], out['sigma']], dim=-1), direct)
    for key in ('rgb', 'sigma'):
        _within_reference_noise(N(out[key]), ref64(key), ref32(key), f'field_deep forward {tag} {marcher} {key}')


# ------------------------------------------------------------------------------------------------ 2. every accepted (F, hid) pair
@pytest.mark.parametrize('F,hid', PAIRS)
def test_every_pair_vs_float64(tdgp, F, hid):
    rs = np.random.RandomState(1000 + F * 7 + hid)
    R = tdgp.renderer
    B, H, P = 2, 24, 16 * 3 + 5
    planes = rs.randn(B, 3 * F, H, H).astype(np.float32)
    coords = rs.uniform(-0.64, 0.64, (B, P, 3)).astype(np.float32)
    mlp, ws, bs = _random_mlp(tdgp, rs, F, hid, 3, 'classical')
    assert R.deep_form(mlp)
    with torch.no_grad():
        ref64 = _reference(*_cpu([planes, coords], torch.float64), _cpu(ws, torch.float64), _cpu(bs, torch.float64), 'classical', 0.5, torch.float64).numpy()
    hw = R.planes_to_hwc(T(planes))
    got = R._field(hw, R._mlp_params_deep(mlp), 0.5, coords=T(coords))
    eager = R._field_eager(hw, mlp, 0.5, coords=T(coords))
    _within_reference_noise(N(got), ref64, N(eager), f'field_deep forward F {F} hid {hid}')


# ------------------------------------------------------------------------------------------------ 3. walk independence, integer rows
@pytest.mark.parametrize('n,marcher', [(3, 'classical'), (4, 'mip')])
@pytest.mark.parametrize('B,h,w,S', [(2, 9, 17, 20), (1, 16, 24, 16)])
def test_walks_give_identical_bytes(tdgp, B, h, w, S, n, marcher):
    rs = np.random.RandomState(31 * h + n)
    R = tdgp.renderer
    F, hid, H = 32, 64, 24
    mlp, _, _ = _random_mlp(tdgp, rs, F, hid, n, marcher)
    pack = R._mlp_params_deep(mlp)
    two = R.TriPlaneMLP(F, hid, 3, marcher).to(DEV)
    hw = R.planes_to_hwc(T(rs.randn(B, 3 * F, H, H).astype(np.float32)))
    Rn = h * w
    ray_o = T(rs.uniform(-0.3, 0.3, (B, Rn, 3)).astype(np.float32))
    d = rs.randn(B, Rn, 3).astype(np.float32)
    ray_d = T(d / np.linalg.norm(d, axis=-1, keepdims=True))
    t = T(np.sort(rs.uniform(0.4, 1.6, (B, Rn, S)).astype(np.float32), axis=-1))           # the cube is [-0.5, 0.5]^3: samples leave it
    coords = (ray_o.unsqueeze(-2) + t.unsqueeze(-1) * ray_d.unsqueeze(-2)).reshape(B, Rn * S, 3)
    assert float((coords.abs().amax(-1) > 0.5).float().mean()) > 0.2
    noise = T(rs.randn(B, Rn * S).astype(np.float32))
    taps2 = torch.empty([B, Rn * S, 3, 2], dtype=torch.int32, device=DEV)
    R._field(hw, R._mlp_params(two), 0.5, coords=coords, tap_idx=taps2)
    for kw in (dict(), dict(sigma_noise=noise, density_noise=0.8)):
        outs, taps = [], []
        for mode in (dict(ray_o=ray_o, ray_d=ray_d, t=t, ray_w=w), dict(ray_o=ray_o, ray_d=ray_d, t=t, ray_w=0), dict(coords=coords)):
            tp = torch.full([B, Rn * S, 3, 2], -99, dtype=torch.int32, device=DEV)
            outs.append(R._field(hw, pack, 0.5, tap_idx=tp, **mode, **kw))
            taps.append(tp)
            plain = R._field(hw, pack, 0.5, **mode, **kw)                                 # the instantiation without tap rows
            assert torch.equal(plain, outs[-1])
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        for tp in taps:
            assert torch.equal(tp, taps2)
    plain = R._field(hw, pack, 0.5, coords=coords)
    noisy = R._field(hw, pack, 0.5, coords=coords, sigma_noise=noise, density_noise=0.8)
    assert torch.equal(plain[..., :3], noisy[..., :3])
    assert torch.equal(noisy[..., 3], plain[..., 3] + noise * 0.8)


# ------------------------------------------------------------------------------------------------ 3b. every branch of the shared addressing
@pytest.mark.parametrize('F,hid', [(8, 16), (32, 64)])
def test_shared_addressing_at_every_branch(tdgp, F, hid):
    rs = np.random.RandomState(500 + F)
    R = tdgp.renderer
    B, H, W, scale = 2, 5, 7, 0.5
    one = _addressing_coords(scale)
    coords = np.stack([one, one[::-1]])                                            # 2 x 37 points: no multiple of 16 or of 32
    P = coords.shape[1]
    assert (B * P) % 16 and (B * P) % 32 and P % 16
    # the list lands where it is meant to: every cell from the lower clamp to the upper one on both axes, out-of-range +1 neighbours on one axis alone
    cells = _expected_cells(coords, scale, H, W)
    assert set(cells[..., 0].ravel()) >= {-2, -1, 0, W - 2, W - 1, W} and set(cells[..., 1].ravel()) >= {-2, -1, 0, H - 2, H - 1, H}
    xy = cells[0, :, 0]
    assert ((xy[:, 0] == W - 1) & (xy[:, 1] >= 0) & (xy[:, 1] < H - 1)).any() and ((xy[:, 1] == H - 1) & (xy[:, 0] >= 0) & (xy[:, 0] < W - 1)).any()
    with torch.no_grad():                                                          # and float64 sees the same cells (the file's _reference: grid_sample's own floor)
        c64 = torch.as_tensor(coords, dtype=torch.float64) / scale
        for pl, (u, v) in enumerate(((0, 1), (0, 2), (1, 2))):
            ref_cell = torch.stack([torch.floor((c64[..., u] + 1) * (W - 1) / 2).clamp(-2, W), torch.floor((c64[..., v] + 1) * (H - 1) / 2).clamp(-2, H)], dim=-1)
            assert np.array_equal(ref_cell.numpy().astype(np.int32), cells[..., pl, :])
    planes = rs.randn(B, 3 * F, H, W).astype(np.float32)
    d_out = rs.randn(B, P, 4).astype(np.float32)
    hw = R.planes_to_hwc(T(planes))
    taps = {}
    for n in (2, 3, 4):
        mlp, ws, bs = _random_mlp(tdgp, rs, F, hid, n, 'classical')
        pack = R._mlp_params(mlp) if n == 2 else R._mlp_params_deep(mlp)
        taps[n] = torch.full([B, P, 3, 2], -99, dtype=torch.int32, device=DEV)
        got = R._field(hw, pack, scale, coords=T(coords), tap_idx=taps[n])
        refs = {}
        for dtype in (torch.float64, torch.float32):
            x, c = _cpu([planes, coords], dtype, grad=True)
            out = _reference(x, c, _cpu(ws, dtype), _cpu(bs, dtype), 'classical', scale, dtype)
            g = torch.autograd.grad(out, [x, c], torch.as_tensor(d_out).to(dtype))
            refs[dtype] = dict(out=out.detach().numpy(), d_planes=g[0].numpy(), d_coords=g[1].numpy())
        _within_reference_noise(N(got), refs[torch.float64]['out'], refs[torch.float32]['out'], f'addressing branches F {F} hid {hid} n_layers {n} forward')
        # each gradient kernel against float64 autograd (not against the other kernel); the MLP gradients are not part of this comparison
        res = R.simple_tri_plane_renderer_backward(T(planes), T(coords), mlp, T(d_out[..., :3]), T(d_out[..., 3:]), scale=scale, coords_grad=True)
        for name, t in (('d_planes', R.planes_from_hwc(res[0])), ('d_coords', res[-1])):
            _within_reference_noise(N(t), refs[torch.float64][name], refs[torch.float32][name], f'addressing branches F {F} hid {hid} n_layers {n} {name}')
    assert torch.equal(taps[2], taps[3]) and torch.equal(taps[2], taps[4])          # byte for byte
    assert np.array_equal(N(taps[2]), cells)


# ------------------------------------------------------------------------------------------------ 4. edges
def test_edges_and_refusals(tdgp):
    rs = np.random.RandomState(4)
    R = tdgp.renderer
    F, hid, H, B = 32, 64, 16, 2
    mlp, ws, bs = _random_mlp(tdgp, rs, F, hid, 3, 'classical')
    pack = R._mlp_params_deep(mlp)
    planes = rs.randn(B, 3 * F, H, H).astype(np.float32)
    hw = R.planes_to_hwc(T(planes))
    empty = R._field(hw, pack, 0.5, coords=torch.empty([B, 0, 3], device=DEV))
    assert tuple(empty.shape) == (B, 0, 4)
    coords = rs.uniform(-0.5, 0.5, (B, 1, 3)).astype(np.float32)
    one = R._field(hw, pack, 0.5, coords=T(coords))
    with torch.no_grad():
        ref64 = _reference(*_cpu([planes, coords], torch.float64), _cpu(ws, torch.float64), _cpu(bs, torch.float64), 'classical', 0.5, torch.float64).numpy()
    _within_reference_noise(N(one), ref64, N(R._field_eager(hw, mlp, 0.5, coords=T(coords))), 'field_deep forward P = 1')

    def pack_of(F_, hid_, n):
        dims = [F_] + [hid_] * (n - 1) + [4]
        return ([T(rs.randn(o, i).astype(np.float32)) for i, o in zip(dims[:-1], dims[1:])], [T(rs.randn(o).astype(np.float32)) for o in dims[1:]], 'classical')

    c = T(rs.uniform(-0.5, 0.5, (B, 40, 3)).astype(np.float32))
    hw64 = R.planes_to_hwc(T(rs.randn(B, 3 * 64, H, H).astype(np.float32)))
    tdgp._lib.profile_enable(True)
    try:
        # a pack of (weights, biases, marcher) routes to the deep entry point whatever its depth: n_layers 2 and 5, hid 128, widths outside the table
        for planes_, pk in ((hw, pack_of(32, 64, 2)), (hw, pack_of(32, 64, 5)), (hw, pack_of(32, 128, 3)), (hw64, pack_of(64, 128, 3)), (hw, pack_of(32, 48, 3))):
            with pytest.raises(tdgp._lib.Unsupported):
                R._field(planes_, pk, 0.5, coords=c)
        torch.cuda.synchronize()
        assert not any('deep' in k for k in tdgp._lib.profile_report())                      # refused before any launch
    finally:
        tdgp._lib.profile_enable(False)
    # the gradient entry point refuses the same depths and hid 128
    wide = R.TriPlaneMLP(32, 128, 3, 'classical', n_layers=3).to(DEV)
    assert not R.deep_form(wide)
    assert int(tdgp._lib.load().tdgp_triplane_field_deep_grad_workspace_bytes(B, 40, 32, 64, 2)) == -1
    assert int(tdgp._lib.load().tdgp_triplane_field_deep_grad_workspace_bytes(B, 40, 32, 64, 5)) == -1


# ------------------------------------------------------------------------------------------------ 5. gradient vs fixtures
def _grad_dict(R, res, n, coords_grad):
    out = dict(d_planes=R.planes_from_hwc(res[0])) if res[0] is not None else {}
    for i in range(n):
        out[f'd_w{i}'], out[f'd_b{i}'] = res[1][i], res[2][i]
    if coords_grad:
        out['d_coords'] = res[3]
    return out


@pytest.mark.parametrize('tag', ['small_n3', 'hot_n4'])
@pytest.mark.parametrize('marcher', ['classical', 'mip'])
def test_gradient_vs_reference_fixture(tdgp, tag, marcher):
    g = load_golden('field_deep')
    R = tdgp.renderer
    mlp, n, ref32, ref64 = _fixture_case(tdgp, g, tag, marcher)
    args = (T(g[f'{tag}_planes']), T(g[f'{tag}_coords']), mlp, T(g[f'{tag}_d_rgb']), T(g[f'{tag}_d_sigma']))
    res = R.simple_tri_plane_renderer_backward(*args, scale=0.5, coords_grad=True)
    assert len(res) == 4 and len(res[1]) == n and len(res[2]) == n
    got = _grad_dict(R, res, n, True)
    for name, t in got.items():
        _within_reference_noise(N(t), ref64(name), ref32(name), f'field_deep grad {tag} {marcher} {name}')
    res2 = R.simple_tri_plane_renderer_backward(*args, scale=0.5)
    assert len(res2) == 3
    for a, b in zip(res[1] + res[2], res2[1] + res2[2]):
        assert torch.equal(a, b)                                                           # fixed reduction order: identical bytes run to run
    assert_close(N(res2[0]), N(res[0]), 1e-5, 'd_planes run to run', 1.0)
    only = R.simple_tri_plane_renderer_backward(*args, scale=0.5, planes_grad=False, coords_grad=True)
    assert only[0] is None and torch.equal(only[3], res[3])
    for a, b in zip(res[1] + res[2], only[1] + only[2]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. gradient at many tiles
def test_gradient_many_tiles_vs_float64(tdgp):
    rs = np.random.RandomState(77)
    R = tdgp.renderer
    B, F, H, hid, P, n = 2, 32, 32, 64, 33333, 3
    planes = rs.randn(B, 3 * F, H, H).astype(np.float32)
    coords = rs.uniform(-0.6, 0.6, (B, P, 3)).astype(np.float32)
    d_out = rs.randn(B, P, 4).astype(np.float32)
    mlp, ws, bs = _random_mlp(tdgp, rs, F, hid, n, 'classical')
    # lrelu has a kink at zero, and of 8.5 M pre-activations a few lie within fp32 rounding of it: two correct computations then take different slopes
    # (1 against 0.2) and differ by that point's whole contribution (measured on the unmasked inputs: the fp32 reference 2.1e-2 of max |d_planes| from its
    # own float64 run, the kernel 5.1e-3 from the fp32 reference), which would hide a wrong point of the ragged last tile.  So the points with a
    # pre-activation within 1e-4 of zero (float64 run; fp32 evaluations of these O(1) sums differ by ~1e-6) get a zero incoming gradient: about 1 %
    # of the points, and every remaining one has the same slopes in any evaluation.
    kink = []
    with torch.no_grad():
        _reference(*_cpu([planes, coords], torch.float64), _cpu(ws, torch.float64), _cpu(bs, torch.float64), 'classical', 0.5, torch.float64, nearest_kink=kink)
    ambiguous = (torch.stack(kink).amin(dim=0) < 1e-4).numpy()
    assert 0 < ambiguous.mean() < 0.03 and not ambiguous[-1, -10:].all()         # the ten points of the ragged last tile are (mostly) kept
    d_out[ambiguous] = 0.0
    names = ['d_planes', 'd_coords'] + [f'd_w{i}' for i in range(n)] + [f'd_b{i}' for i in range(n)]
    refs = {}
    for dtype in (torch.float64, torch.float32):
        x, c = _cpu([planes, coords], dtype, grad=True)
        w_, b_ = _cpu(ws, dtype, grad=True), _cpu(bs, dtype, grad=True)
        out = _reference(x, c, w_, b_, 'classical', 0.5, dtype)
        grads = torch.autograd.grad(out, [x, c] + w_ + b_, torch.as_tensor(d_out).to(dtype))
        refs[dtype] = dict(zip(names, [t.numpy() for t in grads]))
    res = R.simple_tri_plane_renderer_backward(T(planes), T(coords), mlp, T(d_out[..., :3]), T(d_out[..., 3:]), scale=0.5, coords_grad=True)
    got = _grad_dict(R, res, n, True)
    for name in names:
        _within_reference_noise(N(got[name]), refs[torch.float64][name], refs[torch.float32][name], f'field_deep grad 2 x 33333 points {name}')
    # and directly against the fp32 run: 1e-4 of max |ref|, the figure test_field_grad_large holds the two-layer kernel to at this shape
    for name in names:
        ref = refs[torch.float32][name]
        err = float(np.abs(N(got[name]).astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))
        print(f'field_deep grad 2 x 33333 points {name}: kernel vs fp32 autograd {err:.3e}')
        report_parity(f'field_deep grad 2 x 33333 points {name} vs fp32 autograd', err=err)
        assert err <= 1e-4, f'{name}: {err:.3e} of max |ref| from the fp32 autograd result'


# ------------------------------------------------------------------------------------------------ 7. renderer chain
def test_importance_renderer_backward_three_layers(tdgp):
    g = load_golden('field_deep')
    mlp = _deep_mlp(tdgp, [g[f'r_w{i}'] for i in range(3)], [g[f'r_b{i}'] for i in range(3)], 'classical')
    opts = dict(box_size=1.0, num_proposal_steps=8, num_fine_steps=8, clamp_mode='softplus', use_inf_depth=True, ray_start=0.75, ray_end=1.25,
                white_back=False, density_bias=0.0, u_coarse=T(g['r_u_coarse']), u_fine=T(g['r_u_fine']))
    rend = tdgp.renderer.ImportanceRenderer('classical')
    rgb, _, _, _ = rend(T(g['r_planes']), mlp, T(g['r_ray_o']), T(g['r_ray_d']), opts)
    assert_close(N(rgb), g['r_rgb'], 1e-5, 'rgb', 1.0)
    res = rend.backward(T(g['r_planes']), mlp, T(g['r_ray_o']), T(g['r_ray_d']), opts, T(g['r_d_rgb']), T(g['r_d_depth']))
    assert sorted(res) == ['b0', 'b1', 'b2', 'planes', 'w0', 'w1', 'w2']
    for name in ('planes', 'w0', 'b0', 'w1', 'b1', 'w2', 'b2'):
        assert_close(N(res[name]), g['r_d_' + name], 1e-4, 'd_' + name, 1.0)


# ------------------------------------------------------------------------------------------------ 8. generator
def test_generator_with_three_layer_decoder_trains(tdgp):
    cfg = tdgp.config.config_tiny()
    cfg.mlp_n_layers = 3
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=81, exercise_all=True))
    G = G.to(DEV)
    assert tdgp.renderer.deep_form(G.synthesis.tri_plane_mlp)
    for p in G.parameters():
        p.requires_grad_(True)
    inp = tdgp.weights.synthetic_inputs(cfg, batch=2, seed=82)
    cam = {k: T(v) for k, v in inp['camera'].items()}
    img = G.forward_autograd(T(inp['z']), T(inp['c']), cam, noise_mode='const', u_coarse=T(inp['u_coarse']), u_fine=T(inp['u_fine']))
    assert img.shape == (2, 3, cfg.img_resolution, cfg.img_resolution) and torch.isfinite(img).all()
    img.square().mean().backward()
    mlp_params = dict(G.synthesis.tri_plane_mlp.named_parameters())
    assert sorted(mlp_params) == [f'model.{i}.{k}' for i in range(3) for k in ('bias', 'weight')]
    for name, p in list(mlp_params.items()) + [('tri_plane_decoder.' + k, v) for k, v in G.synthesis.tri_plane_decoder.named_parameters()]:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0, name
    with torch.no_grad():
        ev = G(T(inp['z']), T(inp['c']), cam, noise_mode='const', u_coarse=T(inp['u_coarse']), u_fine=T(inp['u_fine']))
    assert ev.shape == (2, 3, cfg.img_resolution, cfg.img_resolution) and torch.isfinite(ev).all()


def test_feat64_decoder_is_forward_only_and_says_so_up_front(tdgp):
    """feat_dim 64 / hid_dim 64 is in the forward table, not in the gradient kernel's: `render_autograd` refuses before the forward runs."""
    R = tdgp.renderer
    mlp = R.TriPlaneMLP(64, 64, 3, 'classical', n_layers=3).to(DEV)
    assert R.deep_form(mlp)
    opts = dict(box_size=1.0, num_proposal_steps=8, num_fine_steps=8, clamp_mode='softplus', use_inf_depth=True, ray_start=0.75, ray_end=1.25)
    planes = torch.randn([1, 3 * 64, 16, 16], device=DEV, requires_grad=True)
    rays = torch.zeros([1, 16, 3], device=DEV)
    with pytest.raises(NotImplementedError, match='forward-only'):
        R.render_autograd(R.ImportanceRenderer('classical'), planes, mlp, rays, rays, opts)

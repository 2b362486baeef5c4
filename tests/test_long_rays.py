"""Long rays: up to 512 coarse + 512 fine samples per ray -- what the reference's inference harness renders with `ray_step_multiplier`
(scripts/inference.py:44-46) -- through every layer: the long-ray kernels of csrc/sampling.hip, the renderer, the eval forward's split at
the field kernel's index bound and `inference.configure_for_inference`.  Reference vectors: tests/golden/sampling_long.npz and
e2e_long.npz (tools/gen_goldens.py:gen_sampling_long / gen_e2e_long).

Bars as in test_gpu_parity.py: integer rows (searchsorted indices, sort permutations) and the fine samples bit-exact on identical inputs;
the fused kernels bit-identical to the staged op chain; the marcher within test_march_classical's tolerances of the oracle; the image
through conftest.assert_image_parity; integer rows through the whole chain explained by a knot window."""
import hashlib
import importlib

import numpy as np
import pytest
import torch

from conftest import assert_close, assert_image_parity, assert_inds_mismatches_in_window, load_golden, max_rel, report_parity

DEV = 'cuda:0'
LONG_S = (192, 256, 384, 512)
gpu = pytest.mark.gpu


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def N(t):
    return t.detach().float().cpu().numpy()


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def unify_long_payload(lead, S1, S2):
    """The colours / densities riding along in sampling_long's unify vectors (tools/gen_goldens.py:unify_long_payload): only the depths
    decide the permutation, so they are regenerated from a seed instead of stored."""
    rs = np.random.RandomState(S1 * 7 + S2)
    return (rs.randn(*lead, S1, 3).astype(np.float32), rs.randn(*lead, S1, 1).astype(np.float32),
            rs.randn(*lead, S2, 3).astype(np.float32), rs.randn(*lead, S2, 1).astype(np.float32))


def _unified_by(perm, d1, c1, s1, d2, c2, s2):
    """concat + gather by a sort permutation: what unify_samples returns for that permutation (tri_plane_renderer.py:196-206)."""
    p = np.asarray(perm, np.int64)[..., None]
    cat = lambda a, b: np.concatenate([a, b], axis=2)                 # noqa: E731
    return (np.take_along_axis(cat(d1, d2), p, 2), np.take_along_axis(cat(c1, c2), np.broadcast_to(p, p.shape[:3] + (3,)), 2),
            np.take_along_axis(cat(s1, s2), p, 2))


def _tdgp():
    return importlib.import_module('3dgp_amd')


# ------------------------------------------------------------------------------------------------ CPU: the goldens and the host checks

@pytest.mark.parametrize('marcher', ['classical', 'mip'])
@pytest.mark.parametrize('S', LONG_S)
def test_oracle_reproduces_sampling_long(oracle, marcher, S):
    """The oracle (torch's CPU sum order spelled out, orc_torch_row_sum) reproduces the reference's searchsorted indices and fine samples
    at S up to 512: guards the golden the GPU test reads."""
    g = load_golden('sampling_long')
    tag = f'{marcher}{S}'
    osf, oaux = oracle.sample_importance(g[f'{tag}_sdist'], g[f'{tag}_weights'], g[f'{tag}_u_fine'], marcher, return_aux=True)
    np.testing.assert_array_equal(np.asarray(oaux['inds']).reshape(-1).astype(np.int64), g[f'{tag}_inds'].reshape(-1).astype(np.int64))
    np.testing.assert_array_equal(np.asarray(osf).reshape(-1), g[f'{tag}_sdist_fine'].reshape(-1))


def assert_differs_only_inside_ties(perm, ref_perm, d1, d2, what):
    """Two sort permutations of the same lists: the sorted depths are identical, and where the permutations differ the depths are equal
    (a different order inside a group of equal depths).  Returns the number of slots that differ."""
    d = np.concatenate([d1, d2], 2)[..., 0]
    a, b = np.asarray(perm, np.int64).reshape(d.shape), np.asarray(ref_perm, np.int64).reshape(d.shape)
    np.testing.assert_array_equal(np.take_along_axis(d, a, -1), np.take_along_axis(d, b, -1), err_msg=what)
    return int((a != b).sum())


@pytest.mark.parametrize('S', [256, 512])
def test_oracle_reproduces_unify_long(oracle, S):
    """unify_samples at 256 + 256 and 512 + 512.  Without ties the oracle's permutation is the reference's and gathering by it gives the
    reference's outputs (their sha256 is in the golden).  With ties it is NOT: the reference sorts with torch.sort(stable=False), whose CPU
    kernel (torch 2.10) is an introsort beyond 16 elements and orders equal depths its own way -- recorded here: the oracle and the kernels
    keep the stable order (coarse before fine, then list order), which differs from the reference's only inside groups of equal depths."""
    g = load_golden('sampling_long')
    d1, d2 = g[f'un{S}_d1'], g[f'un{S}_d2']
    c1, s1, c2, s2 = unify_long_payload(d1.shape[:2], S, S)
    _, _, _, perm = oracle.unify_samples(d1, c1, s1, d2, c2, s2, return_perm=True)
    want = g[f'un{S}_perm'].astype(np.int64)
    np.testing.assert_array_equal(np.asarray(perm).reshape(want.shape).astype(np.int64), want)
    np.testing.assert_array_equal(sha256(*_unified_by(want, d1, c1, s1, d2, c2, s2)), g[f'un{S}_out_sha256'])
    d1, d2 = g[f'un{S}_ties_d1'], g[f'un{S}_ties_d2']
    _, _, _, perm = oracle.unify_samples(d1, c1, s1, d2, c2, s2, return_perm=True)
    stable = np.argsort(np.concatenate([d1, d2], 2)[..., 0], axis=-1, kind='stable')
    np.testing.assert_array_equal(np.asarray(perm).reshape(stable.shape), stable)
    n = assert_differs_only_inside_ties(perm, g[f'un{S}_ties_perm'], d1, d2, f'oracle vs reference, {S} + {S} with ties')
    report_parity(f'unify_samples {S} + {S} with ties: stable order vs the reference (torch.sort, stable=False)', slots_in_other_tie_order=n,
                  slots=int(stable.size))
    assert n > 0          # the golden does exercise the reference's non-stable tie order


def test_configure_for_inference():
    """scripts/inference.py:38-48 on our Generator: resolution, multiplied step count, far plane, white background, no density noise --
    and what the renderer is then asked for.  The settings of the issue (3dgp x 8, epigraf x 4, a 96-step model x 2) fit."""
    tdgp = _tdgp()
    for steps, mult, want in ((32, 8, 256), (48, 4, 192), (96, 2, 192), (64, 8, 512)):
        cfg = tdgp.config.config_tiny()
        cfg.num_ray_steps = steps
        G = tdgp.generator.Generator(cfg)
        G.synthesis.nerf_noise_std = 0.3
        wb, end = cfg.white_back, cfg.ray_end
        assert tdgp.inference.configure_for_inference(G, 64, mult, far_plane_offset=1.0) is G
        assert G.cfg.num_ray_steps == want
        assert G.synthesis.img_resolution == G.synthesis.test_resolution == 64
        assert G.cfg.ray_end == end + 1.0 and G.cfg.white_back == wb
        assert G.synthesis.nerf_noise_std == 0
        opts = G.synthesis.rendering_options(G.synthesis._default_render_options)
        assert opts['num_proposal_steps'] == opts['num_fine_steps'] == want
        assert opts['ray_end'] == end + 1.0 and opts['white_back'] == wb
    G = tdgp.generator.Generator(tdgp.config.config_tiny())
    tdgp.inference.configure_for_inference(G, 32, 2, force_whiteback=True)
    assert G.cfg.white_back and G.cfg.ray_end == 1.25 and G.cfg.num_ray_steps == 16
    assert G.synthesis.rendering_options(G.synthesis._default_render_options)['white_back']


def test_configure_for_inference_refuses_more_than_512_steps():
    tdgp = _tdgp()
    G = tdgp.generator.Generator(tdgp.config.config_tiny())          # 8 steps
    with pytest.raises(NotImplementedError, match='512'):
        tdgp.inference.configure_for_inference(G, 64, 65)
    assert G.cfg.num_ray_steps == 8 and G.synthesis.test_resolution == 16      # nothing was changed


def test_forward_counts_above_512_refused_before_work():
    """ImportanceRenderer.forward refuses S or N above 512 (TDGP_EUNSUPPORTED's exception, naming the limit) before it touches its inputs --
    CPU tensors here, which it would otherwise reject for not being on the GPU; 512 + 512 passes the check."""
    tdgp = _tdgp()
    rend = tdgp.renderer.ImportanceRenderer('classical')
    ro = torch.zeros(1, 4, 3)
    base = dict(box_size=1.0, clamp_mode='softplus', use_inf_depth=True, ray_start=0.75, ray_end=1.25)
    for S, N_ in ((513, 512), (512, 513), (1024, 1)):
        with pytest.raises(tdgp._lib.Unsupported, match='512'):
            rend(None, None, ro, ro, dict(base, num_proposal_steps=S, num_fine_steps=N_))
    with pytest.raises(RuntimeError, match='GPU'):
        rend(None, None, ro, ro, dict(base, num_proposal_steps=512, num_fine_steps=512))


def test_autograd_counts_above_256_refused_before_work():
    """The gradient path keeps tdgp_ray_march_grad's limit (S + N <= 256 merged samples): refused at the call with NotImplementedError,
    before the mapping network, the backbone or any kernel runs (the generator lives on the CPU here: any work would fail differently)."""
    tdgp = _tdgp()
    cfg = tdgp.config.config_tiny()
    G = tdgp.generator.Generator(cfg)
    tdgp.inference.configure_for_inference(G, 16, 17)               # 136 + 136
    cam = dict(angles=torch.zeros(1, 3), fov=torch.full([1], 20.0), radius=torch.ones(1), look_at=torch.zeros(1, 3))
    with pytest.raises(NotImplementedError, match='256'):
        G.forward_autograd(torch.zeros(1, cfg.z_dim), torch.zeros(1, 0), cam)
    with pytest.raises(NotImplementedError, match='256'):
        G.synthesis.forward_autograd(torch.zeros(1, G.num_ws, cfg.w_dim), cam)
    with pytest.raises(NotImplementedError, match='256'):
        tdgp.renderer.render_autograd(G.synthesis.renderer, None, G.synthesis.tri_plane_mlp, None, None,
                                      dict(num_proposal_steps=200, num_fine_steps=57))


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope='module')
def native():
    tdgp = _tdgp()
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()        # raises if libtdgp_hip.so is missing: GPU tests never run on a fallback
    return tdgp


def _mlp(tdgp, w0, b0, w1, b1, marcher):
    m = tdgp.renderer.TriPlaneMLP(w0.shape[1], w0.shape[0], 3, marcher).to(DEV)
    with torch.no_grad():
        m.model[0].weight.copy_(T(w0)); m.model[0].bias.copy_(T(b0)); m.model[1].weight.copy_(T(w1)); m.model[1].bias.copy_(T(b1))
    return m


@gpu
@pytest.mark.parametrize('marcher', ['classical', 'mip'])
@pytest.mark.parametrize('S', LONG_S)
def test_sample_importance_long(native, oracle, marcher, S):
    """tdgp_sample_importance at S = 192 ... 512 (the long kernel above 256) against vectors captured from the reference: searchsorted
    indices and fine samples bit for bit, the cdf equal to the oracle's."""
    g = load_golden('sampling_long')
    tag = f'{marcher}{S}'
    R = native.renderer.ImportanceRenderer(marcher)
    sf, aux = R.sample_importance(T(g[f'{tag}_sdist']), T(g[f'{tag}_weights']), S, u=T(g[f'{tag}_u_fine']), return_aux=True)
    np.testing.assert_array_equal(aux['inds'].cpu().numpy().reshape(-1).astype(np.int64), g[f'{tag}_inds'].reshape(-1).astype(np.int64))
    np.testing.assert_array_equal(N(sf).reshape(-1), g[f'{tag}_sdist_fine'].reshape(-1))
    _, oaux = oracle.sample_importance(g[f'{tag}_sdist'], g[f'{tag}_weights'], g[f'{tag}_u_fine'], marcher, return_aux=True)
    np.testing.assert_array_equal(N(aux['cdf']).reshape(-1), np.asarray(oaux['cdf']).reshape(-1))


@gpu
@pytest.mark.parametrize('S', [256, 512])
def test_unify_long(native, S):
    """tdgp_unify_samples at 256 + 256 and 512 + 512 (the long kernel): without ties the permutation and the outputs are the reference's bit for
    bit; with ties across and inside the lists the permutation is the stable order (coarse before fine, then list order: the short kernel's),
    and the sorted depths are the reference's (its own order inside a tie group is torch's non-stable CPU sort: test_oracle_reproduces_unify_long)."""
    g = load_golden('sampling_long')
    R = native.renderer.ImportanceRenderer('classical')
    for ties in ('', '_ties'):
        d1, d2 = g[f'un{S}{ties}_d1'], g[f'un{S}{ties}_d2']
        c1, s1, c2, s2 = unify_long_payload(d1.shape[:2], S, S)
        d, c, s, perm = R.unify_samples(T(d1), T(c1), T(s1), T(d2), T(c2), T(s2), return_perm=True)
        want = g[f'un{S}{ties}_perm'].astype(np.int64)
        if not ties:
            np.testing.assert_array_equal(perm.cpu().numpy().astype(np.int64), want)
            np.testing.assert_array_equal(sha256(N(d), N(c), N(s)), g[f'un{S}_out_sha256'])
        else:
            stable = np.argsort(np.concatenate([d1, d2], 2)[..., 0], axis=-1, kind='stable')
            np.testing.assert_array_equal(perm.cpu().numpy().astype(np.int64), stable)
            assert_differs_only_inside_ties(perm.cpu().numpy(), want, d1, d2, f'unify {S} + {S} with ties')
            np.testing.assert_array_equal(sha256(*_unified_by(stable, d1, c1, s1, d2, c2, s2)), sha256(N(d), N(c), N(s)))


@gpu
@pytest.mark.parametrize('S,kw', [(512, dict(use_inf_depth=True)), (512, dict(use_inf_depth=False, last_back=True)), (1024, dict(use_inf_depth=True))])
def test_ray_march_long(native, oracle, S, kw):
    """tdgp_ray_march on rays of 512 samples (and 1024: the staged path marches the merged list) against the oracle, within
    test_march_classical's tolerances.  (With a 1-ulp expf in alpha = 1 - exp(-delta sigma) the weights were 3.9e-6 from the oracle at 512
    samples and 7.9e-6 at 1024: the cancellation grows with 1 / delta.  The long form rounds exp from fp64: measured ~1e-7, the report.)"""
    rs = np.random.RandomState(S + len(kw))
    B, R = 2, 40
    depths = np.sort(rs.uniform(0.75, 1.25, (B, R, S, 1)), axis=2).astype(np.float32)
    dens = (rs.randn(B, R, S, 1) * 3.0 + 1.0).astype(np.float32) * (rs.rand(B, R, S, 1) > 0.3)
    colors = rs.randn(B, R, S, 3).astype(np.float32)
    rgb, dep, w, fT = native.renderer.ClassicalRayMarcher()(T(colors), T(dens), T(depths), dict(kw))
    orgb, odep, ow, ofT = oracle.march_classical(colors, dens, depths, **kw)
    report_parity(f'ray_march {S} samples {kw} vs oracle', weights=max_rel(N(w), ow, 1.0), T=max_rel(N(fT), ofT), rgb=max_rel(N(rgb), orgb, 1.0),
                  depth=max_rel(N(dep), odep, 1.0))
    assert_close(N(w), ow, 1e-6, 'weights vs oracle', 1.0)
    assert_close(N(fT), ofT, 2e-6, 'T vs oracle')
    assert_close(N(rgb), orgb, 1e-6, 'rgb vs oracle', 1.0)
    assert_close(N(dep), odep, 5e-6, 'depth vs oracle', 1.0)


def _scene(tdgp, rs, marcher, B=2, hw=12):
    F, H, hid = 8, 32, 16
    planes = T(rs.randn(B, 3 * F, H, H))
    mlp = _mlp(tdgp, rs.randn(hid, F), 0.3 * rs.randn(hid), rs.randn(4, hid), 0.3 * rs.randn(4), marcher)
    cam = dict(angles=T([[0.3, 1.2, 0.0], [-0.6, 1.8, 0.0]][:B]), radius=T([1.0, 1.0][:B]), look_at=T(np.zeros((B, 3))))
    ro, rd = tdgp.renderer.sample_rays(tdgp.renderer.compute_cam2world_matrix(cam), T([25.0, 40.0][:B]), (hw, hw))
    return planes, mlp, ro, rd


@gpu
@pytest.mark.parametrize('S,Nf', [(192, 192), (256, 256), (512, 512), (64, 512), (512, 64), (129, 1), (384, 192), (512, 100), (300, 40)])
def test_long_fused_pair_equals_op_chain(native, S, Nf):
    """tdgp_importance_from_coarse + tdgp_merge_composite (the staged renderer with intermediates) against the reference-named op chain
    (sample_stratified -> run_model -> ray_marcher -> sample_importance -> run_model -> unify_samples -> ray_marcher), bit for bit: fine
    samples and indices in draw order, the fine list written ascending with fine_perm = its stable (depth, draw index) order, the merged
    permutation, rgb / depth / final transmittance; both marchers, equal and unequal lists.  The long importance kernel (S or N above 256)
    is reached with every fine-list sort it has: N <= 64 and N <= 128 (counting ranks), N <= 256 and N <= 512 (the bitonic network over 4 /
    8 slots); the merge with its 512- and 1024-slot forms."""
    tdgp = native
    rs = np.random.RandomState(S * 1000 + Nf)
    for marcher in ('classical', 'mip'):
        planes, mlp, ro, rd = _scene(tdgp, rs, marcher)
        B, R = ro.shape[:2]
        u1, u2 = rs.rand(B, R, S, 1).astype(np.float32), rs.rand(B * R, Nf).astype(np.float32)
        if Nf > 8:
            u2[::3, 5] = u2[::3, 2]                   # equal draws -> equal depths: the sort's tie order
        opts = dict(box_size=1.0, num_proposal_steps=S, num_fine_steps=Nf, clamp_mode='softplus', use_inf_depth=True, ray_start=0.75, ray_end=1.25,
                    white_back=(marcher == 'mip'), density_bias=0.0)
        rend = tdgp.renderer.ImportanceRenderer(marcher)
        (rgb, depth, wsum, fT), inter = rend(planes, mlp, ro, rd, dict(opts, u_coarse=T(u1), u_fine=T(u2)), return_intermediates=True)
        s2t = lambda s: s * opts['ray_end'] + (1 - s) * opts['ray_start']     # noqa: E731
        sd = rend.sample_stratified(ro, 0.0, 1.0, S, noise=T(u1))
        td = s2t(sd)
        out = rend.run_model(planes, mlp, (ro.unsqueeze(-2) + td * rd.unsqueeze(-2)).reshape(B, -1, 3), opts)
        cc, dc = out['rgb'].reshape(B, R, S, 3), out['sigma'].reshape(B, R, S, 1)
        _, _, w, _ = rend.ray_marcher(cc, dc, sd, opts)
        sf, aux = rend.sample_importance(sd, w, Nf, u=T(u2), return_aux=True)
        np.testing.assert_array_equal(N(inter['sdist_fine']).reshape(-1), N(sf).reshape(-1))
        np.testing.assert_array_equal(inter['inds'].cpu().numpy().reshape(-1), aux['inds'].cpu().numpy().reshape(-1))
        tf = s2t(sf)
        t_draw = N(tf).reshape(B * R, Nf)
        order = np.lexsort((np.broadcast_to(np.arange(Nf), t_draw.shape), t_draw))          # stable sort by (depth, draw index)
        np.testing.assert_array_equal(inter['fine_perm'].cpu().numpy().reshape(B * R, Nf).astype(np.int64), order)
        np.testing.assert_array_equal(N(inter['tdist_fine']).reshape(B * R, Nf), np.take_along_axis(t_draw, order, 1))
        out = rend.run_model(planes, mlp, (ro.unsqueeze(-2) + tf * rd.unsqueeze(-2)).reshape(B, -1, 3), opts)
        cf, df = out['rgb'].reshape(B, R, Nf, 3), out['sigma'].reshape(B, R, Nf, 1)
        d_all, c_all, s_all, perm = rend.unify_samples(td, cc, dc, tf, cf, df, return_perm=True)
        np.testing.assert_array_equal(inter['perm'].cpu().numpy().reshape(-1), perm.cpu().numpy().reshape(-1))
        rgb2, depth2, w2, fT2 = rend.ray_marcher(c_all, s_all, d_all, opts)
        np.testing.assert_array_equal(N(rgb), N(rgb2))
        np.testing.assert_array_equal(N(depth), N(depth2))
        np.testing.assert_array_equal(N(fT), N(fT2))
        assert_close(N(wsum), N(w2.sum(2)), 1e-6, 'weights.sum', 1.0)


@gpu
@pytest.mark.parametrize('S', [512, 300])
def test_long_merge_of_unsorted_lists(native, S):
    """tdgp_merge_composite's fallback for lists that are not ascending (arbitrary caller data: the stable rank over 8 / 16 slots per lane)
    against unify_samples -> ray_march, at S + S samples; permutation, rgb, depth and transmittance bit for bit."""
    L = native._lib
    rs = np.random.RandomState(S)
    rays = 70
    t1 = rs.uniform(0.75, 1.25, (rays, S)).astype(np.float32)
    t2 = rs.uniform(0.75, 1.25, (rays, S)).astype(np.float32)
    t1[::3].sort(axis=1)                                          # ascending and arbitrary lists in one launch
    t2[1::2].sort(axis=1)
    t1[5, 3] = t1[5, 7]
    t2[:, 9] = t1[:, 4]                                           # ties across the lists
    c1, c2 = rs.randn(rays, S, 4).astype(np.float32), rs.randn(rays, S, 4).astype(np.float32)
    flags = native.renderer._marcher_flags(dict(use_inf_depth=True), 'classical')
    dt1, dt2, dc1, dc2 = T(t1), T(t2), T(c1), T(c2)
    rgb, dep, wsum, fT = (torch.empty(rays, n, device=DEV) for n in (3, 1, 1, 1))
    perm = torch.empty(rays, 2 * S, dtype=torch.int32, device=DEV)
    L.call('tdgp_merge_composite', dc1.data_ptr(), dt1.data_ptr(), S, dc2.data_ptr(), dt2.data_ptr(), S, rgb.data_ptr(), dep.data_ptr(), wsum.data_ptr(),
           fT.data_ptr(), perm.data_ptr(), None, rays, 0, flags, 0.0, 0.0, L.stream_of(dt1))
    rend = native.renderer.ImportanceRenderer('classical')
    sh = lambda a, c: a.reshape(1, rays, -1, c)                   # noqa: E731
    d, c, sg, uperm = rend.unify_samples(sh(dt1, 1), sh(dc1[..., :3].contiguous(), 3), sh(dc1[..., 3].contiguous(), 1),
                                         sh(dt2, 1), sh(dc2[..., :3].contiguous(), 3), sh(dc2[..., 3].contiguous(), 1), return_perm=True)
    orgb, odep, ow, ofT = rend.ray_marcher(c, sg, d, dict(use_inf_depth=True))
    np.testing.assert_array_equal(perm.cpu().numpy(), uperm.reshape(rays, 2 * S).cpu().numpy())
    np.testing.assert_array_equal(N(rgb), N(orgb).reshape(rays, 3))
    np.testing.assert_array_equal(N(dep), N(odep).reshape(rays, 1))
    np.testing.assert_array_equal(N(fT).reshape(-1), N(ofT).reshape(-1))


@gpu
@pytest.mark.parametrize('marcher', ['classical', 'mip'])
def test_render_fused_long(native, marcher):
    """tdgp_render_fused at 256 + 256 samples per ray equals the staged entry points it stands for, bit for bit."""
    rs = np.random.RandomState(7)
    planes, mlp, ro, rd = _scene(native, rs, marcher, hw=16)
    B, R = ro.shape[:2]
    S = 256
    opts = dict(box_size=1.0, num_proposal_steps=S, num_fine_steps=S, clamp_mode='softplus', use_inf_depth=True, ray_start=0.75, ray_end=1.25,
                white_back=(marcher == 'mip'), density_bias=0.0, u_coarse=T(rs.rand(B, R, S, 1)), u_fine=T(rs.rand(B * R, S)), ray_grid_w=16)
    rend = native.renderer.ImportanceRenderer(marcher)
    fused = rend(planes, mlp, ro, rd, opts)
    rend.fused_entry = False
    staged = rend(planes, mlp, ro, rd, opts)
    for a, b, name in zip(fused, staged, ('rgb', 'depth', 'wsum', 'final_T')):
        assert torch.equal(a, b), (marcher, name)


def _gen(tdgp, cfg, seed):
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=seed, exercise_all=True))
    return G.to(DEV)


@gpu
def test_e2e_long(native, oracle):
    """The reference's whole G.synthesis at config_tiny with 384 + 384 samples per ray (e2e_long.npz): image and depth through
    assert_image_parity (the oracle's image as the exactly rounded one); the importance stage on the reference's own inputs bit for bit;
    through the whole chain at most 4 integer mismatches in `inds` and in `perm`, every `inds` mismatch explained by a knot window."""
    tdgp = native
    g = load_golden('e2e_long')
    cfg = tdgp.config.config_tiny()
    cfg.num_ray_steps = 384
    seed = int(g['seed'][0])
    inp = tdgp.weights.synthetic_inputs(cfg, batch=int(g['seed'][1]), seed=seed + 1)
    np.testing.assert_array_equal(sha256(inp['u_coarse'], inp['u_fine']), g['draws_sha256'])
    G = _gen(tdgp, cfg, seed)
    ws = T(g['ws'])
    cam = {k[4:]: T(v) for k, v in g.items() if k.startswith('cam_')}
    out = G.synthesis(ws, camera_params=cam, noise_mode='const', render_opts=dict(return_depth=True), u_coarse=T(inp['u_coarse']), u_fine=T(inp['u_fine']))
    sd = tdgp.weights.random_state_dict(cfg, seed=seed, exercise_all=True)
    ex_img, ex_depth = oracle.synthesis_forward(sd, cfg.to_dict(), g['ws'], {k[4:]: v for k, v in g.items() if k.startswith('cam_')},
                                                inp['u_coarse'], inp['u_fine'], 'const')
    assert_image_parity(N(out.img), g, 'e2e_long img', exact=ex_img)
    assert_image_parity(N(out.depth), g, 'e2e_long depth', 'depth', exact=ex_depth)
    # the importance stage on the reference's own inputs: coarse depths (regenerated from the draws), weights -> indices, fine samples
    rend = G.synthesis.renderer
    B, R, S = inp['u_coarse'].shape
    sdist = rend.sample_stratified(torch.zeros(B, R, 3, device=DEV), 0.0, 1.0, S, noise=T(inp['u_coarse']).reshape(B, R, S, 1))
    np.testing.assert_array_equal(sha256(N(sdist)), g['imp_sdist_sha256'])
    sf, aux = rend.sample_importance(sdist, T(g['imp_weights']), S, u=T(inp['u_fine']), return_aux=True)
    np.testing.assert_array_equal(aux['inds'].cpu().numpy().reshape(-1).astype(np.int64), g['inds'].reshape(-1).astype(np.int64))
    np.testing.assert_array_equal(sha256(N(sf)), g['imp_sdist_fine_sha256'])
    # through the whole chain: the HIP planes, the HIP coarse densities
    syn = G.synthesis
    planes = syn.tri_plane_decoder(ws, noise_mode='const', hwc=True)
    c2w = tdgp.renderer.compute_cam2world_matrix(cam)
    ro, rd = tdgp.renderer.sample_rays(c2w, fov=cam['fov'], resolution=(syn.test_resolution,) * 2, device=DEV)
    opts = syn.rendering_options(syn._default_render_options)
    opts.update(u_coarse=T(inp['u_coarse']), u_fine=T(inp['u_fine']))
    _, inter = rend(planes, syn.tri_plane_mlp, ro, rd, opts, return_intermediates=True)
    hi = inter['inds'].cpu().numpy().reshape(B * R, -1).astype(np.int64)
    ref_inds = g['inds'].reshape(hi.shape).astype(np.int64)
    ni = int((hi != ref_inds).sum())
    npm = int((inter['perm'].cpu().numpy().reshape(-1) != g['perm'].reshape(-1)).sum())
    report_parity('e2e_long integer rows through the whole chain', inds_mismatches=ni, inds_total=int(hi.size), perm_mismatches=npm,
                  perm_total=int(g['perm'].size))
    _, raux = oracle.sample_importance(N(sdist), g['imp_weights'], inp['u_fine'], cfg.ray_marcher_type, return_aux=True)
    np.testing.assert_array_equal(np.asarray(raux['inds']).reshape(hi.shape), ref_inds)
    rg = inter['rgbs_coarse'].reshape(B, R, S, 4)
    _, _, w, _ = rend.ray_marcher(rg[..., :3].contiguous(), rg[..., 3:4].contiguous(), inter['sdist_coarse'].reshape(B, R, S, 1), opts)
    _, haux = rend.sample_importance(inter['sdist_coarse'].reshape(B, R, S, 1), w, S, u=T(inp['u_fine']), return_aux=True)
    assert torch.equal(haux['inds'].reshape(-1), inter['inds'].reshape(-1)), 'op-level importance stage != fused kernel'
    assert_inds_mismatches_in_window(hi, ref_inds, inp['u_fine'].reshape(hi.shape), np.asarray(raux['cdf']).reshape(hi.shape[0], -1),
                                     N(haux['cdf']).reshape(hi.shape[0], -1), what='e2e_long vs the reference')
    assert ni <= 4, ni
    # the merged order: a fine sample whose draw flipped across a knot, or whose cdf knots differ by an ulp, moves by < 1e-6 and may trade
    # places with a neighbour that close.  Every mismatching slot of `perm` must lie in a run of slots holding the same samples on both
    # sides, whose depths (HIP) are within 5e-6 of each other (assert_inds_mismatches_in_window's output-continuity bound).
    BR, M = B * R, 2 * S
    sf = N(inter['sdist_fine']).reshape(BR, S)
    tn, tf = np.float32(cfg.ray_start), np.float32(cfg.ray_end)
    t_cat = np.concatenate([N(inter['tdist_coarse']).reshape(BR, S), sf * tf + (np.float32(1) - sf) * tn], 1)
    hp, rp = inter['perm'].cpu().numpy().reshape(BR, M).astype(np.int64), g['perm'].reshape(BR, M).astype(np.int64)
    spread = 0.0
    for r in np.nonzero((hp != rp).any(1))[0]:
        cols = np.nonzero(hp[r] != rp[r])[0]
        runs = np.split(cols, np.nonzero(np.diff(cols) > 1)[0] + 1)
        for run in runs:
            sl = slice(run[0], run[-1] + 1)
            assert sorted(hp[r, sl]) == sorted(rp[r, sl]), f'perm row {r} slots {run}: not a reordering of the same samples'
            spread = max(spread, float(np.ptp(t_cat[r, hp[r, sl]])))
    report_parity('e2e_long merged-order mismatches, widest depth spread of a reordered run', perm_mismatches=npm, spread=spread)
    assert spread <= 5e-6, spread


@gpu
def test_forward_split_at_field_bound_equals_images_one_at_a_time(native):
    """16 images of 256^2 rays x 512 samples = 2^29 points per field pass: one more than tdgp_triplane_field takes (B * P <= INT32_MAX / 4).
    The eval forward splits the render by images; the result equals each image rendered on its own, bit for bit.  Then an image too large
    for one call (the bound lowered to a few image rows) takes the split by runs of whole rows, again bit for bit."""
    tdgp = native
    cfg = tdgp.config.config_tiny()
    G = _gen(tdgp, cfg, 5)
    tdgp.inference.configure_for_inference(G, 256, 64)              # 8 x 64 = 512 + 512 samples per ray
    syn = G.synthesis
    B, R, S = 16, 256 * 256, 512
    assert B * R * S > tdgp.generator.FIELD_POINTS_MAX
    inp = tdgp.weights.synthetic_inputs(cfg, batch=B, seed=6)
    gen = torch.Generator(device=DEV).manual_seed(6)
    u1 = torch.rand([B, R, S], device=DEV, generator=gen)
    u2 = torch.rand([B * R, S], device=DEV, generator=gen)
    cam = {k: T(v) for k, v in inp['camera'].items()}
    ws = G.mapping(T(inp['z']), T(inp['c']))
    out = syn(ws, camera_params=cam, noise_mode='const', render_opts=dict(return_depth=True), u_coarse=u1, u_fine=u2)
    planes = syn.tri_plane_decoder(ws, noise_mode='const', hwc=True)
    c2w = tdgp.renderer.compute_cam2world_matrix(cam)
    ro, rd = tdgp.renderer.sample_rays(c2w, fov=cam['fov'], resolution=(256, 256), device=DEV)
    opts = syn.rendering_options(syn._default_render_options)
    for b in range(B):
        o = dict(opts, u_coarse=u1[b:b + 1], u_fine=u2[b * R:(b + 1) * R], ray_grid_w=256)
        rgb, depth, _, _ = syn.renderer(tdgp.renderer.HWCPlanes(planes.t[b:b + 1]), syn.tri_plane_mlp, ro[b:b + 1], rd[b:b + 1], o)
        assert torch.equal(out.img[b], rgb.reshape(256, 256, 3).permute(2, 0, 1)), b
        assert torch.equal(out.depth[b].reshape(-1), depth.reshape(-1)), b
    del out, u1, u2
    torch.cuda.empty_cache()
    # one image too large for a call: the bound lowered to 6 rows of a 64^2 image -> runs of 4 whole rows (whole 4x4-pixel tile strips)
    syn.img_resolution = syn.test_resolution = 64
    Rs = 64 * 64
    u1 = torch.rand([2, Rs, S], device=DEV, generator=gen)
    u2 = torch.rand([2 * Rs, S], device=DEV, generator=gen)
    cam2 = {k: v[:2] for k, v in cam.items()}
    whole = syn(ws[:2], camera_params=cam2, noise_mode='const', render_opts=dict(return_depth=True), u_coarse=u1, u_fine=u2)
    bound = tdgp.generator.FIELD_POINTS_MAX
    try:
        tdgp.generator.FIELD_POINTS_MAX = 6 * 64 * S
        split = syn(ws[:2], camera_params=cam2, noise_mode='const', render_opts=dict(return_depth=True), u_coarse=u1, u_fine=u2)
    finally:
        tdgp.generator.FIELD_POINTS_MAX = bound
    assert torch.equal(whole.img, split.img) and torch.equal(whole.depth, split.depth)


@gpu
def test_graphed_generator_after_configure_for_inference(native):
    """A GraphedGenerator captured after configure_for_inference renders what G.synthesis renders: its rays and draws are sized from the
    resolution the forward renders at, not from cfg.img_resolution."""
    tdgp = native
    cfg = tdgp.config.config_tiny()
    G = _gen(tdgp, cfg, 9)
    tdgp.inference.configure_for_inference(G, 24, 40)               # 24^2 image, 320 + 320 samples per ray
    gg = importlib.import_module('3dgp_amd.graphs').GraphedGenerator(G, batch=2, explicit_draws=True)
    assert tuple(gg.u_coarse.shape) == (2, 24 * 24, 320) and tuple(gg.u_fine.shape) == (2 * 24 * 24, 320)
    inp = tdgp.weights.synthetic_inputs(cfg, batch=2, seed=10)
    rs = np.random.RandomState(10)
    u1, u2 = T(rs.rand(2, 576, 320)), T(rs.rand(2 * 576, 320))
    cam = {k: T(v) for k, v in inp['camera'].items()}
    img = gg(T(inp['z']), T(inp['c']), cam, u1, u2)
    ref = G(T(inp['z']), T(inp['c']), cam, noise_mode='const', u_coarse=u1, u_fine=u2)
    torch.cuda.synchronize()
    assert img.shape == (2, 3, 24, 24) and torch.equal(img, ref)

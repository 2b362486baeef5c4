"""Perceptual path length on the GPU: tdgp_pair_sqdist and tdgp_ppl_frames against numpy / torch-CPU restatements of their contracts
(include/tdgp.h), the sampler on the tiny generator (identical endpoints -> exactly 0; ordinary pairs against a restatement through the
public pieces), aggregate_ppl on the device against the host value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEG = 16384                                               # elements of a row per block (csrc/pair_dist.hip PD_SEG)
EPS2 = 1.0 / (1e-4 * 1e-4)


def _sqdist(tdgp, feats, inv_scale=EPS2):
    return tdgp.metrics.pair_sqdist(torch.from_numpy(feats).cuda(), inv_scale).cpu().numpy()


def _sqdist_f64(feats, inv_scale=EPS2, round_difference=True):
    n = feats.shape[0] // 2
    d = (feats[:n] - feats[n:]).astype(np.float64) if round_difference else feats[:n].astype(np.float64) - feats[n:].astype(np.float64)
    return (d * d).sum(axis=1) * inv_scale


# the first width at which a row is split over two blocks is SEG + 1; 2 * SEG + 5 spans three
@pytest.mark.parametrize('W', [1, 3, 63, 64, 65, 4096 + 17, SEG, SEG + 1, SEG + 2, 2 * SEG + 5])
def test_pair_sqdist_integer_lattice_bit_exact(tdgp, W):
    """Small integers stored as fp32: every difference, product and partial sum is exact in fp64, so any summation order gives the same bits."""
    for n in (1, 2, 3):
        rs = np.random.RandomState(W + n)
        feats = rs.randint(-4, 5, size=(2 * n, W)).astype(np.float32)
        got = _sqdist(tdgp, feats)
        want = _sqdist_f64(feats).astype(np.float32)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (n, W, got, want)


@pytest.mark.parametrize('W', [4096 + 17, SEG + 1, 2 * SEG + 5])
def test_pair_sqdist_gaussian_rows(tdgp, W):
    """Within 2^-23 relative of the float64 value of sum((a - b)^2) / eps^2: one fp32 rounding of each difference, one of the result."""
    rs = np.random.RandomState(W)
    feats = rs.randn(6, W).astype(np.float32)
    got = _sqdist(tdgp, feats).astype(np.float64)
    want = _sqdist_f64(feats, round_difference=False)
    err = np.abs(got - want) / want
    print(f'pair_sqdist W={W}: max relative error {err.max():.3e} (bound {2.0 ** -23:.3e})')
    assert err.max() <= 2.0 ** -23
    # against the contract itself (difference rounded to fp32, then fp64): only the last rounding and the order of the fp64 additions
    assert (np.abs(got - _sqdist_f64(feats)) / want).max() <= 2.0 ** -24 * (1 + 1e-6)


def test_pair_sqdist_writes_its_rows_only(tdgp):
    M = tdgp.metrics
    rs = np.random.RandomState(1)
    W = SEG + 3
    feats = torch.from_numpy(rs.randn(6, W).astype(np.float32)).cuda()
    want = M.pair_sqdist(feats, EPS2)
    buf = torch.full([11], -7.0, device='cuda')
    M.pair_sqdist(feats, EPS2, out=buf[5:8])                    # a non-zero, only 4-byte aligned offset into a larger buffer
    assert torch.equal(buf[5:8], want) and float(buf[:5].max()) == float(buf[:5].min()) == -7.0 and float(buf[8:].max()) == float(buf[8:].min()) == -7.0
    # n = 0 is a no-op
    L = tdgp._lib
    assert L.load().tdgp_pair_sqdist_workspace_bytes(0, W) >= 0
    L.call('tdgp_pair_sqdist', feats.data_ptr(), 0, W, EPS2, buf.data_ptr(), None, 0, L.stream_of(buf))
    assert M.pair_sqdist(feats[:0], EPS2).shape == (0,)
    torch.cuda.synchronize()
    assert float(buf[:5].max()) == -7.0 and torch.equal(buf[5:8], want)


def test_pair_sqdist_nan_stays_in_its_row(tdgp):
    rs = np.random.RandomState(2)
    W = 2 * SEG + 5
    feats = rs.randn(6, W).astype(np.float32)
    clean = _sqdist(tdgp, feats)
    feats[4, SEG + 77] = np.nan                               # the second row of pair 1, in its second segment
    got = _sqdist(tdgp, feats)
    assert np.isnan(got[1]) and got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()
    feats[4, SEG + 77] = np.inf
    assert np.isinf(_sqdist(tdgp, feats)[1])


@pytest.mark.parametrize('W', [65, 4096 + 17, SEG + 1, 2 * SEG + 5])
def test_pair_sqdist_row_bits_do_not_depend_on_the_call(tdgp, W):
    """An odd W puts the rows of a call of 3 at other alignments than the same rows in calls of 1: the bits must not move."""
    rs = np.random.RandomState(W)
    feats = rs.randn(6, W).astype(np.float32)
    three = _sqdist(tdgp, feats)
    for i in range(3):
        one = _sqdist(tdgp, np.stack([feats[i], feats[3 + i]]))
        assert one.tobytes() == three[i:i + 1].tobytes(), (W, i)
    assert _sqdist(tdgp, feats).tobytes() == three.tobytes()   # and the same bytes on a second run


def test_pair_sqdist_refusals(tdgp):
    L = tdgp._lib
    lib = L.load()
    assert lib.tdgp_pair_sqdist_workspace_bytes(3, 0) == -1 and lib.tdgp_pair_sqdist_workspace_bytes(-1, 8) == -1
    assert lib.tdgp_pair_sqdist_workspace_bytes(65536, 8) == -1 and lib.tdgp_pair_sqdist_workspace_bytes(1, 1 << 31) == -1
    assert lib.tdgp_pair_sqdist_workspace_bytes(3, SEG) == 0 and lib.tdgp_pair_sqdist_workspace_bytes(3, SEG + 1) == 48
    x = torch.zeros([4, SEG + 1], device='cuda')
    out = torch.zeros([2], device='cuda')
    ws = torch.zeros([64], dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='failed \\(-1\\)'):
        L.call('tdgp_pair_sqdist', x.data_ptr(), 2, 0, 1.0, out.data_ptr(), ws.data_ptr(), 64, L.stream_of(x))
    with pytest.raises(L.Unsupported):
        L.call('tdgp_pair_sqdist', x.data_ptr(), 65536, 8, 1.0, out.data_ptr(), ws.data_ptr(), 64, L.stream_of(x))
    with pytest.raises(RuntimeError, match='workspace too small'):
        L.call('tdgp_pair_sqdist', x.data_ptr(), 2, SEG + 1, 1.0, out.data_ptr(), ws.data_ptr(), 16, L.stream_of(x))


# ------------------------------------------------------------------------------------------------ tdgp_ppl_frames
def _frames(seed, B, h, w, C):
    return (np.random.RandomState(seed).rand(B, h * w, C).astype(np.float32) * 2.4 - 1.2)


def _chw(frames, h, w):
    B, _, C = frames.shape
    return np.ascontiguousarray(frames.reshape(B, h, w, C).transpose(0, 3, 1, 2))


@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('crop', [False, True])
def test_ppl_frames_factor_1_is_the_torch_cpu_chain(tdgp, C, crop):
    h = w = 16
    fr = _frames(10 + C, 3, h, w, C)
    got = tdgp.renderer.ppl_frames(torch.from_numpy(fr).cuda(), h, w, crop=crop, factor=1).cpu()
    want = tdgp.metrics.ppl_image_tail(torch.from_numpy(_chw(fr, h, w)), crop, 1)
    assert got.shape == want.shape == ((3, 3, 8, 8) if crop else (3, 3, 16, 16))
    assert torch.equal(got, want)


def _tail_numpy(fr, h, w, crop, factor):
    """The contract of tdgp_ppl_frames: fp64 box sum in row-major order, / factor^2 in fp64, one rounding; (x + 1) * 127.5 in two fp32 roundings."""
    x = _chw(fr, h, w)
    if crop:
        c = h // 8
        x = x[:, :, 3 * c:7 * c, 2 * c:6 * c]
    s = np.zeros(x.shape[:2] + (x.shape[2] // factor, x.shape[3] // factor), np.float64)
    for dy in range(factor):
        for dx in range(factor):
            s = s + x[:, :, dy::factor, dx::factor].astype(np.float64)
    m = (s / np.float64(factor * factor)).astype(np.float32)
    y = (m + np.float32(1.0)) * np.float32(127.5)
    assert y.dtype == np.float32
    return np.repeat(y, 3, axis=1) if y.shape[1] == 1 else y


@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('crop', [False, True])
@pytest.mark.parametrize('factor', [2, 3])
def test_ppl_frames_box_mean(tdgp, factor, crop, C):
    h = w = 24
    fr = _frames(20 + factor, 2, h, w, C)
    got = tdgp.renderer.ppl_frames(torch.from_numpy(fr).cuda(), h, w, crop=crop, factor=factor).cpu()
    want = _tail_numpy(fr, h, w, crop, factor)
    side = (12 if crop else 24) // factor
    assert got.shape == (2, 3, side, side)
    assert got.numpy().tobytes() == want.tobytes()
    # torch's fp32 `mean` is within factor^2 * 2^-24 * max|x| of the exact mean (factor^2 - 1 fp32 additions and one division); carried
    # through y = (m + 1) * 127.5 that is 127.5 times as much, plus the two roundings of either side's own chain (each <= 2^-24 of |y| <= max|y|)
    ref = tdgp.metrics.ppl_image_tail(torch.from_numpy(_chw(fr, h, w)), crop, factor)
    tol = 127.5 * factor ** 2 * 2.0 ** -24 * float(np.abs(fr).max()) + 4 * 2.0 ** -24 * float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f'ppl_frames factor={factor} crop={crop} C={C}: max |kernel - torch fp32 chain| = {err:.3e} (bound {tol:.3e})')
    assert err <= tol


def test_ppl_frames_refuses_bad_shapes_before_launch(tdgp):
    R = tdgp.renderer
    fr = torch.zeros([2, 24 * 16, 3], device='cuda')
    with pytest.raises(RuntimeError, match='square'):
        R.ppl_frames(fr, 24, 16, crop=True)
    with pytest.raises(RuntimeError, match='divide'):
        R.ppl_frames(fr, 24, 16, factor=5)
    with pytest.raises(RuntimeError, match='factor'):
        R.ppl_frames(fr, 24, 16, factor=0)
    with pytest.raises(RuntimeError, match='C must be 1 or 3'):
        R.ppl_frames(torch.zeros([2, 16, 2], device='cuda'), 4, 4)
    with pytest.raises(RuntimeError, match='empty'):
        R.ppl_frames(torch.zeros([2, 16, 3], device='cuda'), 4, 4, crop=True)
    with pytest.raises(ValueError):
        R.ppl_frames(fr, 16, 16)
    assert R.ppl_frames(fr[:0], 24, 16).shape == (0, 3, 24, 16)               # no frames: a no-op
    torch.cuda.synchronize()
    assert tdgp._lib.device_fault() == 0


# ------------------------------------------------------------------------------------------------ the sampler on the tiny generator
@pytest.fixture(scope='module')
def tiny(tdgp):
    cfg = tdgp.config.config_tiny()                                           # 16 x 16 rays, 8 + 8 samples
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=41, exercise_all=True))
    G = G.cuda().eval()
    proj = torch.from_numpy(np.random.RandomState(42).randn(3 * 16 * 16, 37).astype(np.float32) / 64).cuda()
    return G, (lambda img: img.flatten(1) @ proj)


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def test_sampler_identical_endpoints_give_exactly_zero(tdgp, tiny):
    G, detector = tiny

    class Same(tdgp.metrics.PPLSampler):
        def draw_latents(self, batch, device):
            z0, _ = super().draw_latents(batch, device)
            return z0, z0.clone()
    sampler = Same(G, detector, 0.0, 'w', 'end', crop=False).eval().requires_grad_(False)
    _seed(1)
    c = torch.zeros([3, 0], device='cuda')
    dist = sampler(c)
    assert dist.shape == (3,) and torch.equal(dist.cpu(), torch.zeros(3))
    # the images behind those zeros are real ones: finite, not constant
    img = sampler.endpoint_images(sampler.draw(c))
    assert img.shape == (6, 3, 16, 16) and bool(torch.isfinite(img).all()) and float(img.std()) > 0
    assert torch.equal(img[:3], img[3:])


@pytest.mark.parametrize('space,sampling', [('w', 'end'), ('z', 'full')])
def test_sampler_against_the_public_pieces(tdgp, tiny, space, sampling):
    """The sampler's distances against: the same ws, cameras and draws through G.synthesis at the same batch size, the torch tail, the detector
    on the same 2B images and (l0 - l1)^2 .sum / eps^2 in float64 -- within 2^-22 relative."""
    G, detector = tiny
    M = tdgp.metrics
    eps, B = 1e-4, 2
    before = {k: v.clone() for k, v in G.named_buffers() if k.endswith('.noise_const')}
    sampler = M.PPLSampler(G, detector, eps, space, sampling, crop=False).eval().requires_grad_(False)
    c = torch.zeros([B, 0], device='cuda')
    _seed(7)
    dist = sampler(c).cpu().double()
    _seed(7)
    d = sampler.draw(c)                                                       # the same draws again (the noise buffers are refilled alike)
    with torch.no_grad():
        imgs = torch.cat([sampler.G.synthesis(ws=ws, camera_params=d.camera_params, noise_mode='const', u_coarse=d.u_coarse, u_fine=d.u_fine)
                          for ws in (d.ws0, d.ws1)])
        l0, l1 = detector(M.ppl_image_tail(imgs, False, 1)).double().cpu().chunk(2)
    want = (l0 - l1).square().sum(1) / eps ** 2
    assert float(want.min()) > 0
    err = ((dist - want).abs() / want).max()
    print(f'sampler {space}/{sampling}: distances {dist.tolist()}, max relative error vs the restatement {float(err):.3e} (bound {2.0 ** -22:.3e})')
    assert float(err) <= 2.0 ** -22
    assert len(before) > 0 and all(torch.equal(v, dict(G.named_buffers())[k]) for k, v in before.items())      # the caller's noise is untouched


def test_compute_ppl_on_the_device(tdgp, tiny):
    G, detector = tiny
    M = tdgp.metrics
    values = []
    for _ in range(2):
        _seed(3)
        values.append(M.ppl_for_generator(G, detector, num_samples=5, batch_size=2))
    assert np.isfinite(values[0]) and values[0] > 0 and values[0] == values[1]


def test_aggregate_ppl_device_equals_host(tdgp):
    M = tdgp.metrics
    rs = np.random.RandomState(5)
    d = (rs.rand(5000).astype(np.float32) ** 3) * 1e4
    d[rs.randint(0, 5000, 40)] = d[7]                                         # ties
    d[:60] = np.sort(d)[49]                                                   # ties at lo (k_lo = 49)
    d[60:130] = np.sort(d)[4950]                                              # and at hi (k_hi = 4950)
    x = torch.from_numpy(d).cuda()
    k_lo, k_hi = M.ppl_ranks(d.size)
    ordered = np.sort(d)
    for k in (k_lo, k_hi):
        assert M._order_statistic(x, k).cpu().numpy().tobytes() == ordered[k].tobytes()
    host, dev = M.aggregate_ppl(d), M.aggregate_ppl(x)
    assert abs(dev - host) <= 1e-12 * abs(host)
    for n in (1, 2, 3):
        assert abs(M.aggregate_ppl(x[:n]) - M.aggregate_ppl(d[:n])) <= 1e-12 * abs(M.aggregate_ppl(d[:n]))

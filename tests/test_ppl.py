"""Perceptual path length on the CPU (3dgp_amd/metrics.py: slerp, ppl_ranks, aggregate_ppl, PPLSampler, compute_ppl): the aggregation against
numpy's percentile arithmetic, the sampler's logic on a stand-in generator made of plain torch modules that record what they are given."""
import types

import numpy as np
import pytest
import torch


def _percentile(a, q, how):
    try:
        return np.percentile(a, q, method=how)
    except TypeError:                                       # numpy < 1.22 spells the keyword `interpolation`
        return np.percentile(a, q, interpolation=how)


def _reference_ppl(dist):
    """perceptual_path_length.py:120-122 with the mean taken in float64."""
    dist = np.asarray(dist, np.float32)
    lo, hi = _percentile(dist, 1, 'lower'), _percentile(dist, 99, 'higher')
    return float(np.extract(np.logical_and(dist >= lo, dist <= hi), dist).astype(np.float64).mean())


def test_ppl_ranks_are_numpys_percentile_indices(tdgp):
    for n in range(1, 401):
        a = np.arange(n, dtype=np.float32)
        k_lo, k_hi = tdgp.metrics.ppl_ranks(n)
        assert 0 <= k_lo <= k_hi < n
        assert a[k_lo] == _percentile(a, 1, 'lower') and a[k_hi] == _percentile(a, 99, 'higher'), n


@pytest.mark.parametrize('n', [1, 2, 3, 100, 101, 257, 5000])
def test_aggregate_ppl_is_the_reference_expression(tdgp, n):
    rs = np.random.RandomState(n)
    d = (rs.rand(n).astype(np.float32) ** 2) * 1e3
    assert tdgp.metrics.aggregate_ppl(torch.from_numpy(d)) == _reference_ppl(d)
    assert tdgp.metrics.aggregate_ppl(d) == _reference_ppl(d)


def test_aggregate_ppl_keeps_ties_at_both_ends(tdgp):
    rs = np.random.RandomState(7)
    d = rs.rand(300).astype(np.float32) + 1.0
    d[:5] = 0.25                       # five copies of the minimum: k_lo = 2 falls among them, all five stay
    d[5:11] = 9.0                      # six copies of the maximum around k_hi = 297
    d = d[rs.permutation(300)]
    got = tdgp.metrics.aggregate_ppl(torch.from_numpy(d))
    assert got == _reference_ppl(d) == float(d.astype(np.float64).mean())
    d[17] = 0.125                      # one value below lo and one above hi are dropped, the ties stay
    d[18] = 10.0
    got = tdgp.metrics.aggregate_ppl(torch.from_numpy(d))
    keep = np.delete(d, [17, 18])
    assert got == _reference_ppl(d) == float(keep.astype(np.float64).mean())
    assert np.isnan(tdgp.metrics.aggregate_ppl(np.array([1.0, np.nan, 2.0], np.float32)))


def test_slerp_against_float64(tdgp):
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(6, 32, generator=g), torch.randn(6, 32, generator=g)
    t = torch.rand(6, 1, generator=g)
    got = tdgp.metrics.slerp(a, b, t)
    a64, b64, t64 = a.double(), b.double(), t.double()
    an, bn = a64 / a64.norm(dim=-1, keepdim=True), b64 / b64.norm(dim=-1, keepdim=True)
    omega = torch.acos((an * bn).sum(-1, keepdim=True))
    want = (torch.sin((1 - t64) * omega) * an + torch.sin(t64 * omega) * bn) / torch.sin(omega)      # the textbook form of the same point
    assert float((got.double() - want).abs().max()) < 1e-6
    assert float((got.norm(dim=-1) - 1).abs().max()) < 1e-6
    at0 = tdgp.metrics.slerp(a, b, torch.zeros(6, 1))
    assert float((at0 - a / a.norm(dim=-1, keepdim=True)).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ the sampler on a stand-in generator
RES, STEPS, ZD, NUM_WS = 8, 3, 5, 4


class _Mapping(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(ZD, ZD)
        self.calls = []

    def forward(self, z, c):
        self.calls.append((z.clone(), c.clone()))
        return self.lin(z).unsqueeze(1).repeat(1, NUM_WS, 1)


class _Layer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer('noise_const', torch.randn(RES, RES))


class _Synthesis(torch.nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.channels = channels
        self.cfg = types.SimpleNamespace(num_ray_steps=STEPS)
        self.test_resolution = RES
        self.b4, self.b8 = _Layer(), _Layer()
        self.calls = []

    def forward(self, ws, camera_params, noise_mode, u_coarse, u_fine, **kw):
        self.calls.append(dict(ws=ws.clone(), camera=camera_params, noise_mode=noise_mode, u_coarse=u_coarse.clone(), u_fine=u_fine.clone(), kw=kw,
                               noise=[self.b4.noise_const.clone(), self.b8.noise_const.clone()]))
        B = ws.shape[0]
        base = ws.mean(dim=1)[:, :3].reshape(B, 3, 1, 1) + camera_params.angles[:, 0].reshape(B, 1, 1, 1)
        jitter = u_coarse.reshape(B, RES, RES, -1).mean(dim=3) + u_fine.reshape(B, RES, RES, -1).mean(dim=3)
        return torch.tanh(base + 0.1 * jitter.unsqueeze(1) + 0.01 * (self.b4.noise_const + self.b8.noise_const))[:, :self.channels]


class _Generator(torch.nn.Module):
    def __init__(self, channels=3):
        super().__init__()
        self.z_dim, self.c_dim, self.img_resolution, self.img_channels = ZD, 0, RES, channels
        self.mapping, self.synthesis = _Mapping(), _Synthesis(channels)


def _detector(img):
    g = torch.Generator().manual_seed(11)
    return img.flatten(1) @ torch.randn(img[0].numel(), 7, generator=g)


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def test_sampler_end_sampling_shared_camera_and_draws(tdgp):
    M = tdgp.metrics
    torch.manual_seed(0)
    G = _Generator()
    before = {k: v.clone() for k, v in G.named_buffers()}
    eps, B = 1e-2, 3
    sampler = M.PPLSampler(G, _detector, eps, 'w', 'end', crop=False, G_kwargs=dict(flag=5))
    _seed(5)
    c = torch.zeros([B, 0])
    d = sampler.draw(c)
    assert torch.equal(d.t, torch.zeros(B))                                    # sampling='end'
    (z, cc), = sampler.G.mapping.calls
    assert z.shape == (2 * B, ZD) and cc.shape == (2 * B, 0)
    w0, w1 = sampler.G.mapping.lin(z).unsqueeze(1).repeat(1, NUM_WS, 1).chunk(2)
    assert torch.equal(d.ws0, w0) and torch.equal(d.ws1, w0.lerp(w1, torch.full([B, 1, 1], eps)))
    assert not torch.equal(d.ws0, d.ws1)
    assert d.u_coarse.shape == (B, RES * RES, STEPS) and d.u_fine.shape == (B, RES * RES, STEPS)
    for k in ('angles', 'fov', 'radius', 'look_at'):
        assert d.camera_params[k].shape[0] == B

    # the RNG call order of one call under a fixed seed: t, z, noise buffers in named_buffers() order, camera, u_coarse, u_fine
    _seed(5)
    t = torch.rand([B])
    zz = torch.randn([2 * B, ZD])
    noise = [torch.randn(RES, RES), torch.randn(RES, RES)]
    cam = M.sample_camera_params(M.camera_base(), B, 'cpu')
    uc, uf = torch.rand([B, RES * RES, STEPS, 1]), torch.rand([B * RES * RES, STEPS])
    assert t.shape == d.t.shape and torch.equal(zz, z)
    names = [k for k, _ in sampler.G.named_buffers() if k.endswith('.noise_const')]
    assert names == ['synthesis.b4.noise_const', 'synthesis.b8.noise_const']
    assert all(torch.equal(a, dict(sampler.G.named_buffers())[k]) for a, k in zip(noise, names))
    assert all(torch.equal(cam[k], d.camera_params[k]) for k in ('angles', 'fov', 'radius', 'look_at'))
    assert torch.equal(uc.reshape(B, RES * RES, STEPS), d.u_coarse) and torch.equal(uf.reshape(B, RES * RES, STEPS), d.u_fine)

    # the two endpoints of every pair are rendered with the same camera rows and the same draws, as two calls of B images
    _seed(5)
    dist = sampler(c)
    first, second = sampler.G.synthesis.calls
    assert first['ws'].shape[0] == second['ws'].shape[0] == B
    assert torch.equal(first['ws'], d.ws0) and torch.equal(second['ws'], d.ws1)
    assert first['camera'] is second['camera'] and torch.equal(first['camera'].angles, d.camera_params.angles)
    assert torch.equal(first['u_coarse'], second['u_coarse']) and torch.equal(first['u_fine'], second['u_fine'])
    assert torch.equal(first['u_coarse'], d.u_coarse) and torch.equal(first['u_fine'], d.u_fine)
    assert first['noise_mode'] == second['noise_mode'] == 'const' and first['kw'] == second['kw'] == dict(flag=5)
    assert all(torch.equal(a, b) for a, b in zip(first['noise'], second['noise']))
    # the distance is the float64 differential quotient of the detector rows
    imgs = torch.cat([sampler.G.synthesis(ws=ws, camera_params=d.camera_params, noise_mode='const', u_coarse=d.u_coarse, u_fine=d.u_fine)
                      for ws in (d.ws0, d.ws1)])
    l0, l1 = _detector((imgs + 1) * 127.5).double().chunk(2)
    want = ((l0 - l1).square().sum(1) / eps ** 2).detach()
    assert dist.shape == (B,) and dist.dtype == torch.float32
    assert float(((dist.double() - want).abs() / want).max()) < 1e-3           # (the fp32 rounding of l0 - l1 next to cancellation)
    assert float(dist.min()) > 0
    # the caller's generator is untouched
    assert G.mapping.calls == [] and G.synthesis.calls == []
    assert all(torch.equal(v, before[k]) for k, v in G.named_buffers())


def test_sampler_full_sampling_z_space_crop_and_grey(tdgp):
    M = tdgp.metrics
    torch.manual_seed(1)
    G = _Generator(channels=1)
    seen = []

    def detector(img):
        seen.append(img)
        return _detector(img)
    eps, B = 1e-3, 4
    sampler = M.PPLSampler(G, detector, eps, 'z', 'full', crop=True, target_resolution=4)
    assert sampler.factor == 2
    _seed(9)
    d = sampler.draw(torch.zeros([B, 0]))
    assert float(d.t.min()) >= 0 and float(d.t.max()) < 1 and float(d.t.max()) > 0
    (z, _), = sampler.G.mapping.calls
    zt0, zt1 = z.chunk(2)
    assert float((zt0.norm(dim=-1) - 1).abs().max()) < 1e-6                   # slerp leaves unit vectors
    assert torch.equal(zt1, M.slerp(d.z0, sampler_z1(9, B), d.t.unsqueeze(1) + eps))
    _seed(9)
    dist = sampler(torch.zeros([B, 0]))
    assert dist.shape == (B,) and seen[0].shape == (2 * B, 3, 2, 2)           # crop 8 -> 4, box mean 4 -> 2, grey -> 3 channels
    assert torch.equal(seen[0][:, 0], seen[0][:, 1]) and torch.equal(seen[0][:, 0], seen[0][:, 2])
    assert float(seen[0].min()) >= 0 and float(seen[0].max()) <= 255


def sampler_z1(seed, B):
    """z1 of a call under `seed`: the second half of the sampler's one randn, drawn behind t."""
    _seed(seed)
    torch.rand([B])
    return torch.randn([2 * B, ZD]).chunk(2)[1]


def test_sampler_identical_endpoints_give_zero(tdgp):
    M = tdgp.metrics
    torch.manual_seed(2)

    class Same(M.PPLSampler):
        def draw_latents(self, batch, device):
            z0, _ = super().draw_latents(batch, device)
            return z0, z0.clone()
    sampler = Same(_Generator(), _detector, 0.0, 'w', 'end', crop=False)
    _seed(3)
    dist = sampler(torch.zeros([5, 0]))
    assert torch.equal(dist, torch.zeros(5))


def test_pair_sqdist_cpu_contract(tdgp):
    M = tdgp.metrics
    rs = np.random.RandomState(0)
    f = rs.randn(6, 1001).astype(np.float32)
    got = M.pair_sqdist(torch.from_numpy(f), 1e8)
    d = (f[:3] - f[3:]).astype(np.float64)
    want = ((d * d).sum(1) * 1e8).astype(np.float32)
    assert float(np.abs(got.numpy() / want - 1).max()) <= 2.0 ** -23
    buf = torch.full([8], -1.0)
    M.pair_sqdist(torch.from_numpy(f), 1e8, out=buf[2:5])
    assert torch.equal(buf[2:5], got) and float(buf[:2].max()) == float(buf[5:].max()) == -1.0
    with pytest.raises(ValueError):
        M.pair_sqdist(torch.zeros(3, 4), 1.0)


def test_compute_ppl_two_rank_interleave_and_truncation(tdgp, monkeypatch):
    M = tdgp.metrics
    torch.manual_seed(4)
    G = _Generator()
    captured = []
    monkeypatch.setattr(M, 'aggregate_ppl', lambda d: captured.append(d.clone()) or 0.5)
    args = dict(epsilon=1e-2, space='w', sampling='end', crop=False, batch_size=2, device='cpu')
    _seed(6)
    assert M.compute_ppl(G, _detector, num_samples=6, **args) == 0.5
    single, = captured                                       # three iterations of one rank: blocks x0, x1, x2
    assert single.shape == (6,)
    x = single.reshape(3, 2)

    class TwoRanks:
        """Rank 1's block is rank 0's + 1000; rows interleaved rank-major as `distributed.FeatureGatherer.gather` returns them."""
        calls = 0

        def gather(self, y):
            assert y.shape == (2, 1)
            TwoRanks.calls += 1
            return torch.stack([y, y + 1000], dim=1).flatten(0, 1)
    captured.clear()
    _seed(6)
    assert M.compute_ppl(G, _detector, num_samples=6, num_gpus=2, rank=0, gatherer=TwoRanks(), **args) == 0.5
    both, = captured
    assert TwoRanks.calls == 2                               # ceil(6 / (2 * 2)) iterations, one sampler call and one gather each
    want = torch.cat([x[0], x[0] + 1000, x[1], x[1] + 1000])[:6]        # every rank's block whole, in rank order; cut to num_samples
    assert torch.equal(both, want)
    _seed(6)
    assert np.isnan(M.compute_ppl(G, _detector, num_samples=6, num_gpus=2, rank=1, gatherer=TwoRanks(), **args))
    # a caller's label sampler: the cameras are then drawn by the sampler itself
    captured.clear()
    _seed(6)
    M.compute_ppl(G, _detector, num_samples=3, c_sampler=lambda b: torch.zeros([b, 0]), **args)
    assert captured[0].shape == (3,) and float(captured[0].min()) > 0


def test_entry_points_by_name(tdgp, monkeypatch):
    M = tdgp.metrics
    seen = {}

    def fake(G, detector, num_samples, epsilon, space, sampling, crop, batch_size, **kw):
        seen.update(num_samples=num_samples, epsilon=epsilon, space=space, sampling=sampling, crop=crop, batch_size=batch_size, kw=kw)
        return 1.25
    monkeypatch.setattr(M, 'compute_ppl', fake)
    G = _Generator()
    assert M.ppl2_wend(G, _detector) == dict(ppl2_wend=1.25)
    assert seen == dict(num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2, kw=dict(device=torch.device('cpu')))
    assert M.ppl_for_generator(G, _detector, num_samples=10, space='z', sampling='full', crop=True, batch_size=4, rank=0) == 1.25
    assert (seen['num_samples'], seen['space'], seen['sampling'], seen['crop'], seen['batch_size']) == (10, 'z', 'full', True, 4)

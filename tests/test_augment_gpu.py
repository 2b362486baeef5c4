"""The ADA augmentation pipe on the GPU (3dgp_amd/augment.py over csrc/augment.hip): tdgp_augment_params, tdgp_augment_geom and its adjoint,
tdgp_augment_color, the autograd pair, the random path, graph capture and the loss integration.  Reads only tests/golden/.

The bound throughout ("the reference's own noise", tests/test_field_deep_gpu.py): e_ref = max |reference fp32 - reference float64|, e_hip =
max |kernel - reference float64|, both over max(1, max |reference|); e_hip <= 2 max(e_ref, 2^-23).  Where the goldens cannot reach (per-sample
parameters) the reference is tests/augment_reference.py, which tests/test_augment.py pins to the goldens."""
import math

import numpy as np
import pytest
import torch

import augment_reference as R
from conftest import load_golden, report_parity

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()


@pytest.fixture(scope='module')
def A(tdgp):
    return tdgp.augment


def _eye(B, n):
    return torch.eye(n, device=DEV).expand(B, n, n).contiguous()


# ------------------------------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('name', list(R.CASES))
def test_goldens_forward_and_dx(A, name):
    """Every golden case and percentile: forward(..., debug_percentile=q) and its dx for the recorded dy, against the reference's float64 run."""
    pipe = A.AugmentPipe(**R.CASE_KW[name]).to(DEV)
    for q in R.PERCENTILES:
        g = R.load_case(name, q)
        x = T(g['x']).requires_grad_(True)
        y = pipe(x, R.CASES[name], debug_percentile=q)
        dx, = torch.autograd.grad(y, x, T(g['dy']))
        R.within_reference_noise(N(y), g['y64'], g['y32'], f'augment {name} q={q} y', report_parity)
        R.within_reference_noise(N(dx), g['dx64'], g['dx32'], f'augment {name} q={q} dx', report_parity)


def test_percentile_params_are_the_reference_scalars(A):
    """tdgp_augment_params under a percentile against the restatement of the reference's float64 parameter chain: the matrices are composed
    in fp64 and rounded once, so every entry is within one fp32 ulp of the largest entry of its matrix (gains, cutout: of 1)."""
    kw = dict(R.BASE, imgfilter=1, imgfilter_bands=[1, 0, 1, 1], noise=1, cutout=1)
    pipe = A.AugmentPipe(**kw).to(DEV)
    for q in R.PERCENTILES:
        for C in (3, 1):
            got = pipe.params(5, 24, 40, debug_percentile=q, num_channels=C)
            ref = R.percentile_params(kw, q, 5, 24, 40, C, torch.float64)
            for k in ('G_inv', 'C', 'gains', 'noise_sigma', 'cutout'):
                a, b = N(getattr(got, k)).astype(np.float64), getattr(ref, k).numpy()
                assert a.shape == b.shape, (k, a.shape, b.shape)
                err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
                report_parity(f'augment params q={q} C={C} {k}', err=err)
                assert err <= 2.0 ** -23, (q, C, k, err)


# ------------------------------------------------------------------------------------------------------------------------ per-sample parameters
def _extremes(B, H, W, which):
    rot = math.pi / 4
    mats = dict(identity=[[1, 0, 0], [0, 1, 0]], small=[[0.4, 0, 0], [0, 0.4, 0]], big=[[2.5, 0, 0], [0, 2.5, 0]],
                rot45=[[math.cos(rot), -math.sin(rot), 0], [math.sin(rot), math.cos(rot), 0]], shift=[[1, 0, 0.6 * W], [0, 1, 0.6 * H]],
                far=[[1, 0, 1.2 * W], [0, 1, 0]])
    G = torch.tensor([mats[k] + [[0, 0, 1]] for k in which[:B]], dtype=torch.float32)
    assert G.shape == (B, 3, 3)
    return G


PARAM_SETS = ['random', 'identity,small,rot45', 'big,shift,identity', 'shift,shift,shift', 'far,rot45,small']


@pytest.mark.parametrize('shape', [(3, 4, 24, 40), (2, 4, 17, 33)])
@pytest.mark.parametrize('which', PARAM_SETS)
def test_per_sample_parameters(A, shape, which):
    """apply() with a different transform per sample against the restatement in float64 on the CPU, output and dx.  `random`: params from a
    seeded draw of the full default list.  The hand-made extremes: identity, scale 0.4 and 2.5, a 45 degree rotation, a translation by 0.6
    of the width and height (at H = 17 the margin 0.6 H + 6 clamps at H - 1; at these widths reflect padding of W - 1 still covers the shift),
    and a translation by 1.2 of the width, where the margin clamps at W - 1 and zeros enter the frame."""
    B, C, H, W = shape
    rs = np.random.RandomState(11)
    x = rs.randn(*shape).astype(np.float32)
    dy = rs.randn(*shape).astype(np.float32)
    pipe = A.AugmentPipe(**R.BASE).to(DEV)
    if which == 'random':
        torch.manual_seed(5)
        p = pipe.params(B, H, W, num_channels=C)
        assert float((p.G_inv[0] - p.G_inv[1]).abs().max()) > 1e-3                    # the samples do differ
    else:
        Cm = torch.eye(4).repeat(B, 1, 1)
        Cm[:, :3, :] += torch.from_numpy(0.3 * rs.randn(B, 3, 4).astype(np.float32))
        p = A.AugmentParams(G_inv=_extremes(B, H, W, which.split(',')).to(DEV), C=Cm.to(DEV))
    xg = T(x).requires_grad_(True)
    y = pipe.apply(xg, p, 3)
    dx, = torch.autograd.grad(y, xg, T(dy))
    pc = R.Params(G_inv=p.G_inv.cpu(), C=p.C.cpu())
    ref = {}
    for dt in (torch.float64, torch.float32):
        xc = torch.from_numpy(x).to(dt).requires_grad_(True)
        yc = R.apply_reference(xc, pc.to(dtype=dt), 3, pipe.Hz_geom.cpu())
        dxc, = torch.autograd.grad(yc, xc, torch.from_numpy(dy).to(dt))
        ref[dt] = (yc.detach().numpy(), dxc.numpy())
    if 'far' in which:
        assert (ref[torch.float64][0][0, 3, :, -W // 8:] == 0).all()                  # zeros did enter the frame (channel 3: no colour bias)
    R.within_reference_noise(N(y), ref[torch.float64][0], ref[torch.float32][0], f'augment apply {shape} {which} y', report_parity)
    R.within_reference_noise(N(dx), ref[torch.float64][1], ref[torch.float32][1], f'augment apply {shape} {which} dx', report_parity)


def test_color_forms_noise_and_cutout(A):
    """tdgp_augment_color alone (no geometry): 3 colour channels + pass-through, the 1-channel form, noise times sigma, the cutout mask,
    and the adjoint, against the restatement in float64."""
    rs = np.random.RandomState(3)
    pipe = A.AugmentPipe().to(DEV)
    for C, ncc in ((4, 3), (3, 3), (2, 1), (1, 1)):
        B, H, W = 3, 9, 13
        x = rs.randn(B, C, H, W).astype(np.float32)
        dy = rs.randn(B, C, H, W).astype(np.float32)
        Cm = (np.eye(4)[None] + 0.4 * rs.randn(B, 4, 4)).astype(np.float32)
        cut = np.stack([[0.5, 0.5, 0.31, 0.77], [0.0, 0.0, 0.5, 0.5], [0.5, 0.5, 0.93, 0.02]]).astype(np.float32)
        sigma = np.abs(rs.randn(B)).astype(np.float32)
        p = A.AugmentParams(C=T(Cm), noise_sigma=T(sigma), cutout=T(cut))
        xg = T(x).requires_grad_(True)
        torch.manual_seed(9)
        y = pipe.apply(xg, p, ncc)
        torch.manual_seed(9)
        noise = torch.randn(x.shape, device=DEV).cpu()
        dx, = torch.autograd.grad(y, xg, T(dy))
        ref = {}
        for dt in (torch.float64, torch.float32):
            xc = torch.from_numpy(x).to(dt).requires_grad_(True)
            yc = R.apply_reference(xc, R.Params(C=torch.from_numpy(Cm), noise_sigma=torch.from_numpy(sigma), cutout=torch.from_numpy(cut)).to(dtype=dt), ncc,
                                   None, noise=noise)
            dxc, = torch.autograd.grad(yc, xc, torch.from_numpy(dy).to(dt))
            ref[dt] = (yc.detach().numpy(), dxc.numpy())
        assert (ref[torch.float64][0] == 0).any()                                      # the mask cut something
        R.within_reference_noise(N(y), ref[torch.float64][0], ref[torch.float32][0], f'augment color C={C} ncc={ncc} y', report_parity)
        R.within_reference_noise(N(dx), ref[torch.float64][1], ref[torch.float32][1], f'augment color C={C} ncc={ncc} dx', report_parity)


# ------------------------------------------------------------------------------------------------------------------------ second order, determinism
def _seeded_case(A, B=2, C=4, H=24, W=40):
    pipe = A.AugmentPipe(**dict(R.BASE, cutout=1)).to(DEV)
    torch.manual_seed(21)
    p = pipe.params(B, H, W, num_channels=C)
    g = torch.Generator(device='cpu').manual_seed(22)
    mk = lambda: torch.randn(B, C, H, W, generator=g).to(DEV)                          # noqa: E731
    return pipe, p, mk


def test_second_order_is_the_forward_again(A):
    pipe, p, mk = _seeded_case(A)
    x, dy, v = mk().requires_grad_(True), mk().requires_grad_(True), mk()
    y = pipe.apply(x, p, 3)
    g, = torch.autograd.grad((y * dy).sum(), x, create_graph=True)
    h, = torch.autograd.grad((g * v).sum(), dy)
    # <g, v> = <A^T dy, v> = <dy, A v>: its gradient in dy is A v, the linear part of apply (no colour bias)
    lin = pipe.apply(v, p, 3) - pipe.apply(torch.zeros_like(v), p, 3)                  # reference value, to rounding
    assert float((h - lin).abs().max()) <= 1e-4 * float(lin.abs().max())
    Av = A._Color.apply(A._Geom.apply(v, p.G_inv, pipe.Hz_geom), p.C, False, False, None, None, p.cutout, 3)
    assert torch.equal(h, Av)                                                          # byte for byte


def test_r1_shape_double_backward(A):
    """grad(||A^T w||^2, w) = 2 A (A^T w), composed from explicit calls, byte for byte."""
    pipe, p, mk = _seeded_case(A)
    x, w = mk().requires_grad_(True), mk().requires_grad_(True)
    y = pipe.apply(x, p, 3)
    g, = torch.autograd.grad((y * w).sum(), x, create_graph=True)                      # A^T w
    r, = torch.autograd.grad(g.square().sum(), w)
    with torch.no_grad():
        Atw = A._GeomAdj.apply(A._Color.apply(w, p.C, True, False, None, None, p.cutout, 3), p.G_inv, pipe.Hz_geom)
        assert torch.equal(g.detach(), Atw)
        want = A._Color.apply(A._Geom.apply(2 * Atw, p.G_inv, pipe.Hz_geom), p.C, False, False, None, None, p.cutout, 3)
    assert torch.equal(r, want)


def test_adjoint_is_deterministic_and_adjoint(A):
    pipe, p, mk = _seeded_case(A, B=3, C=5, H=33, W=17)
    dy, x = mk(), mk()
    a = A._GeomAdj.apply(dy, p.G_inv, pipe.Hz_geom)
    b = A._GeomAdj.apply(dy.clone(), p.G_inv, pipe.Hz_geom)
    assert torch.equal(a, b)
    # <A x, dy> = <x, A^T dy> in float64 sums of the fp32 results: the two kernels are the same operator
    lhs = float((A._Geom.apply(x, p.G_inv, pipe.Hz_geom).double() * dy.double()).sum())
    rhs = float((x.double() * a.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), float(x.double().norm() * a.double().norm()) * 1e-2)


# ------------------------------------------------------------------------------------------------------------------------ random path
def test_random_path_seed_and_p_zero(A):
    pipe = A.AugmentPipe(**dict(R.BASE, noise=1, cutout=1)).to(DEV)
    x = T(np.random.RandomState(1).randn(4, 4, 24, 40))
    torch.manual_seed(77)
    a = pipe(x, 3)
    torch.manual_seed(77)
    b = pipe(x, 3)
    assert torch.equal(a, b)
    assert not torch.equal(a, pipe(x, 3))
    # p = 0: every matrix is the identity -- and the chain still runs (the reference's `G_inv is not I_3` is true whenever a multiplier is set)
    pipe = A.AugmentPipe(**R.BASE).to(DEV)
    pipe.p.fill_(0.0)
    p = pipe.params(4, 24, 40, num_channels=4)
    assert torch.equal(p.G_inv, _eye(4, 3)) and torch.equal(p.C, _eye(4, 4))
    assert p.gains is None and p.noise_sigma is None and p.cutout is None
    y = pipe(x, 3)
    assert torch.equal(y, pipe.apply(x, A.AugmentParams(G_inv=_eye(4, 3), C=_eye(4, 4)), 3))
    assert not torch.equal(y, x) and float((y - x).abs().max()) < 1e-5 * float(x.abs().max())
    # no multiplier set: nothing runs
    assert A.AugmentPipe().to(DEV)(x, 3) is x


@pytest.mark.parametrize('kind', ['xflip', 'rotate90'])
def test_random_blits_hit_every_candidate(A, kind):
    """Only xflip=1 (only rotate90=1) at p = 1, B = 64: every sample is one of the 2 (4) candidate outputs and each candidate occurs.  The
    candidates are built from hand-made matrices (a quarter turn's cosine is 6e-17 in the kernel, 0 here; the batch's margin may be 6 or 7
    either way), so `is` means to 1e-5 of the range -- a different candidate is O(1) away."""
    B, C, H, W = 64, 3, 16, 16
    img = T(np.random.RandomState(2).randn(1, C, H, W))
    x = img.expand(B, C, H, W).contiguous()
    pipe = A.AugmentPipe(**{kind: 1}).to(DEV)
    torch.manual_seed(3)
    y = pipe(x, 3)
    if kind == 'xflip':
        mats = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[-1, 0, 0], [0, 1, 0], [0, 0, 1]]]
    else:
        mats = [[[round(math.cos(k * math.pi / 2)), round(math.sin(-k * math.pi / 2)), 0], [round(math.sin(k * math.pi / 2)), round(math.cos(k * math.pi / 2)), 0],
                 [0, 0, 1]] for k in range(4)]
    cands = [pipe.apply(img, A.AugmentParams(G_inv=torch.tensor([m], dtype=torch.float32, device=DEV)), 3)[0] for m in mats]
    rng = float(img.abs().max())
    hits = torch.stack([(y - c[None]).abs().amax(dim=(1, 2, 3)) <= 1e-5 * rng for c in cands], dim=1)        # [B, candidates]
    assert bool((hits.sum(dim=1) == 1).all()), hits.sum(dim=1).tolist()
    assert bool(hits.any(dim=0).all()), hits.sum(dim=0).tolist()
    for a in range(len(cands)):
        for b in range(a):
            assert float((cands[a] - cands[b]).abs().max()) > 0.1 * rng


def test_random_scale_and_brightness_spread(A):
    """params(4096, 64, 64) with only scale=1 (only brightness=1): log2 of the scale (the offset) has standard deviation within 6 % of 0.2,
    five standard errors of a 4096-sample estimate (1 / sqrt(2 * 4096) = 1.1 %)."""
    torch.manual_seed(13)
    p = A.AugmentPipe(scale=1).to(DEV).params(4096, 64, 64)
    s = torch.log2(p.G_inv[:, 0, 0])
    assert torch.equal(p.G_inv[:, 0, 0], p.G_inv[:, 1, 1]) and p.C is None
    assert abs(float(s.std()) / 0.2 - 1) <= 0.06 and abs(float(s.mean())) <= 5 * 0.2 / 64
    p = A.AugmentPipe(brightness=1).to(DEV).params(4096, 64, 64)
    b = p.C[:, 0, 3]
    assert torch.equal(b, p.C[:, 2, 3]) and p.G_inv is None
    assert abs(float(b.std()) / 0.2 - 1) <= 0.06 and abs(float(b.mean())) <= 5 * 0.2 / 64
    # at p = 0.5 about half of the samples are left alone
    pipe = A.AugmentPipe(brightness=1).to(DEV)
    pipe.p.fill_(0.5)
    frac = float((pipe.params(4096, 64, 64).C[:, 0, 3] == 0).float().mean())
    assert abs(frac - 0.5) <= 5 * 0.5 / 64


def test_noise_has_unit_variance_over_sigma(A):
    pipe = A.AugmentPipe(noise=1).to(DEV)
    x = T(np.random.RandomState(4).randn(8, 3, 32, 32))
    torch.manual_seed(17)
    p = pipe.params(8, 32, 32)
    assert p.G_inv is None and p.C is None and float(p.noise_sigma.min()) > 0
    out = pipe.apply(x, p, 3)
    base = pipe.apply(x, A.AugmentParams(), 3)
    assert base is x
    z = (out - x) / p.noise_sigma.reshape(-1, 1, 1, 1)
    assert abs(float(z.std()) - 1) <= 0.06 and abs(float(z.mean())) <= 5 / math.sqrt(z.numel())
    s = p.noise_sigma / 0.1                                                             # |N(0,1)|: mean sqrt(2 / pi)
    assert 0.2 < float(s.mean()) < 1.6


# ------------------------------------------------------------------------------------------------------------------------ no host round trip
def test_forward_is_capturable_in_a_graph(A):
    """A debug_percentile forward at [4,4,64,64] captured with torch.cuda.graph and replayed on new input contents equals the eager call
    byte for byte: nothing in the chain reads a value back (a read-back would fail the capture).  The chain is linear: no parallel branches."""
    pipe = A.AugmentPipe(**R.BASE).to(DEV)
    rs = np.random.RandomState(6)
    static = T(rs.randn(4, 4, 64, 64))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipe(static, 3, debug_percentile=0.35)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pipe(static, 3, debug_percentile=0.35)
    for _ in range(2):
        fresh = T(rs.randn(4, 4, 64, 64))
        static.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, pipe(fresh, 3, debug_percentile=0.35))


# ------------------------------------------------------------------------------------------------------------------------ loss integration
def test_loss_applies_the_pipe_before_the_discriminator(tdgp, A):
    """StyleGAN2Loss(augment_pipe=pipe), the pipe pinned to a percentile, leaves the same Dmain / Dreg / Gmain gradients as a loss without a
    pipe whose discriminator is D(pipe(img)) composed by hand; augment_pipe=None leaves the bytes of a loss built without the argument."""
    g = load_golden('loss')
    TR = tdgp.training
    cfg = tdgp.config.config_tiny()
    cfg.use_noise = False
    cfg.patch_resolution = 16
    dcfg = tdgp.discriminator.DiscriminatorConfig(c_dim=0, cbase=256, cmax=16, patch_params_cond=True, hyper_mod=True, mbstd_group_size=2)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=201, exercise_all=True))
    G = G.to(DEV).train()
    D = tdgp.discriminator.seeded_discriminator(dcfg, 16, 3, seed=202).to(DEV).train()
    pcfg = TR.PatchConfig(enabled=True, distribution='uniform', resolution=16, min_scale_trg=0.5, max_scale=1.0, anneal_kimg=10, mbstd_group_size=2)

    class Pinned(A.AugmentPipe):
        def forward(self, images, num_color_channels):
            return super().forward(images, num_color_channels, debug_percentile=0.35)

    class Composed(torch.nn.Module):
        def __init__(self, D, pipe):
            super().__init__()
            self.D, self.pipe = D, pipe

        def forward(self, img, c, **kw):
            return self.D(self.pipe(img, num_color_channels=3), c, **kw)

    pipe = Pinned(**R.BASE).to(DEV)
    kw = dict(r1_gamma=2.0, patch_cfg=pcfg, synthesis_kwargs=dict(u_coarse=T(g['u_coarse']), u_fine=T(g['u_fine'])))
    losses = dict(pipe=TR.StyleGAN2Loss(G, D, DEV, augment_pipe=pipe, **kw), hand=TR.StyleGAN2Loss(G, Composed(D, pipe), DEV, **kw),
                  none=TR.StyleGAN2Loss(G, D, DEV, augment_pipe=None, **kw), plain=TR.StyleGAN2Loss(G, D, DEV, **kw))
    pps = [dict(scales=T(g[f'pp{i}_scales']), offsets=T(g[f'pp{i}_offsets'])) for i in range(3)]
    queue = []
    orig = TR.sample_patch_params
    TR.sample_patch_params = lambda n, pc, device='cpu': queue.pop(0)
    c0 = torch.zeros(4, 0, device=DEV)
    cam = {k[4:]: T(v) for k, v in g.items() if k.startswith('cam_')}

    def run(which, phase, pp_list):
        for m in (G, D):
            m.zero_grad(set_to_none=True)
        G.requires_grad_(phase.startswith('G'))
        D.requires_grad_(phase.startswith('D'))
        queue[:] = pp_list
        real = tdgp.generator.TensorGroup(img=T(g['real']), c=c0, depth=torch.zeros(4, 1, 32, 32, device=DEV))
        gen = tdgp.generator.TensorGroup(z=T(g['z']), c=c0, camera_params=tdgp.generator.TensorGroup(**cam))
        losses[which].accumulate_gradients(phase, real, gen, gain=1, cur_nimg=0)
        assert not queue
        mod = G if phase.startswith('G') else D
        return {k: v.grad.clone() for k, v in mod.named_parameters() if v.grad is not None}

    try:
        for phase, pl in (('Gmain', [pps[0]]), ('Dmain', [pps[0], pps[1]]), ('Dreg', [pps[2]])):
            a, b, again = run('pipe', phase, pl), run('hand', phase, pl), run('pipe', phase, pl)
            assert a.keys() == b.keys() and len(a) >= 20
            # The two compositions launch the same kernels on the same bytes.  Where the phase itself returns the same bytes twice they must
            # agree byte for byte; the generator's backward scatters the plane gradients with float atomics (the order of the additions, and
            # with it the last bits, changes from run to run), so there the two agree as two runs of one composition do: to 1e-4 of the
            # tensor's largest entry (thousands of fp32 additions of either sign, 2^-24 each).
            repeatable = all(torch.equal(a[k], again[k]) for k in a)
            assert repeatable or phase == 'Gmain'

            def same(u, v, what):
                if repeatable:
                    assert all(torch.equal(u[k], v[k]) for k in u), (what, [k for k in u if not torch.equal(u[k], v[k])][:4])
                    return
                worst = max(float((u[k] - v[k]).abs().max()) / max(float(u[k].abs().max()), 1e-20) for k in u)
                report_parity(f'augment loss {phase}: {what}', worst_rel=worst)
                assert worst <= 1e-4, (what, worst)
            same(a, b, 'pipe in the loss vs composed by hand')
            n, p0 = run('none', phase, pl), run('plain', phase, pl)
            same(n, p0, 'augment_pipe=None vs no argument')
            assert any(not torch.equal(a[k], n[k]) for k in a)                         # and the pipe does change what D sees
        assert pipe.ada_stats is not None and pipe.ada_stats.tolist()[1] == 16.0         # Dmain and Dreg, each run twice above, added 4 signs a time
    finally:
        TR.sample_patch_params = orig

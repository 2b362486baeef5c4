"""tdgp_quantile_select (csrc/metrics.hip): exact order statistics by radix select, and its place behind `cut_quantile`.

The yardstick is never the kernel: order statistics are read off `torch.sort` of the same buffer (bit for bit), the interpolated third
output is held to `renderer._quantile(x, q)` -- torch.quantile up to 2^24 elements, sort + lerp above -- bit for bit, which is what lets
the select stand in front of march kernels that cut at a hard threshold.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
QS = (0.5, 0.3, 0.4, 0.123, 1.0)
N_DEGENERATE = (1 << 18) + 5


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def softplus_shaped(n, seed, offset=0):
    """Activated-density-like values (most of them near zero, a long tail), n elements starting `offset` elements into their allocation."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.nn.functional.softplus(torch.randn(n + offset, device=DEV, generator=g) * 4 - 3)
    return base[offset:]


def select(tdgp, x, k_lo, k_hi, weight, short_by=0):
    """The entry point itself, ranks given."""
    L = tdgp._lib
    n = x.numel()
    need = int(L.load().tdgp_quantile_select_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    out = torch.full([3], -123.0, device=x.device)
    L.call('tdgp_quantile_select', x.data_ptr(), n, k_lo, k_hi, weight, out.data_ptr(), ws.data_ptr(), need - short_by, L.stream_of(x))
    return out


def check_quantiles(tdgp, x, qs):
    R = tdgp.renderer
    xs = torch.sort(x).values
    n = x.numel()
    for q in qs:
        k_lo, k_hi, _ = R.quantile_ranks(q, n)
        out = R.quantile_select(x, q)
        assert bits(out[0]) == bits(xs[k_lo]) and bits(out[1]) == bits(xs[k_hi]), (n, q, k_lo, k_hi, out.tolist(), xs[k_lo].item(), xs[k_hi].item())
        want = R._quantile(x, q)
        assert bits(out[2]) == bits(want), (n, q, out.tolist(), want.item())


@pytest.mark.parametrize('n', [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4 * 21845 * 64 + 1])
def test_lengths(tdgp, n):
    x = softplus_shaped(n, seed=n % 1000)
    if n == 1:
        assert tdgp.renderer.quantile_ranks(0.5, 1)[:2] == (0, 0)
    check_quantiles(tdgp, x, QS)


def test_unaligned_head(tdgp):
    x = softplus_shaped((1 << 20) + 3, seed=5, offset=1)
    assert x.data_ptr() % 16 == 4
    check_quantiles(tdgp, x, QS)


def test_all_equal(tdgp):
    x = torch.full([N_DEGENERATE], 0.37, device=DEV)
    check_quantiles(tdgp, x, (0.5, 0.123, 1.0))


def test_zero_plateau(tdgp):
    """60 % exact zeros (clamp_mode='relu'): the plateau itself, and the step from its last zero to the first value above it."""
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.rand(N_DEGENERATE, device=DEV, generator=g) + 1e-3
    zeros = int(0.6 * N_DEGENERATE)
    x[torch.randperm(N_DEGENERATE, device=DEV, generator=g)[:zeros]] = 0.0
    check_quantiles(tdgp, x, (0.5, 0.7))
    xs = torch.sort(x).values
    out = select(tdgp, x, zeros - 1, zeros, 0.25)
    assert out[0].item() == 0.0 and bits(out[1]) == bits(xs[zeros]) and out[1].item() > 0.0
    assert bits(out[2]) == bits(torch.lerp(xs[zeros - 1], xs[zeros], 0.25))


def test_duplicates_straddling_the_ranks(tdgp):
    g = torch.Generator(device=DEV).manual_seed(7)
    xs = torch.sort(torch.randn(N_DEGENERATE, device=DEV, generator=g)).values
    mid = N_DEGENERATE // 2
    xs[mid - 500:mid + 500] = xs[mid]
    x = xs[torch.randperm(N_DEGENERATE, device=DEV, generator=g)].contiguous()
    check_quantiles(tdgp, x, (0.5,))
    for k in (mid - 501, mid - 500, mid + 498, mid + 499):                # both ends of the block, between the two ranks
        out = select(tdgp, x, k, k + 1, 0.5)
        assert bits(out[0]) == bits(xs[k]) and bits(out[1]) == bits(xs[k + 1])


def test_special_values(tdgp):
    """Negatives, -0.0, denormals and +inf order as floats; -0.0 is keyed as +0.0, so these compare as values."""
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn(N_DEGENERATE, device=DEV, generator=g)
    x[:4000] = -0.0
    x[4000:8000] = 0.0
    x[8000:9000] = torch.rand(1000, device=DEV, generator=g) * 1e-40            # denormals
    x[9000:10000] = -torch.rand(1000, device=DEV, generator=g) * 1e-40
    x[10000:10007] = float('inf')
    x[10007:10010] = float('-inf')
    x = x[torch.randperm(N_DEGENERATE, device=DEV, generator=g)].contiguous()
    xs = torch.sort(x).values
    n = N_DEGENERATE
    below = int((xs < 0).sum())                                          # the first zero of either sign
    for k in (0, 2, 3, below - 1000, below - 1, below, below + 7999, below + 8000, below + 8999, n // 3, n - 9, n - 8, n - 2):
        out = select(tdgp, x, k, k + 1, 0.0)
        assert out[0].item() == xs[k].item() and out[1].item() == xs[k + 1].item(), (k, out.tolist(), xs[k].item(), xs[k + 1].item())
    for q in (0.5, 0.123):
        assert tdgp.renderer.quantile_select(x, q)[2].item() == tdgp.renderer._quantile(x, q).item()


def test_first_and_last_rank(tdgp):
    x = softplus_shaped(N_DEGENERATE, seed=9)
    xs = torch.sort(x).values
    n = N_DEGENERATE
    for k_lo, k_hi in ((0, 0), (0, 1), (n - 2, n - 1), (n - 1, n - 1)):
        out = select(tdgp, x, k_lo, k_hi, 0.75)
        assert bits(out[0]) == bits(xs[k_lo]) and bits(out[1]) == bits(xs[k_hi])
        assert bits(out[2]) == bits(torch.lerp(xs[k_lo], xs[k_hi], 0.75))
    with pytest.raises(RuntimeError, match='ranks'):
        select(tdgp, x, n - 1, n, 0.5)


def test_nan_poisons_all_three(tdgp):
    x = softplus_shaped(N_DEGENERATE, seed=10).clone()
    x[12345] = float('nan')
    assert torch.isnan(tdgp.renderer.quantile_select(x, 0.5)).all()
    assert torch.isnan(tdgp.renderer._quantile(x, 0.5))


def test_above_2_24(tdgp):
    """Past torch.quantile's input limit: `_quantile`'s second branch (double-precision rank), and a bin holding more than 2^24 elements."""
    n = (1 << 24) + 5
    check_quantiles(tdgp, softplus_shaped(n, seed=11), (0.3,))
    x = torch.full([n], 1.0, device=DEV)
    x[100], x[2000], x[30000] = 0.25, 2.0, 3.0
    out = select(tdgp, x, 0, 1, 0.5)
    assert out.tolist() == [0.25, 1.0, 0.625]
    out = select(tdgp, x, n - 3, n - 2, 0.5)
    assert out.tolist() == [1.0, 2.0, 1.5]
    check_quantiles(tdgp, x, (0.5, 1.0))


def test_identical_bytes_from_run_to_run(tdgp):
    x = softplus_shaped(4 * 21845 * 64 + 1, seed=12)
    a, b = tdgp.renderer.quantile_select(x, 0.5), tdgp.renderer.quantile_select(x, 0.5)
    assert (bits(a) == bits(b)).all()


def test_workspace_one_byte_short_is_refused(tdgp):
    x = softplus_shaped(1025, seed=13)
    with pytest.raises(RuntimeError, match='workspace too small'):
        select(tdgp, x, 512, 513, 0.5, short_by=1)
    assert tdgp._lib.load().tdgp_quantile_select_workspace_bytes(0) == -1
    assert tdgp._lib.load().tdgp_quantile_select_workspace_bytes(1 << 31) == -1


# ------------------------------------------------------------------------------------------------ wiring behind cut_quantile
def _both_routes(tdgp, monkeypatch, run):
    """`run()` with the threshold from the select, then with `_quantile` (the sort) in its place."""
    R = tdgp.renderer
    calls = []
    real = R._select_threshold
    monkeypatch.setattr(R, '_select_threshold', lambda d, q: calls.append(d.numel()) or real(d, q))
    a = run()
    monkeypatch.setattr(R, '_select_threshold', lambda d, q: float(R._quantile(d, q)))
    b = run()
    assert calls, 'the select was not on the path'
    return a, b


@pytest.mark.parametrize('marcher,colors,q', [('ClassicalRayMarcher', 'colors', 0.5), ('MipRayMarcher2', 'colors01', 0.3)])
def test_marchers_cut_the_same_samples(tdgp, monkeypatch, marcher, colors, q):
    g = load_golden('marchers')
    m = getattr(tdgp.renderer, marcher)()
    a, b = _both_routes(tdgp, monkeypatch, lambda: m(T(g[colors]), T(g['densities']), T(g['depths']), dict(use_inf_depth=True, cut_quantile=q)))
    for x, y in zip(a, b):
        assert (bits(x) == bits(y)).all()


def test_importance_renderer_cut_quantile_bit_identical(tdgp, monkeypatch):
    cfg = tdgp.config.config_tiny()
    g = load_golden('e2e_tiny')
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=21, exercise_all=True))
    G = G.to(DEV)
    cam = {k[4:]: T(v) for k, v in g.items() if k.startswith('cam_')}

    def run():
        out = G.synthesis(T(g['ws']), camera_params=cam, noise_mode='const', render_opts=dict(return_depth=True, cut_quantile=0.5),
                          u_coarse=T(g['u_coarse']), u_fine=T(g['u_fine']))
        return out.img, out.depth
    a, b = _both_routes(tdgp, monkeypatch, run)
    for x, y in zip(a, b):
        assert (bits(x) == bits(y)).all()

"""Feature-space metrics on captured rows (src/metrics/{kernel_inception_distance,inception_score,precision_recall}.py): the host half.

Golden `feature_metrics.npz` (tools/gen_goldens.py:gen_feature_metrics): the reference's own compute_kid / compute_is / compute_pr on
synthetic rows that both sides regenerate from the stored recipe.  The precision / recall figures are checked on the GPU
(tests/test_pr_knn_gpu.py); here: KID and IS on CPU tensors, and the argument checks that need no device.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, report_parity


def feature_rows(g, index):
    """Set `index` of the golden's recipe: real = randn, gen = randn * scale + shift from ONE RandomState, fp32."""
    F, shift, scale = g['sets'][index]
    rs = np.random.RandomState(int(g['seed']))
    rows = int(g['rows'])
    real = rs.randn(rows, int(F)).astype(np.float32)
    gen = (rs.randn(rows, int(F)) * scale + shift).astype(np.float32)
    return real, gen


def class_probs(g):
    u = np.random.RandomState(int(g['is_seed'])).rand(int(g['is_rows']), int(g['is_classes'])) + 0.05
    return (u / u.sum(axis=1, keepdims=True)).astype(np.float32)


class FakeG(torch.nn.Module):
    """Stand-in generator for the feature loops: unconditional, no camera adaptor, images of zeros (the detector below ignores them)."""
    z_dim, c_dim = 4, 0

    def __init__(self, device='cpu'):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=device))
        self.synthesis = torch.nn.Identity()
        self.calls = 0

    def forward(self, z, c, camera_params, **kw):
        self.calls += 1
        return torch.zeros(z.shape[0], 3, 2, 2, device=z.device)


class RowsDetector:
    """Stand-in detector: hands out the given rows in order, one per image, on the images' device."""

    def __init__(self, rows, device='cpu'):
        self.rows, self.at = torch.from_numpy(rows).to(device), 0

    def __call__(self, images):
        assert images.dtype == torch.uint8 and images.shape[1] == 3
        out = self.rows[self.at:self.at + images.shape[0]]
        self.at += images.shape[0]
        return out


def test_generator_wrappers_on_the_host(tdgp, tmp_path):
    """kid_for_generator / is_for_generator through compute_feature_stats_for_generator (capture_all passed through, the last block cut to
    num_gen): the figures of compute_kid / compute_is on the same rows; ranks other than 0 answer NaN after taking part in the loop."""
    M = tdgp.metrics
    g = load_golden('feature_metrics')
    real, gen = feature_rows(g, 0)                                  # 600 rows: 64 does not divide them, the last block is cut
    G = FakeG()
    np.random.seed(5)
    got = M.kid_for_generator(G, RowsDetector(gen), real, num_gen=600, num_subsets=3, max_subset_size=80, batch_size=64, batch_gen=16)
    # the camera prior of the feature loop draws from numpy's global RNG too (scipy's truncnorm), as the reference's does: the subsets follow
    np.random.seed(5)
    rows = M.compute_feature_stats_for_generator(FakeG(), RowsDetector(gen), 600, batch_size=64, batch_gen=16, device='cpu', capture_all=True).get_all()
    np.testing.assert_array_equal(rows, gen)
    assert got == M.compute_kid(torch.from_numpy(real), torch.from_numpy(rows), num_subsets=3, max_subset_size=80) and G.calls == 10 * 4
    st = M.FeatureStats(capture_all=True)
    st.append(real)
    st.save(str(tmp_path / 'real.npz'))
    np.random.seed(5)
    assert M.kid_for_generator(FakeG(), RowsDetector(gen), str(tmp_path / 'real.npz'), num_gen=600, num_subsets=3, max_subset_size=80, batch_size=64, batch_gen=16) == got
    probs = class_probs(g)
    assert M.is_for_generator(FakeG(), RowsDetector(probs), num_gen=500, num_splits=5, batch_size=100) == M.compute_is(torch.from_numpy(probs), num_splits=5)
    other = M.kid_for_generator(FakeG(), RowsDetector(gen), real, num_gen=64, num_gpus=2, rank=1, gatherer=type('One', (), dict(gather=staticmethod(lambda x: x)))())
    assert np.isnan(other)
    assert all(np.isnan(v) for v in M.is_for_generator(FakeG(), RowsDetector(probs), num_gen=50, num_gpus=2, rank=1,
                                                       gatherer=type('One', (), dict(gather=staticmethod(lambda x: x)))()))


def test_calc_feature_metrics_tool(tdgp, tmp_path, capsys, monkeypatch):
    """tools/calc_feature_metrics.py: saved FeatureStats in, one JSON line out; kid and is need no GPU."""
    import importlib.util
    import json
    import os
    M = tdgp.metrics
    g = load_golden('feature_metrics')
    real, gen = (np.abs(a) + 0.01 for a in feature_rows(g, 0))    # positive rows, so that the same file can be read as probabilities
    gen = (gen / gen.sum(1, keepdims=True)).astype(np.float32)
    for name, rows in (('real', real.astype(np.float32)), ('gen', gen)):
        st = M.FeatureStats(capture_all=True)
        st.append(rows)
        st.save(str(tmp_path / f'{name}.npz'))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('calc_feature_metrics', os.path.join(repo, 'tools', 'calc_feature_metrics.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)       # the host route, wherever the test runs
    tool.main(['--real', str(tmp_path / 'real.npz'), '--gen', str(tmp_path / 'gen.npz'), '--metrics', 'kid,is', '--num-subsets', '3', '--max-subset-size', '50',
               '--num-splits', '4', '--seed', '9'])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    np.random.seed(9)
    assert out['kid'] == M.compute_kid(torch.from_numpy(real.astype(np.float32)), torch.from_numpy(gen), num_subsets=3, max_subset_size=50)
    assert (out['is_mean'], out['is_std']) == M.compute_is(torch.from_numpy(gen), num_splits=4)
    assert out['num_real'] == out['num_gen'] == 600 and 'precision' not in out
    with pytest.raises(SystemExit):
        tool.main(['--gen', str(tmp_path / 'gen.npz'), '--metrics', 'pr'])


def test_inception_score_matches_the_reference(tdgp):
    """Same operations as the reference's fp32 numpy, in fp64: 1e-6 relative."""
    g = load_golden('feature_metrics')
    mean, std = tdgp.metrics.compute_is(torch.from_numpy(class_probs(g)), num_splits=int(g['is_splits']))
    ref_mean, ref_std = (float(v) for v in g['inception_score'])
    report_parity('inception score vs the reference', mean=mean, ref_mean=ref_mean, std=std, ref_std=ref_std)
    assert abs(mean - ref_mean) <= 1e-6 * abs(ref_mean)
    # the std is a difference of scores that agree to 1e-6 of the MEAN: its own error is 1e-6 of the mean, not of itself (measured: the
    # std is 5.3e-6 of ITSELF from the reference's fp32 numpy value, i.e. 6e-9 of the mean)
    assert abs(std - ref_std) <= 1e-6 * abs(ref_mean)
    assert ref_std > 0 and mean > 1


def test_kid_matches_the_reference(tdgp):
    """KID is a difference of large sums: the bound is not typed in.  The formula is also evaluated in float64 on the SAME subsets; ours must
    be no further from that than twice the reference's own distance (a third rounding scheme: fp32 products, fp64 sums), with an absolute
    floor of one fp32 ulp of the largest term, a.sum() / (m - 1).
    Measured (CPU): |ours - float64| = 9.5e-10, |reference - float64| = 1.0e-08 on a KID of 0.14158; floor 1.5e-07."""
    g = load_golden('feature_metrics')
    real, gen = feature_rows(g, int(g['kid_set']))
    num_subsets, max_subset = int(g['kid_num_subsets']), int(g['kid_max_subset_size'])
    np.random.seed(int(g['kid_seed']))
    ours = tdgp.metrics.compute_kid(torch.from_numpy(real), torch.from_numpy(gen), num_subsets=num_subsets, max_subset_size=max_subset)
    # float64 on the same subsets, the reference's draw order: generated first, then real
    np.random.seed(int(g['kid_seed']))
    n, m = real.shape[1], min(real.shape[0], gen.shape[0], max_subset)
    r64, g64 = real.astype(np.float64), gen.astype(np.float64)
    t, largest = 0.0, 0.0
    for _ in range(num_subsets):
        x = g64[np.random.choice(gen.shape[0], m, replace=False)]
        y = r64[np.random.choice(real.shape[0], m, replace=False)]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
        largest = max(largest, a.sum() / (m - 1))
    exact = t / num_subsets / m
    ref = float(g['kid'])
    floor = float(np.spacing(np.float32(largest))) / m          # one fp32 ulp of the largest term, carried through the final / m
    bound = max(2 * abs(ref - exact), floor)
    print(f'kid: ours {ours!r}, reference {ref!r}, float64 {exact!r}; |ours - f64| {abs(ours - exact):.3e}, |ref - f64| {abs(ref - exact):.3e}, floor {floor:.3e}')
    report_parity('KID vs float64 on the same subsets', ours=abs(ours - exact), reference=abs(ref - exact), floor=floor, kid=exact)
    assert abs(ours - exact) <= bound
    assert 0.01 < exact < 1.0                                   # a real distance between the two sets, not a degenerate zero


def test_kid_follows_the_reference_draw_order(tdgp):
    """Two seeded calls agree; swapping the seed changes the subsets and with them the estimate."""
    g = load_golden('feature_metrics')
    real, gen = (torch.from_numpy(a) for a in feature_rows(g, 0))
    out = []
    for seed in (3, 3, 4):
        np.random.seed(seed)
        out.append(tdgp.metrics.compute_kid(real, gen, num_subsets=4, max_subset_size=50))
    assert out[0] == out[1] and out[0] != out[2]


def test_pr_argument_checks(tdgp):
    M = tdgp.metrics
    a, b = torch.zeros(6, 8), torch.zeros(5, 8)
    with pytest.raises(RuntimeError, match='GPU'):
        M.compute_pr(a, b)
    with pytest.raises(RuntimeError, match='GPU'):
        M.compute_distances_kth(a, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        M.compute_manifold_membership(a, b, torch.zeros(5, dtype=torch.float16))
    with pytest.raises(ValueError, match=r'k \+ 1 > Nc'):
        M.compute_distances_kth(torch.zeros(3, 8), 3)
    with pytest.raises(ValueError, match=r'k \+ 1 > Nc'):
        M.compute_pr(a, torch.zeros(2, 8), nhood_size=2)
    with pytest.raises(ValueError, match='nhood_size'):
        M.compute_distances_kth(torch.zeros(20, 8), 8)
    with pytest.raises(ValueError, match=r'feature width mismatch \(F\)'):
        M.compute_pr(a, torch.zeros(5, 9))
    with pytest.raises(ValueError, match=r'feature width mismatch \(F\)'):
        M.compute_manifold_membership(a, torch.zeros(5, 9), torch.zeros(5, dtype=torch.float16))
    with pytest.raises(ValueError, match=r'feature width mismatch \(F\)'):
        M.compute_kid(a, torch.zeros(5, 9))
    with pytest.raises(ValueError, match='kth'):
        M.compute_manifold_membership(a, b, torch.zeros(4, dtype=torch.float16))
    # other ranks return NaN before anything touches a device, as the reference's do
    p, r = M.compute_pr(a, b, num_gpus=2, rank=1)
    assert np.isnan(p) and np.isnan(r)
    # the reference's batching arguments are accepted
    import inspect
    assert list(inspect.signature(M.compute_pr).parameters)[:5] == ['real_features', 'gen_features', 'nhood_size', 'row_batch_size', 'col_batch_size']


def test_workspace_queries_need_no_device(tdgp):
    lib = tdgp._lib.load()
    # 128 x 128 tiles, 8 column tiles per block: 50 000 columns are 49 runs; lists of 4 uint32 per (run, row) for k + 1 <= 4, of 8 above
    assert lib.tdgp_pr_kth_workspace_bytes(50000, 50000, 4) == 49 * 50000 * 4 * 4
    assert lib.tdgp_pr_kth_workspace_bytes(50000, 50000, 5) == 49 * 50000 * 8 * 4
    assert lib.tdgp_pr_member_workspace_bytes(50000, 50000) == 50000 * 4 + 49 * 50000
    assert lib.tdgp_pr_kth_workspace_bytes(10, 10, 9) == -1 and lib.tdgp_pr_kth_workspace_bytes(0, 10, 4) == -1
    assert lib.tdgp_pr_member_workspace_bytes(10, (1 << 24) + 1) == -1


def test_generator_wrappers_accept_saved_stats(tdgp, tmp_path):
    """The real side of the generator-side wrappers: an array, a FeatureStats, or the path of a saved one."""
    M = tdgp.metrics
    rows = np.random.RandomState(0).randn(7, 5).astype(np.float32)
    st = M.FeatureStats(capture_all=True)
    st.append(rows)
    path = str(tmp_path / 'real.npz')
    st.save(path)
    for real in (rows, st, path, torch.from_numpy(rows)):
        np.testing.assert_array_equal(M._real_rows(real).numpy(), rows)

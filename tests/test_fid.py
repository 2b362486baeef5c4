"""FID on the host side: the eigh form of the Frechet distance against the reference's expression, compute_fid's three input forms, the `fid`
entry of tools/calc_feature_metrics.py, the unchanged host FeatureStats, and the moments entry points in header / loader / library."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden, report_parity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mean_cov(x):
    return x.mean(0), np.cov(x, rowvar=False)


def distance_sets():
    """Two pairs of (mu, sigma) at F = 64: full rank (500 and 400 rows, one set mixed by a random matrix) and rank deficient (40 and 50 rows)."""
    rs = np.random.RandomState(0)
    full = (mean_cov(rs.randn(500, 64)), mean_cov(rs.randn(400, 64) @ rs.randn(64, 64)))
    deficient = (mean_cov(rs.randn(40, 64)), mean_cov(rs.randn(50, 64) * 1.3 + 0.2))
    return dict(full=full, deficient=deficient)


@pytest.mark.parametrize('name', ['full', 'deficient'])
def test_frechet_distance_eigh_against_the_reference_expression(tdgp, name):
    """Tolerance: 1e-8 * max(1, |value|), the one test_frechet_distance uses for the eigenvalue form."""
    M = tdgp.metrics
    (mu_a, s_a), (mu_b, s_b) = distance_sets()[name]
    ref = M.frechet_distance(mu_a, s_a, mu_b, s_b)
    got = M.frechet_distance_eigh(mu_a, s_a, mu_b, s_b)
    swapped = M.frechet_distance_eigh(mu_b, s_b, mu_a, s_a)
    tensors = M.frechet_distance_eigh(*(torch.from_numpy(a) for a in (mu_a, s_a, mu_b, s_b)))
    report_parity(f'frechet_distance_eigh vs sqrtm ({name}, CPU)', value=ref, rel=abs(got - ref) / max(1.0, abs(ref)), swapped_rel=abs(got - swapped) / max(1.0, abs(ref)))
    tol = 1e-8 * max(1.0, abs(ref))
    assert abs(got - ref) <= tol and abs(swapped - got) <= tol and tensors == got


def test_frechet_distance_eigh_is_zero_on_identical_statistics(tdgp):
    mu, sigma = distance_sets()['full'][1]
    assert abs(tdgp.metrics.frechet_distance_eigh(mu, sigma, mu, sigma)) < 1e-6


def golden_stats(M, **kw):
    g = load_golden('metrics')
    st = M.FeatureStats(capture_all=True, capture_mean_cov=True, max_items=200, **kw)
    for f in g['fs_feats']:
        st.append(f)
    return g, st


def test_host_feature_stats_are_the_old_object(tdgp):
    """FeatureStats(device=None): numpy inside, get_mean_cov on the golden blocks bit-identical to the golden; the torch read-outs are views of it."""
    g, st = golden_stats(tdgp.metrics, device=None)
    assert st.device is None and isinstance(st._moments.s2, np.ndarray) and all(isinstance(b, np.ndarray) for b in st._kept)
    mean, cov = st.get_mean_cov()
    np.testing.assert_array_equal(mean, g['fs_mean'])
    np.testing.assert_array_equal(cov, g['fs_cov'])
    mean_t, cov_t = st.get_mean_cov_torch()
    assert mean_t.dtype == cov_t.dtype == torch.float64 and np.array_equal(cov_t.numpy(), g['fs_cov']) and np.array_equal(mean_t.numpy(), g['fs_mean'])
    assert np.array_equal(st.get_all_torch().numpy(), g['fs_all'])
    with pytest.raises(ValueError, match='GPU'):
        tdgp.metrics.FeatureStats(device='cpu')
    with pytest.raises(AssertionError, match='device'):
        st.add_rows(torch.zeros(2, g['fs_all'].shape[1]))


def test_compute_fid_input_forms(tdgp, tmp_path):
    """FeatureStats, saved paths and (mu, sigma) pairs give the same float: frechet_distance of the golden's mean and covariance against a
    second set made from the same rows."""
    M = tdgp.metrics
    g, real = golden_stats(M)
    gen = M.FeatureStats(capture_mean_cov=True)
    gen.append(g['fs_all'][::-1][:150] * 0.9 + 0.05)
    real.save(str(tmp_path / 'real.npz'))
    gen.save(str(tmp_path / 'gen.npz'))
    want = M.frechet_distance(*gen.get_mean_cov(), g['fs_mean'], g['fs_cov'])
    assert np.isfinite(want) and want > 0
    assert M.compute_fid(real, gen) == want
    assert M.compute_fid(str(tmp_path / 'real.npz'), str(tmp_path / 'gen.npz')) == want
    assert M.compute_fid(tmp_path / 'real.npz', gen) == want
    assert M.compute_fid((g['fs_mean'], g['fs_cov']), gen.get_mean_cov()) == want
    assert M.compute_fid(tuple(torch.from_numpy(a) for a in (g['fs_mean'], g['fs_cov'])), gen.get_mean_cov_torch()) == want


class FakeG:
    z_dim, c_dim, device = 4, 0, 'cpu'

    class synthesis:
        camera_adaptor = None

    def __call__(self, z, c, camera_params, **kw):
        return torch.zeros(z.shape[0], 3, 2, 2)


def test_fid_for_generator_on_the_host(tdgp):
    """fid_for_generator on a CPU generator: host statistics, compute_fid of them; NaN on ranks other than 0."""
    M = tdgp.metrics
    g, real = golden_stats(M)
    rows = np.ascontiguousarray(g['fs_all'][::-1]) * 0.5

    class Detector:
        def __init__(self):
            self.at = 0

        def __call__(self, images):
            out = torch.from_numpy(rows[self.at:self.at + images.shape[0]])
            self.at += images.shape[0]
            return out
    got = M.fid_for_generator(FakeG(), Detector(), real, num_gen=150, batch_size=64, batch_gen=16)
    gen = M.FeatureStats(capture_mean_cov=True)
    for a in (0, 64, 128):                                              # the loop's blocks: 64 + 64 + 22, the last one cut to num_gen
        gen.append(rows[a:min(a + 64, 150)])
    assert got == M.compute_fid(real, gen) and np.isfinite(got)
    one = type('One', (), dict(gather=staticmethod(lambda x: x)))()
    assert np.isnan(M.fid_for_generator(FakeG(), Detector(), real, num_gen=64, num_gpus=2, rank=1, gatherer=one))


def load_tool():
    spec = importlib.util.spec_from_file_location('calc_feature_metrics', os.path.join(REPO, 'tools', 'calc_feature_metrics.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_prints_fid_and_leaves_kid_is_alone(tdgp, tmp_path, capsys, monkeypatch):
    M = tdgp.metrics
    g = load_golden('metrics')
    rows = g['fs_all']
    real_rows = np.abs(rows) + 0.01
    gen_rows = (np.abs(rows[::-1]) + 0.02)
    gen_rows = (gen_rows / gen_rows.sum(1, keepdims=True)).astype(np.float32)
    for name, r in (('real', real_rows), ('gen', gen_rows)):
        both = M.FeatureStats(capture_all=True, capture_mean_cov=True)
        both.append(r)
        both.save(str(tmp_path / f'{name}.npz'))
        only_rows = M.FeatureStats(capture_all=True)
        only_rows.append(r)
        only_rows.save(str(tmp_path / f'{name}_rows.npz'))
    tool = load_tool()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)       # the host route, wherever the test runs

    def run(*argv):
        tool.main(list(argv))
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = M.compute_fid(str(tmp_path / 'real.npz'), str(tmp_path / 'gen.npz'))
    out = run('--real', str(tmp_path / 'real.npz'), '--gen', str(tmp_path / 'gen.npz'), '--metrics', 'fid')
    assert out['fid'] == want and out['num_real'] == out['num_gen'] == rows.shape[0]
    # files that hold only rows: the moments are accumulated first (one block, the host's own arithmetic here)
    assert run('--real', str(tmp_path / 'real_rows.npz'), '--gen', str(tmp_path / 'gen_rows.npz'), '--metrics', 'fid')['fid'] == want
    # kid,is: the keys and values of before, with or without fid beside them
    kw = ('--num-subsets', '3', '--max-subset-size', '50', '--num-splits', '4', '--seed', '9')
    plain = run('--real', str(tmp_path / 'real_rows.npz'), '--gen', str(tmp_path / 'gen_rows.npz'), '--metrics', 'kid,is', *kw)
    np.random.seed(9)
    assert plain['kid'] == M.compute_kid(torch.from_numpy(real_rows.astype(np.float32)), torch.from_numpy(gen_rows), num_subsets=3, max_subset_size=50)
    assert (plain['is_mean'], plain['is_std']) == M.compute_is(torch.from_numpy(gen_rows), num_splits=4)
    assert sorted(plain) == sorted(['kid', 'is_mean', 'is_std', 'num_real', 'num_gen', 'seed', 'real', 'gen'])
    mixed = run('--real', str(tmp_path / 'real.npz'), '--gen', str(tmp_path / 'gen.npz'), '--metrics', 'kid,is,fid', *kw)
    assert mixed['fid'] == want and all(mixed[k] == plain[k] for k in ('kid', 'is_mean', 'is_std', 'num_real', 'num_gen'))
    with pytest.raises(SystemExit):
        tool.main(['--gen', str(tmp_path / 'gen.npz'), '--metrics', 'fid'])


def test_moments_entry_points_in_header_loader_and_library(tdgp):
    """include/tdgp.h, _lib.py and the built library agree on the two new symbols and on their argument lists."""
    from ctypes import c_int, c_int64, c_void_p
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'tdgp.h')).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r'\b(int64_t|int)\s+(tdgp_moments_\w+)\s*\(([^)]*)\)\s*;', header)}
    assert sorted(protos) == ['tdgp_moments_add', 'tdgp_moments_workspace_bytes']

    def ctype(arg):
        arg = arg.strip()
        return c_void_p if '*' in arg or arg.startswith('tdgp_stream_t') else {'int64_t': c_int64, 'int': c_int}[arg.split()[0]]
    table = tdgp._lib._PROTOTYPES
    for name, (res, args) in protos.items():
        assert name in tdgp._lib.EXPORTS
        assert table[name] == ({'int64_t': c_int64, 'int': c_int}[res], [ctype(a) for a in args.split(',')]), name
    lib_path = tdgp.build.build_native()
    lib = tdgp._lib.load()
    out = subprocess.run(['nm', '-D', '--defined-only', lib_path], capture_output=True, text=True).stdout
    for name in protos:
        assert hasattr(lib, name) and re.search(rf' T {name}\b', out), name
    # the size query answers without a GPU: -1 for shapes it refuses, 16 bytes (untouched) for one run of rows, more once the rows are split
    q = lib.tdgp_moments_workspace_bytes
    assert q(-1, 64) == -1 and q(10, 0) == -1 and q(10, 1 << 20) == -1 and q(1 << 31, 64) == -1
    assert q(0, 64) == 16 and q(64, 2048) == 16 and q(1 << 21, 4096) >= 16 and q(1 << 21, 64) > q(512, 64) == 16

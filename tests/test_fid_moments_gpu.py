"""FID on the device: tdgp_moments_add (csrc/metrics.hip), FeatureStats(device=...), the feature loop with device statistics, and the eigh
form of the Frechet distance on device tensors.

Bit-exact part: rows are integers in [-4, 4] (times a power of two where the test says so), so every sum is an integer below 2^53 times that
power and exact in fp64 in ANY order; numpy's fp64 `r.sum(0)` and `r.T @ r` are then the exact values and s1 / s2 must equal them bit for bit.
The data has no symmetry, so a transposed or permuted MFMA layout cannot pass.

The kernel's s2 tile is T x T, it stages C rows per K step, and rows are split into runs of at least RUN once tiles x 2 <= 2048 blocks: the
shapes below sit on those edges.

Rounding part: on Gaussian rows the bound is the standard one for n exact products summed in fp64 in any order,
|s2 - exact| <= n 2^-53 (|R|^T |R|) element-wise (and the same for s1 with sum |R|); nothing in it is measured.
"""
import numpy as np
import pytest
import torch

from conftest import report_parity
from test_fid import distance_sets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = 64                                   # MOM_T: tile edge of s2
C = 32                                   # MOM_C: rows per K step
RUN = 512                                # MOM_RUN_MIN: the shortest run of rows; RUN + 3 rows make two runs at the widths used here
U = 2.0 ** -53


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()


def lattice(rs, n, F, scale=1.0):
    return (rs.randint(-4, 5, size=(n, F)) * scale).astype(np.float32)


def host_moments(rows):
    r = np.asarray(rows, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return r.sum(axis=0), r.T @ r


def runs_of(tdgp, n, F):
    return int(tdgp._lib.load().tdgp_moments_workspace_bytes(n, F)) > 16


def gpu_add(tdgp, rows, s1, s2, short_by=0):
    """One tdgp_moments_add on device tensors; returns the status."""
    L = tdgp._lib
    n, F = rows.shape
    need = int(L.load().tdgp_moments_workspace_bytes(n, F))
    assert need >= 16
    ws = torch.empty([need], dtype=torch.uint8, device=DEV)
    return int(L.load().tdgp_moments_add(rows.data_ptr(), n, F, s1.data_ptr(), s2.data_ptr(), ws.data_ptr(), need - short_by, L.stream_of(rows)))


def gpu_moments(tdgp, rows, s1=None, s2=None):
    """rows (numpy) -> (s1, s2) numpy after one call into `s1` / `s2` (zeros by default).  The rows sit at the front of a buffer whose rest is
    NaN: a read past n rows cannot go unnoticed."""
    n, F = rows.shape
    buf = torch.full([n * F + 8192], float('nan'), dtype=torch.float32, device=DEV)
    buf[:n * F] = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV).reshape(-1)
    s1 = torch.zeros([F], dtype=torch.float64, device=DEV) if s1 is None else s1
    s2 = torch.zeros([F, F], dtype=torch.float64, device=DEV) if s2 is None else s2
    assert gpu_add(tdgp, buf[:n * F].view(n, F), s1, s2) == 0
    return s1.cpu().numpy(), s2.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------ bit for bit on lattices
@pytest.mark.parametrize('F', [1, 3, 15, 16, 17, T - 1, T, T + 1, 2 * T + 1])
def test_moments_on_lattices_at_the_tile_edges(tdgp, F):
    rs = np.random.RandomState(F)
    assert runs_of(tdgp, RUN + 3, F) and not runs_of(tdgp, RUN, F)
    for n, scale in ((1, 1.0), (3, 1.0), (4, 2.0 ** -10), (5, 1.0), (C - 1, 2.0 ** 20), (C, 1.0), (C + 1, 1.0), (RUN + 3, 1.0)):
        rows = lattice(rs, n, F, scale)
        s1, s2 = gpu_moments(tdgp, rows)
        w1, w2 = host_moments(rows)
        assert same_bits(s1, w1), (n, F, 's1')
        assert same_bits(s2, w2), (n, F, 's2', np.argwhere(s2 != w2)[:4])


def test_moments_on_a_lattice_at_the_loop_shape(tdgp):
    rows = lattice(np.random.RandomState(1), 64, 2048)
    s1, s2 = gpu_moments(tdgp, rows)
    w1, w2 = host_moments(rows)
    assert same_bits(s1, w1) and same_bits(s2, w2)


def test_moments_accumulate_into_running_totals(tdgp):
    """Three calls of different n (the last one split into runs) into non-zero totals = one host accumulation of the concatenation."""
    rs = np.random.RandomState(2)
    F = T + 7
    blocks = [lattice(rs, n, F) for n in (40, 5, 70, RUN + C + 1)]
    w1, w2 = host_moments(blocks[0])
    s1, s2 = torch.from_numpy(w1).to(DEV), torch.from_numpy(w2).to(DEV)
    for b in blocks[1:]:
        gpu_moments(tdgp, b, s1, s2)
    w1, w2 = host_moments(np.concatenate(blocks))
    assert same_bits(s1.cpu().numpy(), w1) and same_bits(s2.cpu().numpy(), w2)


# ------------------------------------------------------------------------------------------------ Gaussian rows
def test_moments_are_symmetric_and_deterministic(tdgp):
    rs = np.random.RandomState(3)
    n, F = 3 * RUN + 17, 2 * T + 9
    assert runs_of(tdgp, n, F)
    rows = rs.randn(n, F).astype(np.float32)
    a1, a2 = gpu_moments(tdgp, rows)
    b1, b2 = gpu_moments(tdgp, rows)
    assert same_bits(a2, a2.T) and same_bits(a1, b1) and same_bits(a2, b2)
    one = rs.randn(200, F).astype(np.float32)                      # one run: the in-place route
    assert not runs_of(tdgp, 200, F)
    c1, c2 = gpu_moments(tdgp, one)
    d1, d2 = gpu_moments(tdgp, one)
    assert same_bits(c2, c2.T) and same_bits(c1, d1) and same_bits(c2, d2)


def test_moments_rounding_bound(tdgp):
    """n = 200 in blocks of 64 + 64 + 72, F = 96, N(0, 1): |s2 - exact| <= n 2^-53 |R|^T |R| and |s1 - exact| <= n 2^-53 sum |R|, the exact
    values in extended precision (products of fp32 values are exact there, the 200-term sums are good to 2^-64 relative)."""
    assert np.finfo(np.longdouble).nmant >= 63
    rs = np.random.RandomState(4)
    n, F = 200, 96
    rows = rs.randn(n, F).astype(np.float32)
    s1 = torch.zeros([F], dtype=torch.float64, device=DEV)
    s2 = torch.zeros([F, F], dtype=torch.float64, device=DEV)
    for a, b in ((0, 64), (64, 128), (128, 200)):
        gpu_moments(tdgp, rows[a:b], s1, s2)
    s1, s2 = s1.cpu().numpy(), s2.cpu().numpy()
    r = rows.astype(np.longdouble)
    exact1, exact2 = r.sum(axis=0), np.einsum('kf,kg->fg', r, r)
    bound1, bound2 = n * U * np.abs(r).sum(axis=0), n * U * np.einsum('kf,kg->fg', np.abs(r), np.abs(r))
    e1, e2 = np.abs(s1.astype(np.longdouble) - exact1), np.abs(s2.astype(np.longdouble) - exact2)
    h1, h2 = host_moments(rows)
    report_parity('fp64 moments vs exact, as a share of n 2^-53 |R|^T |R|', s2=float((e2 / bound2).max()), s1=float((e1 / bound1).max()),
                  numpy_s2=float((np.abs(h2.astype(np.longdouble) - exact2) / bound2).max()))
    print(f'moments rounding: s2 at {float((e2 / bound2).max()):.3f} of the bound, s1 at {float((e1 / bound1).max()):.3f}')
    assert (e1 <= bound1).all() and (e2 <= bound2).all()


def test_moments_special_values_stay_in_their_rows_and_columns(tdgp):
    """One NaN and one +Inf inside a partial tile and a partial K step: the NaN pattern is numpy's (only those rows and columns of s2, those
    entries of s1), every other entry is bit-equal."""
    rs = np.random.RandomState(5)
    n, F = C + 5, T + 6
    rows = lattice(rs, n, F)
    rows[C + 1, 5] = np.nan
    rows[C + 3, T + 2] = np.inf
    s1, s2 = gpu_moments(tdgp, rows)
    w1, w2 = host_moments(rows)
    assert np.array_equal(np.isnan(s1), np.isnan(w1)) and np.array_equal(np.isnan(s2), np.isnan(w2))
    assert np.isnan(w2).sum() < 4 * F and np.isinf(w2).any()
    keep1, keep2 = ~np.isnan(w1), ~np.isnan(w2)
    assert same_bits(s1[keep1], w1[keep1]) and same_bits(s2[keep2], w2[keep2])


def test_moments_refusals(tdgp):
    rs = np.random.RandomState(6)
    lib = tdgp._lib.load()
    for n, F in ((RUN + 3, T), (40, T)):                            # several runs (a real workspace) and one run (16 bytes, untouched)
        rows = torch.from_numpy(lattice(rs, n, F)).to(DEV)
        s1 = torch.full([F], 3.0, dtype=torch.float64, device=DEV)
        s2 = torch.full([F, F], -2.0, dtype=torch.float64, device=DEV)
        assert gpu_add(tdgp, rows, s1, s2, short_by=1) != 0
        assert b'workspace too small' in lib.tdgp_last_error()
        assert gpu_add(tdgp, rows[:0], s1, s2) == 0                 # n = 0: nothing to do
        torch.cuda.synchronize()
        assert bool((s1 == 3.0).all()) and bool((s2 == -2.0).all())
    assert lib.tdgp_moments_workspace_bytes(10, 0) == -1 and lib.tdgp_moments_workspace_bytes(-1, 8) == -1
    ws = torch.empty([16], dtype=torch.uint8, device=DEV)
    assert lib.tdgp_moments_add(rows.data_ptr(), 10, 0, s1.data_ptr(), s2.data_ptr(), ws.data_ptr(), 16, tdgp._lib.stream_of(rows)) != 0


# ------------------------------------------------------------------------------------------------ FeatureStats on the device
def test_device_feature_stats_match_the_host_object(tdgp, tmp_path, monkeypatch):
    """Lattice blocks, max_items cutting the middle block: counts, rows, mean / covariance and the saved file bit-equal to the host class;
    append_torch makes no host copy."""
    M = tdgp.metrics
    rs = np.random.RandomState(7)
    F = 40
    blocks = [lattice(rs, n, F, 0.25) for n in (70, 64, 50)]
    host = M.FeatureStats(capture_all=True, capture_mean_cov=True, max_items=100)
    dev = M.FeatureStats(capture_all=True, capture_mean_cov=True, max_items=100, device=DEV)
    copies = []

    def spy(owner, name):
        real = getattr(owner, name)
        monkeypatch.setattr(owner, name, lambda *a, **k: (copies.append(name), real(*a, **k))[1])
    for name in ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__float__', '__int__'):     # every way a value or a block reaches the host
        spy(torch.Tensor, name)
    spy(torch.cuda, 'synchronize')
    spy(torch.cuda.Stream, 'synchronize')
    spy(torch.cuda.Event, 'synchronize')
    for i, b in enumerate(blocks):
        host.append(b)
        if i == 1:
            dev.append(b)                                           # numpy rows are uploaded and take the same route
        else:
            dev.append_torch(torch.from_numpy(b).to(DEV))
        assert dev.num_items == host.num_items and dev.is_full() == host.is_full()
    monkeypatch.undo()
    assert copies == [] and host.num_items == 100 and host.is_full()
    # the object owns what it keeps: a caller that reuses its block (already fp32, contiguous, on the device) does not change the kept rows
    reused = torch.from_numpy(blocks[0][:4]).to(DEV)
    own = M.FeatureStats(capture_all=True, device=DEV)
    own.append_torch(reused)
    reused.zero_()
    np.testing.assert_array_equal(own.get_all(), blocks[0][:4])
    assert dev.get_all_torch().device == torch.device(DEV) and dev.get_mean_cov_torch()[1].device == torch.device(DEV)
    np.testing.assert_array_equal(dev.get_all(), host.get_all())
    for a, b in zip(dev.get_mean_cov(), host.get_mean_cov()):
        assert same_bits(a, b)
    for a, b in zip(dev.get_mean_cov_torch(), host.get_mean_cov()):
        assert same_bits(a.cpu().numpy(), b)
    host.save(str(tmp_path / 'host.npz'))
    dev.save(str(tmp_path / 'dev.npz'))
    fh, fd = np.load(tmp_path / 'host.npz'), np.load(tmp_path / 'dev.npz')
    assert sorted(fh.files) == sorted(fd.files)
    for k in fh.files:
        assert fh[k].dtype == fd[k].dtype and np.array_equal(fh[k], fd[k]), k
    for back in (M.FeatureStats.load(tmp_path / 'dev.npz'), M.FeatureStats.load(tmp_path / 'dev.npz', device=DEV)):
        assert back.num_items == 100 and back.is_full()
        np.testing.assert_array_equal(back.get_all(), host.get_all())
        for a, b in zip(back.get_mean_cov(), host.get_mean_cov()):
            assert same_bits(a, b)
    # add_rows: a saved row set in one call
    whole = M.FeatureStats(capture_mean_cov=True, device=DEV)
    whole.add_rows(torch.from_numpy(host.get_all()).to(DEV))
    one = M.FeatureStats(capture_mean_cov=True)
    one.append(host.get_all())
    for a, b in zip(whole.get_mean_cov(), one.get_mean_cov()):
        assert same_bits(a, b)
    assert M.compute_fid(whole, dev) == M.compute_fid(dev.get_mean_cov_torch(), whole.get_mean_cov_torch())


def test_feature_loop_with_device_statistics(tdgp):
    """test_generator_feature_loop's configuration once with host and once with device statistics: identical rows, mean / covariance within
    the rounding bound of two fp64 accumulations of the same rows carried through `central`; fid_for_generator = compute_fid of the stats."""
    from test_gpu_parity import _gen
    M = tdgp.metrics
    tag, cfg = tdgp.config.configs_adaptor_goldens()[0]
    G = _gen(tdgp, cfg, 51)
    det = lambda im: tdgp.distributed.stand_in_features(im, 64)        # noqa: E731
    kw = dict(batch_size=8, batch_gen=4, device=DEV, G_kwargs=dict(noise_mode='const'))

    def run(**more):
        torch.manual_seed(7)
        np.random.seed(7)
        return M.compute_feature_stats_for_generator(G, det, max_items=10, capture_all=True, capture_mean_cov=True, **kw, **more)
    host, dev = run(), run(stats_device=DEV)
    assert host.device is None and dev.device == torch.device(DEV) and dev.num_items == host.num_items == 10 and dev.is_full()
    rows = host.get_all()
    np.testing.assert_array_equal(dev.get_all(), rows)
    (mh, ch), (md, cd) = host.get_mean_cov(), dev.get_mean_cov()
    n = 10
    r = np.abs(rows.astype(np.float64))
    e_s1, e_s2 = 2 * n * U * r.sum(0), 2 * n * U * (r.T @ r)       # both sides are within n u of the exact sums
    e_mu = e_s1 / n + 2 * U * np.abs(mh)                           # ... one division each
    outer = np.abs(np.outer(mh, mh))
    e_outer = np.outer(np.abs(mh), e_mu) + np.outer(e_mu, np.abs(mh)) + np.outer(e_mu, e_mu) + 2 * U * outer
    e_cov = e_s2 / n + 2 * U * (r.T @ r) / n + e_outer + 2 * U * (np.abs(ch) + e_s2 / n + e_outer)
    report_parity('feature loop, device vs host statistics, share of the rounding bound', mean=float((np.abs(md - mh) / np.maximum(e_mu, 1e-300)).max()),
                  cov=float((np.abs(cd - ch) / np.maximum(e_cov, 1e-300)).max()))
    assert (np.abs(md - mh) <= e_mu).all() and (np.abs(cd - ch) <= e_cov).all()
    real = M.FeatureStats(capture_mean_cov=True)
    real.append(rows[::-1] * 0.75 + 0.1)
    torch.manual_seed(7)
    np.random.seed(7)
    got = M.fid_for_generator(G, det, real, num_gen=10, batch_size=8, batch_gen=4, G_kwargs=dict(noise_mode='const'))
    assert np.isfinite(got) and got == M.compute_fid(real, dev)


# ------------------------------------------------------------------------------------------------ the distance
@pytest.mark.parametrize('name', ['full', 'deficient'])
def test_frechet_distance_eigh_on_the_device(tdgp, name):
    """Tolerance: 1e-8 * max(1, |value|), the one test_frechet_distance uses for the eigenvalue form (on the CPU: 4e-14 and 3e-9)."""
    M = tdgp.metrics
    (mu_a, s_a), (mu_b, s_b) = distance_sets()[name]
    ref = M.frechet_distance(mu_a, s_a, mu_b, s_b)
    got = M.frechet_distance_eigh(*(torch.from_numpy(a).to(DEV) for a in (mu_a, s_a, mu_b, s_b)))
    report_parity(f'frechet_distance_eigh on the device vs sqrtm ({name})', value=ref, rel=abs(got - ref) / max(1.0, abs(ref)))
    assert abs(got - ref) <= 1e-8 * max(1.0, abs(ref))

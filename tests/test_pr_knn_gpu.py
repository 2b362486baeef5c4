"""Precision / recall k-NN passes on the GPU (tdgp_pr_pack / tdgp_pr_kth / tdgp_pr_member, csrc/metrics.hip).

Bit-exact part: features are integers in [-4, 4] (times a power of two where the test says so) with F <= 4096, so every dot product and norm
is an integer below 2^24 times that power: exact in fp32 in ANY summation order.  The check is numpy: exact integer d2, np.sqrt in float32,
.astype(float16), np.partition, <=.  kth and membership must equal it bit for bit.

The kernel's tile is 128 x 128 (rows x columns) and a block walks a run of 8 column tiles (1024 columns): the shapes below sit on those
edges -- 1, 3, 127, 128, 129, 257 rows / columns (one partial tile ... three tiles, the last partial) and 1153 / 1202 columns (two runs).

Golden part: compute_pr on the three Gaussian sets of tests/golden/feature_metrics.npz against the reference's own fp16 path.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, report_parity
from test_feature_metrics import feature_rows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EDGES = (1, 3, 127, 128, 129, 257)


# ------------------------------------------------------------------------------------------------ the numpy check
def ref_dist(a, b):
    """fp16 distances [len(a), len(b)] by the contract, from values that are exact in every format involved."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.sqrt(np.maximum(d2, 0.0).astype(np.float32)).astype(np.float16)


def ref_kth(d, k1):
    return np.partition(d.astype(np.float32), k1 - 1, axis=1)[:, k1 - 1].astype(np.float16)        # NaN sorts last


def ref_member(d, kth):
    with np.errstate(invalid='ignore'):
        return (d <= kth[None, :]).any(axis=1)


def lattice(rs, n, F, lo=-4, hi=4):
    return rs.randint(lo, hi + 1, size=(n, F)).astype(np.float32)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint16), want.view(np.uint16))


# ------------------------------------------------------------------------------------------------ the entry points with separate row / column sets
def gpu_kth(tdgp, rows, cols, k1, short_by=0):
    M, L = tdgp.metrics, tdgp._lib
    r, c = M._PackedRows(torch.from_numpy(rows).to(DEV), 'rows'), M._PackedRows(torch.from_numpy(cols).to(DEV), 'cols')
    kth = torch.empty([r.n], dtype=torch.float16, device=DEV)
    need = int(L.load().tdgp_pr_kth_workspace_bytes(r.n, c.n, k1))
    ws = torch.empty([max(need, 16)], dtype=torch.uint8, device=DEV)
    L.call('tdgp_pr_kth', r.half.data_ptr(), r.norms.data_ptr(), r.n, c.half.data_ptr(), c.norms.data_ptr(), c.n, r.half.shape[1], k1, kth.data_ptr(),
           ws.data_ptr(), need - short_by, L.stream_of(kth))
    return kth.cpu().numpy()


def gpu_member(tdgp, probes, cols, kth, short_by=0):
    M, L = tdgp.metrics, tdgp._lib
    p, c = M._PackedRows(torch.from_numpy(probes).to(DEV), 'probes'), M._PackedRows(torch.from_numpy(cols).to(DEV), 'cols')
    k = torch.from_numpy(np.ascontiguousarray(kth)).to(DEV)
    out = torch.empty([p.n], dtype=torch.uint8, device=DEV)
    need = int(L.load().tdgp_pr_member_workspace_bytes(p.n, c.n))
    ws = torch.empty([need], dtype=torch.uint8, device=DEV)
    L.call('tdgp_pr_member', p.half.data_ptr(), p.norms.data_ptr(), p.n, c.half.data_ptr(), c.norms.data_ptr(), k.data_ptr(), c.n, p.half.shape[1],
           out.data_ptr(), ws.data_ptr(), need - short_by, L.stream_of(out))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ bit-exact on the lattice
def test_pack_rounds_pads_and_sums(tdgp):
    rs = np.random.RandomState(0)
    x = (rs.randn(131, 40) * 3).astype(np.float32)
    x[5, 7] = 1e6                                                  # overflows fp16: +inf, as `.to(torch.float16)`
    p = tdgp.metrics._PackedRows(torch.from_numpy(x).to(DEV), 'x')
    h = p.half.cpu().numpy()
    assert h.shape == (131, 64) and not h[:, 40:].any()
    with np.errstate(over='ignore'):
        want = x.astype(np.float16)
    assert same_bits(h[:, :40], want)
    with np.errstate(over='ignore'):
        norms = (want.astype(np.float64) ** 2).sum(1)
    got = p.norms.cpu().numpy().astype(np.float64)
    assert np.isinf(got[5]) and np.allclose(np.delete(got, 5), np.delete(norms, 5), rtol=1e-6, atol=0)      # fp32 sums of 40 terms, any order


@pytest.mark.parametrize('F', [8, 32, 40])
def test_kth_and_membership_at_the_tile_edges(tdgp, F):
    """Every pair of edge sizes, k + 1 in {1, 4, 8} (both list widths of the kernel); F = 8 / 40 pad to 32 / 64, F = 32 does not."""
    rs = np.random.RandomState(F)
    pool_r, pool_c = lattice(rs, max(EDGES), F), lattice(rs, max(EDGES), F)
    pool_c[::5] = pool_r[::5]                                       # shared rows: zero distances and ties
    checked = 0
    for nr in EDGES:
        for nc in EDGES:
            rows, cols = pool_r[:nr], pool_c[:nc]
            d = ref_dist(rows, cols)
            dcc = ref_dist(cols, cols)
            for k1 in (1, 4, 8):
                if k1 > nc:
                    continue
                assert same_bits(gpu_kth(tdgp, rows, cols, k1), ref_kth(d, k1)), (nr, nc, k1)
                kth = ref_kth(dcc, k1)
                assert np.array_equal(gpu_member(tdgp, rows, cols, kth).astype(bool), ref_member(d, kth)), (nr, nc, k1)
                checked += 1
    assert checked == 36 * 3 - 12 - 12                              # k + 1 = 4 and 8 need that many columns: not with 1 or 3


def test_long_k_loop(tdgp):
    """F = 4096: 128 K steps; every sum is still an integer below 2^24 (4096 * 16 * 2 + ...)."""
    rs = np.random.RandomState(1)
    rows, cols = lattice(rs, 257, 4096), lattice(rs, 257, 4096)
    cols[:40] = rows[:40]
    cols[40:80, :7] = rows[40:80, :7] + 1                           # near neighbours at small distances
    cols[40:80, 7:] = rows[40:80, 7:]
    d, dcc = ref_dist(rows, cols), ref_dist(cols, cols)
    for k1 in (1, 4, 8):
        assert same_bits(gpu_kth(tdgp, rows, cols, k1), ref_kth(d, k1)), k1
    kth = ref_kth(dcc, 4)
    want = ref_member(d, kth)
    assert np.array_equal(gpu_member(tdgp, rows, cols, kth).astype(bool), want) and 0 < want.sum() < want.size


@pytest.mark.parametrize('where', ['first_tile', 'one_per_tile', 'last_partial_tile'])
def test_merge_across_tiles_and_runs(tdgp, where):
    """1202 columns = 10 column tiles in two runs of a block (8 + 2), the last tile partial (50 columns).  The k + 1 = 4 nearest columns of row 0
    are planted: all in the first tile, one in each of four tiles (both runs, the partial tile among them), all in the last partial tile --
    the lane lists, the merge through LDS and the merge across runs each have to carry them."""
    rs = np.random.RandomState(2)
    F, nc = 32, 1202
    rows, cols = lattice(rs, 130, F), lattice(rs, nc, F)
    rows[0] = rs.randint(-3, 4, size=F)
    at = dict(first_tile=[3, 40, 77, 127], one_per_tile=[5, 3 * 128 + 64, 8 * 128 + 9, 9 * 128 + 49], last_partial_tile=[1152, 1160, 1190, 1201])[where]
    for n, j in enumerate(at):                                      # distances 1, sqrt 2, sqrt 3, 2 -- far below anything random (about 36)
        cols[j] = rows[0]
        cols[j, :n + 1] += 1
    d = ref_dist(rows, cols)
    want = ref_kth(d, 4)
    assert want[0] == np.float16(2.0) and np.sort(d[0].astype(np.float32))[4] > 8
    for k1 in (1, 2, 3, 4, 8):
        assert same_bits(gpu_kth(tdgp, rows, cols, k1), ref_kth(d, k1)), k1
    kth = ref_kth(ref_dist(cols, cols), 4)
    assert np.array_equal(gpu_member(tdgp, rows, cols, kth).astype(bool), ref_member(d, kth))


def test_duplicates_straddle_the_rank(tdgp):
    """Every row three times: for k + 1 = 4 the distances of a row are 0, 0, 0 and then a group of three equal values -- rank 4 sits inside
    a tie; duplicates count separately, as kthvalue counts them."""
    rs = np.random.RandomState(3)
    base = lattice(rs, 60, 8)
    m = np.repeat(base, 3, axis=0)[rs.permutation(180)]
    d = ref_dist(m, m)
    for k1 in (1, 3, 4, 5, 6, 7):
        got = tdgp.metrics.compute_distances_kth(torch.from_numpy(m).to(DEV), k1 - 1).cpu().numpy()
        assert same_bits(got, ref_kth(d, k1)), k1
    assert not ref_kth(d, 3).any() and ref_kth(d, 4).all()


def test_identical_rows(tdgp):
    m = np.tile(np.array([[1, -2, 3, 0, 4, -4, 2, 1]], np.float32), (200, 1))
    M = tdgp.metrics
    kth = M.compute_distances_kth(torch.from_numpy(m).to(DEV), 3)
    assert kth.dtype == torch.float16 and not kth.cpu().numpy().view(np.uint16).any()
    probes = np.concatenate([m[:5], m[:5] + 1])
    member = M.compute_manifold_membership(torch.from_numpy(probes).to(DEV), torch.from_numpy(m).to(DEV), kth)
    assert member.dtype == torch.bool and member.cpu().tolist() == [True] * 5 + [False] * 5


def test_probe_exactly_on_the_ball(tdgp):
    """`<=`: a probe at exactly kth[j] from column j and inside no other ball is a member; one lattice step further out it is not."""
    rs = np.random.RandomState(4)
    m = lattice(rs, 40, 8, -3, 3)
    kth = ref_kth(ref_dist(m, m), 2)
    found = None
    for j in range(40):
        for _ in range(400):
            p = m[j] + rs.randint(-2, 3, size=8)
            dp = ref_dist(p[None], m)[0]
            hits = dp <= kth
            if np.abs(p).max() <= 4 and hits.sum() == 1 and hits[j] and dp[j] == kth[j]:
                found = (j, p.astype(np.float32))
                break
        if found:
            break
    assert found, 'the seeded search finds such a probe'
    j, p = found
    step = np.sign(p - m[j])
    step[np.abs(p + step) > 4] = 0
    outside = (p + step).astype(np.float32)
    probes = np.stack([p, outside])
    want = ref_member(ref_dist(probes, m), kth)
    assert want.tolist() == [True, False]
    assert gpu_member(tdgp, probes, m, kth).tolist() == [1, 0]


def test_nan_row(tdgp):
    """One NaN row in the manifold: its kth is NaN, it makes no probe a member (itself included), the other rows are unaffected -- and when
    k + 1 equals the row count the NaN distance IS the k + 1-th: NaN for everybody."""
    rs = np.random.RandomState(5)
    m = lattice(rs, 150, 8)
    m[131, 3] = np.nan
    d = ref_dist(m, m)
    want = ref_kth(d, 4)
    got = tdgp.metrics.compute_distances_kth(torch.from_numpy(m).to(DEV), 3).cpu().numpy()
    assert same_bits(got, want) and np.isnan(got[131]) and got.view(np.uint16)[131] == 0x7e00 and np.isfinite(np.delete(got, 131)).all()
    clean = np.delete(m, 131, axis=0)
    assert same_bits(np.delete(got, 131), ref_kth(ref_dist(clean, clean), 4))
    probes = np.concatenate([m, lattice(rs, 20, 8)])
    member = gpu_member(tdgp, probes, m, got).astype(bool)
    assert np.array_equal(member, ref_member(ref_dist(probes, m), want)) and not member[131] and member[:131].all()
    small = m[128:136]                                              # 8 rows, row 3 of them NaN, k + 1 = 8
    assert np.isnan(gpu_kth(tdgp, small, small, 8)).all() and same_bits(gpu_kth(tdgp, small, small, 7), ref_kth(ref_dist(small, small), 7))


def test_overflow_to_inf(tdgp):
    """Lattice times 2^13: distances are 8192 * sqrt(integer), still exact; from 8192 * 8 on they round to +inf.  20 groups of four rows
    one, two and three steps apart and 30 pairs one step apart, the groups far from each other: for k + 1 = 2 every kth is finite, for
    k + 1 = 4 the rows of the pairs get +inf.  inf <= inf is true: with one infinite ball every probe is a member."""
    rs = np.random.RandomState(6)
    base = lattice(rs, 50, 32) * np.float32(8192)
    m = np.concatenate([np.repeat(base[:20], 4, axis=0), np.repeat(base[20:], 2, axis=0)])
    m[:80, 0] += np.float32(8192) * (np.arange(80) % 4)
    m[80:, 0] += np.float32(8192) * (np.arange(60) % 2)
    m = m[rs.permutation(140)]
    d = ref_dist(m, m)
    assert np.isinf(d).any() and np.isfinite(d).any()
    for k1 in (2, 4):
        want = ref_kth(d, k1)
        got = tdgp.metrics.compute_distances_kth(torch.from_numpy(m).to(DEV), k1 - 1).cpu().numpy()
        assert same_bits(got, want), k1
    assert np.isfinite(ref_kth(d, 2)).all() and np.isinf(want).sum() == 60 and np.isfinite(want).sum() == 80
    probes = lattice(rs, 50, 32) * np.float32(8192)
    for kth in (ref_kth(d, 2), want):
        member = gpu_member(tdgp, probes, m, kth).astype(bool)
        assert np.array_equal(member, ref_member(ref_dist(probes, m), kth))
    assert member.all() and not ref_member(ref_dist(probes, m), ref_kth(d, 2)).any()      # an infinite ball holds everybody; the finite ones nobody


def test_same_bytes_twice_and_refusals(tdgp):
    rs = np.random.RandomState(7)
    rows, cols = lattice(rs, 300, 40), lattice(rs, 1153, 40)
    a, b = gpu_kth(tdgp, rows, cols, 4), gpu_kth(tdgp, rows, cols, 4)
    assert a.tobytes() == b.tobytes() and same_bits(a, ref_kth(ref_dist(rows, cols), 4))
    kth = ref_kth(ref_dist(cols, cols), 4)
    ma, mb = gpu_member(tdgp, rows, cols, kth), gpu_member(tdgp, rows, cols, kth)
    assert ma.tobytes() == mb.tobytes() and set(np.unique(ma)) <= {0, 1}
    with pytest.raises(RuntimeError, match='workspace too small'):
        gpu_kth(tdgp, rows, cols, 4, short_by=1)
    with pytest.raises(RuntimeError, match='workspace too small'):
        gpu_member(tdgp, rows, cols, kth, short_by=1)
    with pytest.raises(RuntimeError, match=r'k \+ 1 > Nc'):
        gpu_kth(tdgp, rows, cols[:3], 4)
    with pytest.raises(RuntimeError, match=r'outside \[1, 8\]'):
        gpu_kth(tdgp, rows, cols, 9)


# ------------------------------------------------------------------------------------------------ against the reference golden
def f16_ulp(x):
    return np.spacing(np.asarray(x, np.float64).astype(np.float16)).astype(np.float64)


@pytest.mark.parametrize('index', [0, 1, 2])
def test_compute_pr_against_the_reference(tdgp, index):
    """|ours - reference| <= max(2 x |reference fp16 - reference fp32|, 2 / 600) for precision and recall: the reference's CPU cdist in half is
    itself another rounding of the same distances (two rows of floor), and ours is a third scheme (the factor 2).
    Then every row whose membership differs from a float64 evaluation (of the fp16-rounded features: the contract's inputs) must be
    explained -- some manifold column whose float64 distance is within one fp16 ulp of that column's float64 kth (half an ulp for rounding the
    distance, half for rounding kth) -- and such rows are at most 1 % of all.  Precision and recall lie in (0.1, 0.95): a kernel answering all
    ones or all zeros cannot pass.
    Measured on MI355X, sets 0 / 1 / 2: ours off the reference's fp16 path by 0 / 0 / 0 rows of 600 in precision and 0 / 0 / 1 in recall (the
    reference's own fp16-to-fp32 gap: 0 / 0 / 1 and 0 / 0 / 3 rows); memberships differing from float64: 0 / 0 / 3 of 1200, none unexplained."""
    g = load_golden('feature_metrics')
    real, gen = feature_rows(g, index)
    k = int(g['nhood_size'])
    precision, recall = tdgp.metrics.compute_pr(torch.from_numpy(real).to(DEV), torch.from_numpy(gen).to(DEV), nhood_size=k, row_batch_size=10000,
                                                col_batch_size=10000)
    ref_p, ref_r = (float(v) for v in g['pr_half'][index])
    flt_p, flt_r = (float(v) for v in g['pr_float'][index])
    n = real.shape[0]
    report_parity(f'precision / recall set {index}', precision=precision, recall=recall, ref_precision=ref_p, ref_recall=ref_r,
                  precision_rows_off=round(abs(precision - ref_p) * n), recall_rows_off=round(abs(recall - ref_r) * n))
    print(f'set {index}: ours {precision!r} / {recall!r}, reference half {ref_p!r} / {ref_r!r}, float {flt_p!r} / {flt_r!r}')
    for ours, ref, flt in ((precision, ref_p, flt_p), (recall, ref_r, flt_r)):
        assert 0.1 < ours < 0.95
        assert abs(ours - ref) <= max(2 * abs(ref - flt), 2 / n) + 1e-9
    # float64 on the rounded features
    M = tdgp.metrics
    r64, g64 = real.astype(np.float16).astype(np.float64), gen.astype(np.float16).astype(np.float64)
    unexplained, mismatched = 0, 0
    for manifold32, probes32, m64, p64 in ((real, gen, r64, g64), (gen, real, g64, r64)):
        dist = lambda a, b: np.sqrt(np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None] - 2 * a @ b.T, 0))      # noqa: E731
        kth64 = np.partition(dist(m64, m64), k, axis=1)[:, k]
        dpm = dist(p64, m64)
        want = (dpm <= kth64[None]).any(1)
        mt, pt = M.pack_feature_rows(torch.from_numpy(manifold32).to(DEV)), torch.from_numpy(probes32).to(DEV)       # the manifold packed once
        got = M.compute_manifold_membership(pt, mt, M.compute_distances_kth(mt, k)).cpu().numpy()
        for i in np.nonzero(got != want)[0]:
            mismatched += 1
            if not (np.abs(dpm[i] - kth64) <= f16_ulp(kth64)).any():
                unexplained += 1
    report_parity(f'membership vs float64 set {index}', rows_differing=mismatched, unexplained=unexplained, rows=2 * n)
    print(f'set {index}: {mismatched} of {2 * n} memberships differ from float64, {unexplained} unexplained')
    assert unexplained == 0 and mismatched <= 0.01 * 2 * n


# ------------------------------------------------------------------------------------------------ generator-side wrapper
def test_pr_for_generator(tdgp):
    """pr_for_generator through compute_feature_stats_for_generator with a stand-in generator and detector: the features the detector
    returned, in order, against the real rows given as an array -- the same figures as compute_pr on those rows."""
    from test_feature_metrics import FakeG, RowsDetector
    g = load_golden('feature_metrics')
    real, gen = feature_rows(g, 0)
    M = tdgp.metrics
    got = M.pr_for_generator(FakeG(DEV), RowsDetector(gen, DEV), real, num_gen=gen.shape[0], nhood_size=3, batch_size=64, batch_gen=16)
    want = M.compute_pr(torch.from_numpy(real).to(DEV), torch.from_numpy(gen).to(DEV), nhood_size=3)
    assert got == want and 0.1 < got[0] < 0.95 and 0.1 < got[1] < 0.95

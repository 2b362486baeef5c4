#!/usr/bin/env python3
"""Write tests/golden/instance_selection.npz: what the reference's instance selection computes on two synthetic feature sets (CPU only).

    python tools/gen_instance_selection_goldens.py [--out tests/golden/instance_selection.npz]

The reference (`scripts/data_scripts/run_instance_selection.py:29-33`) scores with scikit-learn:
`GaussianMixture(n_components=1, reg_covar=reg_covar).fit(X).score_samples(X)`, everything else default, on float32 embeddings -- and current
scikit-learn then fits and scores in float32.  Two runs are recorded per case: that one (`scores32`), and the same call on the same values as
float64 (`scores64`), whose distance from the first is the reference's own noise and the yardstick of the tests.

  case 1   [777, 130]  rectified-Gaussian features (mixed through a random matrix, then max(., 0)) with unequal column scales, reg_covar 1e-5
  case 2   [600, 96]   Gaussian features with a mild correlation, reg_covar 0
Both have n > 512 and an F that crosses a 64-column tile edge.  Cuts at keep ratios 0.5 and 0.9 (`int(N * ratio)` images kept).

The tests rely on two facts, asserted here: at every stored cut the float32 and the float64 run select the same set, and the score gap at
the cut is at least 10 x the largest float32-vs-float64 score difference.  A seed that misses them is replaced, never the assertion.
The file holds data only: rows, reg_covar, the two score vectors, the cuts.
"""
import argparse
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = (0.5, 0.9)


def reference_scores(x, reg_covar):
    from sklearn.mixture import GaussianMixture
    gmm = GaussianMixture(n_components=1, reg_covar=reg_covar)
    gmm.fit(x)
    return gmm.score_samples(x)


def closed_form(x, reg_covar, raw_moments):
    """The Gaussian's closed form in float64, covariance centred or from raw moments: printed for the record only."""
    import scipy.linalg
    x = x.astype(np.float64)
    n, f = x.shape
    mu = x.sum(0) / n
    cov = (x.T @ x) / n - np.outer(mu, mu) if raw_moments else ((x - mu).T @ (x - mu)) / n
    cov[np.diag_indices(f)] += reg_covar
    P = scipy.linalg.solve_triangular(scipy.linalg.cholesky(cov, lower=True), np.eye(f), lower=True).T
    y = (x - mu) @ P
    return -0.5 * (f * np.log(2 * np.pi) + (y * y).sum(1)) + np.log(np.diag(P)).sum()


def case_rectified(seed, n=777, f=130):
    rs = np.random.RandomState(seed)
    mix = np.eye(f) + 0.15 * rs.randn(f, f) / np.sqrt(f)
    z = rs.randn(n, f) @ mix + 0.6 * rs.rand(f)
    scales = np.exp(rs.uniform(np.log(0.2), np.log(3.0), size=f))
    return (np.maximum(z, 0.0) * scales).astype(np.float32)


def case_gaussian(seed, n=600, f=96):
    rs = np.random.RandomState(seed)
    mix = np.eye(f) + 0.3 * rs.randn(f, f) / np.sqrt(f)
    return (rs.randn(n, f) @ mix + rs.randn(f)).astype(np.float32)


def check(name, rows, reg_covar):
    s32 = np.asarray(reference_scores(rows, reg_covar), np.float64)
    s64 = reference_scores(rows.astype(np.float64), reg_covar)
    noise = float(np.abs(s32 - s64).max())
    n = rows.shape[0]
    cuts = np.array([int(n * r) for r in RATIOS], np.int64)
    o32, o64 = np.argsort(s32, kind='stable'), np.argsort(s64, kind='stable')
    gaps = []
    for k in cuts:
        assert set(o32[n - k:]) == set(o64[n - k:]), f'{name}: the float32 and float64 runs select different sets at keep = {k}'
        gap = float(s64[o64[n - k]] - s64[o64[n - k - 1]])
        assert gap >= 10 * noise, f'{name}: gap {gap:.3e} at keep = {k} is below 10 x the float32 noise {noise:.3e}: choose another seed'
        gaps.append(gap)
    c, r = closed_form(rows, reg_covar, False), closed_form(rows, reg_covar, True)
    print(f'{name}: rows {rows.shape}, reg_covar {reg_covar:g}, float32-vs-float64 noise {noise:.3e}, gaps at the cuts {gaps}, score range '
          f'{s64.min():.2f} .. {s64.max():.2f}; closed form vs float64 run {np.abs(c - s64).max():.2e}, raw-moment form {np.abs(r - s64).max():.2e}')
    return dict(rows=rows, reg_covar=np.float64(reg_covar), scores32=s32, scores64=s64, cuts=cuts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'instance_selection.npz'))
    args = ap.parse_args(argv)
    cases = dict(case1=check('case1', case_rectified(11), 1e-5), case2=check('case2', case_gaussian(12), 0.0))
    flat = {f'{c}_{k}': v for c, d in cases.items() for k, v in d.items()}
    np.savez_compressed(args.out, **flat)
    size = os.path.getsize(args.out)
    assert size < 1_000_000, size
    print(f'wrote {args.out}: {size} bytes')


if __name__ == '__main__':
    main()

"""Instance selection: the dataset filter behind the reference's ImageNet recipe ("Instance Selection for GANs", arXiv 2007.15255).

Reference: `scripts/data_scripts/run_instance_selection.py` -- fit ONE full-covariance Gaussian to the detector features of a folder (per class
directory with `--subdir_wise`), score every image by its log-likelihood, copy the `num_imgs_to_keep` best.  The reference calls scikit-learn's
`GaussianMixture(n_components=1, reg_covar=...)` on float32 embeddings, which fits and scores in float32.

Here the fit is the closed form it converges to, in fp64 throughout:

    mu = s1 / N,   Sigma = s2 / N - mu mu^T + reg_covar I          (s1, s2: the raw moments of the fp32 rows)
    L L^T = Sigma,  P = L^-T                                          (the "precision Cholesky" factor, upper triangular)
    maha_i = | (x_i - mu) P |^2
    score_i = -0.5 (F log 2 pi + maha_i) + sum log diag P

On a GPU the raw moments come from `tdgp_moments_add` and the Mahalanobis part from `tdgp_gaussian_maha` (csrc/gaussian.hip), both on the fp64
matrix pipe; the factorisation is torch's (`cholesky_ex`, `solve_triangular`) in fp64 on the device.  `device=None` is the same closed form in
numpy / scipy on the host.

The covariance comes from RAW moments: s2 / N and mu mu^T each carry a rounding error of about 2^-53 of their own size, so the difference is
good to about 2^-53 (|mu|^2 + sigma^2) per entry, not 2^-53 sigma^2.  With detector features (non-negative, |mu| of the order of the spread)
that costs nothing measurable -- 2e-13 in the score against scikit-learn's float64 run on the goldens, the centred form 6e-14; for data whose mean is many orders of magnitude
above its spread (|mu| / sigma near 1e6 and beyond) the covariance loses the corresponding digits and the Cholesky factorisation may refuse
it.  Centre such data before scoring.

The Inception detector is a URL-fetched pickle in the reference and is not reproduced: pass `embeddings`, or a `detector` callable.
"""
import math
import os
import shutil

import numpy as np
import torch

CHUNK_ROWS = 1 << 16          # rows per kernel call on the device route: temporaries stay O(chunk); the kernel's bits do not depend on it


# ----------------------------------------------------------------------------------------------------------------------
# scores
# ----------------------------------------------------------------------------------------------------------------------
def _maha_device(rows, mu, P):
    """tdgp_gaussian_maha on device tensors: rows [n, F] fp32 contiguous, mu [F] and P [F, F] fp64 (upper triangular) -> [n] fp64."""
    from . import _lib
    n, width = int(rows.shape[0]), int(rows.shape[1])
    out = torch.empty([n], dtype=torch.float64, device=rows.device)
    if n == 0:
        return out
    ws, need = _lib.byte_workspace('tdgp_gaussian_maha_workspace_bytes', (n, width), rows.device,
                                   RuntimeError(f'tdgp_gaussian_maha refuses {n} rows of {width} features'))
    with torch.cuda.device(rows.device):
        _lib.call('tdgp_gaussian_maha', rows.data_ptr(), n, width, mu.data_ptr(), P.data_ptr(), out.data_ptr(), ws.data_ptr(), need, _lib.stream_of(rows))
    return out


def _not_finite():
    return ValueError('compute_gaussian_ll_scores: the embeddings contain NaN or infinity')


def _not_positive_definite(reg_covar):
    return ValueError(f'compute_gaussian_ll_scores: the covariance of the embeddings is not positive definite with reg_covar = {reg_covar!r} '
                      '(fewer rows than features, or collinear features): increase reg_covar (the reference uses 1e-05 for ImageNet classes)')


def _scores_host(rows, reg_covar):
    import scipy.linalg
    from .metrics import _RawMoments
    n, width = rows.shape
    m = _RawMoments(width)
    for a in range(0, n, CHUNK_ROWS):
        with np.errstate(invalid='ignore', over='ignore'):
            m.add_block(rows[a:a + CHUNK_ROWS])
    if not (np.isfinite(m.s1).all() and np.isfinite(m.s2).all()):
        raise _not_finite()
    mu, cov = m.central(n)
    cov[np.diag_indices(width)] += reg_covar
    try:
        L = scipy.linalg.cholesky(cov, lower=True)
    except np.linalg.LinAlgError:
        raise _not_positive_definite(reg_covar) from None
    P = scipy.linalg.solve_triangular(L, np.eye(width), lower=True).T
    diag = np.diag(P)
    if not (np.isfinite(diag).all() and (diag > 0).all()):
        raise _not_positive_definite(reg_covar)
    log_det = np.log(diag).sum()
    maha = np.empty([n], np.float64)
    for a in range(0, n, CHUNK_ROWS):
        y = (rows[a:a + CHUNK_ROWS].astype(np.float64) - mu) @ P
        maha[a:a + CHUNK_ROWS] = (y * y).sum(axis=1)
    return -0.5 * (width * math.log(2.0 * math.pi) + maha) + log_det


def _scores_device(rows, reg_covar, device):
    from . import _lib
    from .metrics import _DeviceMoments
    _lib.load()
    n, width = int(rows.shape[0]), int(rows.shape[1])

    def chunks():
        for a in range(0, n, CHUNK_ROWS):
            yield a, rows[a:a + CHUNK_ROWS].to(device=device, dtype=torch.float32).contiguous()

    m = _DeviceMoments(width, device)
    for _, block in chunks():
        m.add_block(block)
    if not bool((torch.isfinite(m.s1).all() & torch.isfinite(m.s2).all()).item()):          # the one read-back before the factorisation
        raise _not_finite()
    mu, cov = m.central(n)
    cov.diagonal().add_(float(reg_covar))
    L, info = torch.linalg.cholesky_ex(cov)
    if int(info.item()) != 0:
        raise _not_positive_definite(reg_covar)
    P = torch.linalg.solve_triangular(L, torch.eye(width, dtype=torch.float64, device=device), upper=False).T.contiguous()
    diag = P.diagonal()
    if not bool((torch.isfinite(diag).all() & (diag > 0).all()).item()):
        raise _not_positive_definite(reg_covar)
    log_det = torch.log(diag).sum()
    mu = mu.contiguous()
    scores = torch.empty([n], dtype=torch.float64, device=device)
    for a, block in chunks():
        maha = _maha_device(block, mu, P)
        scores[a:a + block.shape[0]] = -0.5 * (width * math.log(2.0 * math.pi) + maha) + log_det
    return scores


def compute_gaussian_ll_scores(embeddings, reg_covar=0.0, device='cuda'):
    """Log-likelihood of every row of `embeddings` [N, F] under the one full-covariance Gaussian fitted to all of them
    (`run_instance_selection.py:29-33`, scikit-learn's `GaussianMixture(n_components=1, reg_covar=reg_covar).fit(X).score_samples(X)`).

    The rows are taken as fp32 (what the reference's feature extraction stores); everything after that is fp64.  `device`: a GPU -- the raw
    moments and the Mahalanobis part run as HIP kernels on the fp64 matrix pipe, rows pass through in chunks, and the scores come back as an
    fp64 tensor on that device; `device=None` -- numpy / scipy on the host, the scores a numpy array.  Both evaluate the closed form of the
    module docstring; the kernel's arithmetic is stated in include/tdgp.h (tdgp_gaussian_maha).

    The covariance is formed from raw moments, s2 / N - mu mu^T: its entries are good to about 2^-53 (|mu|^2 + sigma^2), which is the fp64
    rounding of the spread itself only while |mu| is not large against the spread (see the module docstring).

    Raises ValueError for non-finite embeddings and for a covariance that is not positive definite (as scikit-learn does)."""
    if isinstance(embeddings, torch.Tensor):
        rows = embeddings
    else:
        rows = np.asarray(embeddings)
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError(f'compute_gaussian_ll_scores: expected [N, F] embeddings, got shape {tuple(rows.shape)}')
    if not (reg_covar >= 0.0):
        raise ValueError(f'compute_gaussian_ll_scores: reg_covar = {reg_covar!r} must be non-negative')
    if rows.shape[0] <= rows.shape[1] and reg_covar == 0:
        # N centred rows span at most N - 1 dimensions: the covariance is singular in exact arithmetic, whatever rounding makes of its last pivots
        raise _not_positive_definite(float(reg_covar))
    if device is None:
        if isinstance(rows, torch.Tensor):
            rows = rows.detach().cpu().numpy()
        return _scores_host(np.ascontiguousarray(rows, dtype=np.float32), float(reg_covar))
    device = torch.device(device)
    if device.type != 'cuda':
        raise ValueError(f'compute_gaussian_ll_scores(device={str(device)!r}): the device route needs a GPU (its kernels have no CPU path); device=None is the host route')
    if not isinstance(rows, torch.Tensor):
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32))
    return _scores_device(rows.detach(), float(reg_covar), device)


compute_gassian_ll_scores = compute_gaussian_ll_scores          # the reference's spelling


def select_instances(scores, num_to_keep):
    """Indices of the `num_to_keep` highest scores in ascending score order: the reference's `np.argsort(scores)[-num_to_keep:]`, with a STABLE
    sort on the scores' own device, so that of equal scores the later rows are kept and the result does not depend on the sort's mood."""
    num_to_keep = int(num_to_keep)
    n = int(scores.shape[0])
    if scores.ndim != 1:
        raise ValueError(f'select_instances: expected [N] scores, got shape {tuple(scores.shape)}')
    if not 0 < num_to_keep <= n:
        raise ValueError(f'select_instances: num_to_keep must be in [1, {n}]: {num_to_keep}')
    if isinstance(scores, torch.Tensor):
        return torch.sort(scores, stable=True).indices[n - num_to_keep:]
    return np.argsort(np.asarray(scores), kind='stable')[n - num_to_keep:]


# ----------------------------------------------------------------------------------------------------------------------
# folders
# ----------------------------------------------------------------------------------------------------------------------
def find_images_in_dir(dir_path):
    """Relative paths of every file under `dir_path` whose extension PIL knows, sorted (`scripts/utils.py:208-216`)."""
    import PIL.Image
    PIL.Image.init()
    names = [os.path.relpath(os.path.join(root, f), start=dir_path) for root, _, files in os.walk(dir_path) for f in files]
    return sorted(f for f in names if os.path.splitext(f)[1].lower() in PIL.Image.EXTENSION)


def extract_embeddings(source_dir, rel_paths, detector, batch_size=256):
    """`detector` on uint8 [B, 3, H, W] batches of the images in order -> [N, F] fp32 (`run_instance_selection.py:80-96` with the detector
    supplied by the caller)."""
    import PIL.Image
    feats = []
    for a in range(0, len(rel_paths), batch_size):
        batch = [np.asarray(PIL.Image.open(os.path.join(source_dir, p)).convert('RGB'), dtype=np.uint8).transpose(2, 0, 1) for p in rel_paths[a:a + batch_size]]
        out = detector(torch.from_numpy(np.stack(batch)))
        feats.append(out.detach().float().cpu().numpy() if isinstance(out, torch.Tensor) else np.asarray(out, dtype=np.float32))
    return np.concatenate(feats, axis=0).astype(np.float32)


def _check_arguments(num_imgs_to_keep, keep_ratio, embeddings, detector):
    if num_imgs_to_keep is None and keep_ratio is None:
        raise ValueError(f'Either num_imgs_to_keep or keep_ratio must be specified: {num_imgs_to_keep}, {keep_ratio}.')
    if num_imgs_to_keep is not None and keep_ratio is not None:
        raise ValueError(f'Only one of num_imgs_to_keep or keep_ratio must be specified: {num_imgs_to_keep}, {keep_ratio}.')
    if num_imgs_to_keep is not None and not num_imgs_to_keep > 0:
        raise ValueError(f'num_imgs_to_keep must be positive: {num_imgs_to_keep}.')
    if keep_ratio is not None and not 0 < keep_ratio <= 1:
        raise ValueError(f'keep_ratio must be in (0, 1]: {keep_ratio}.')
    if (embeddings is None) == (detector is None):
        raise ValueError('Exactly one of embeddings and detector must be given.')


def run_instance_selection(source_dir, output_dir, num_imgs_to_keep=None, keep_ratio=None, subdir_wise=False, reg_covar=0.0, embeddings=None,
                           detector=None, verbose=True, device='cuda'):
    """`run_instance_selection.py:37-76`: copy the `num_imgs_to_keep` (or `int(N * keep_ratio)`) images of `source_dir` with the highest Gaussian
    log-likelihood to the same relative paths under `output_dir`; `subdir_wise` selects inside every immediate subdirectory on its own.

    Exactly one of `embeddings` ([N, F], row i belonging to the i-th path of `find_images_in_dir(source_dir)`) and `detector` (a callable on
    uint8 [B, 3, H, W] batches returning [B, F] features) is given.  `device` is handed to `compute_gaussian_ll_scores`.
    Returns the kept relative paths in ascending score order (per subdirectory, in subdirectory order, with `subdir_wise`)."""
    _check_arguments(num_imgs_to_keep, keep_ratio, embeddings, detector)
    rel_paths = find_images_in_dir(source_dir)
    if embeddings is not None and int(embeddings.shape[0]) != len(rel_paths):
        raise ValueError(f'embeddings has {int(embeddings.shape[0])} rows, {source_dir} has {len(rel_paths)} images')

    if subdir_wise:
        kept = []
        for subdir in sorted(d for d in os.listdir(source_dir) if os.path.isdir(os.path.join(source_dir, d))):
            sub_embeddings = None
            if embeddings is not None:
                rows = [i for i, p in enumerate(rel_paths) if p.split(os.sep, 1)[0] == subdir]
                sub_embeddings = embeddings[rows]
            sub = run_instance_selection(os.path.join(source_dir, subdir), os.path.join(output_dir, subdir), num_imgs_to_keep=num_imgs_to_keep,
                                         keep_ratio=keep_ratio, subdir_wise=False, reg_covar=reg_covar, embeddings=sub_embeddings, detector=detector,
                                         verbose=False, device=device)
            kept += [os.path.join(subdir, p) for p in sub]
        return kept

    total = len(rel_paths)
    keep = int(total * keep_ratio) if num_imgs_to_keep is None else int(num_imgs_to_keep)
    if not 0 < keep <= total:
        raise ValueError(f'num_imgs_to_keep must be in [1, {total}]: {keep}.')
    if verbose:
        print(f'Going to keep {keep}/{total} images.')
    if embeddings is None:
        embeddings = extract_embeddings(source_dir, rel_paths, detector)
    scores = compute_gaussian_ll_scores(embeddings, reg_covar=reg_covar, device=device)
    order = select_instances(scores, keep)
    order = order.cpu().numpy() if isinstance(order, torch.Tensor) else order
    kept = [rel_paths[int(i)] for i in order]
    for p in kept:
        dst = os.path.join(output_dir, p)
        os.makedirs(os.path.dirname(dst) or '.', exist_ok=True)
        shutil.copy(os.path.join(source_dir, p), dst)
    return kept

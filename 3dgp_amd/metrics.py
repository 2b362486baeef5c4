"""FID (feature statistics, Frechet distance), the other feature-space metrics (precision / recall, KID, IS) and camera priors of the generator harness
(host side).

Reference: `src/metrics/metric_utils.py:104-169` (FeatureStats), `:288-320` (compute_feature_stats_for_generator),
`src/metrics/frechet_inception_distance.py:20-39` (compute_fid), `src/training/rendering_utils.py:72-156` (camera priors).

`FeatureStats(device=None)` and `frechet_distance` are the host-side pieces: fp64 mean / covariance accumulation in numpy and
`scipy.linalg.sqrtm`, bit for bit what the golden pins.  `FeatureStats(device=gpu)` keeps the same statistics on the device (fp64 raw moments
on the fp64 matrix pipe, `tdgp_moments_add`, csrc/metrics.hip) and `frechet_distance_eigh` takes the distance from two symmetric eigenproblems
there.  Also here: the
camera prior samplers (torch RNG in the reference's draw order, scipy for the truncated normal).  The device work they drive is
the generator forward (HIP) and ONE all-gather per feature block (`distributed.FeatureGatherer`, RCCL) instead of the
reference's `world` sequential broadcasts.  Precision / recall (`src/metrics/precision_recall.py`) is the exception: its k-NN distance
passes run on the fp16 matrix pipe (`tdgp_pr_kth` / `tdgp_pr_member`, csrc/metrics.hip) and no distance leaves the device.  The Inception detector itself is a URL-fetched TorchScript pickle
(`frechet_inception_distance.py:22`) and is not reproduced: `detector` is any callable `uint8 images [N,3,H,W] -> features [N,F]`.
"""
import numpy as np
import torch

from .generator import TensorGroup


# ----------------------------------------------------------------------------------------------------------------------
# camera priors (configs/camera/base.yaml), rendering_utils.py:72-156
# ----------------------------------------------------------------------------------------------------------------------
def camera_base():
    """configs/camera/base.yaml as a nested dict."""
    return dict(
        ray=dict(start=0.75, end=1.25),
        fov=dict(dist='uniform', min=10.0, max=45.0),
        origin=dict(radius=dict(dist='normal', mean=1.0, std=0.0),
                    angles=dict(dist='truncnorm', yaw=dict(min=-1.57079633, max=1.57079633, mean=0.0, std=0.4),
                                pitch=dict(min=0.392699082, max=2.74889357, mean=1.57, std=0.2))),
        look_at=dict(radius=dict(dist='uniform', min=0.0, max=0.0),
                     angles=dict(dist='spherical_uniform', yaw=dict(min=-3.14159265, max=3.14159265), pitch=dict(min=0.0, max=3.14159265))),
        cube_scale=0.5)


def _g(cfg, path):
    for k in path.split('.'):
        cfg = cfg[k] if isinstance(cfg, dict) else getattr(cfg, k)
    return cfg


def sample_truncnorm(mean, std, lo, hi, batch_size, device):
    """rendering_utils.py:136-142 (scipy's sampler on numpy's global RNG, like the reference)."""
    from scipy.stats import truncnorm
    x = truncnorm.rvs(a=(lo - mean) / std, b=(hi - mean) / std, loc=mean, scale=std, size=(batch_size,))
    return torch.from_numpy(x).float().to(device)


def sample_camera_angles(cfg, batch_size, device):
    """rendering_utils.py:72-109: yaw / pitch / roll = 0 from the configured distribution; pitch clamped to (1e-5, pi - 1e-5)."""
    dist = _g(cfg, 'dist')
    rand = lambda: torch.rand((batch_size, 1), device=device)         # noqa: E731
    randn = lambda: torch.randn((batch_size, 1), device=device)       # noqa: E731
    if dist == 'uniform':
        yaw = rand() * (_g(cfg, 'yaw.max') - _g(cfg, 'yaw.min')) + _g(cfg, 'yaw.min')
        pitch = rand() * (_g(cfg, 'pitch.max') - _g(cfg, 'pitch.min')) + _g(cfg, 'pitch.min')
    elif dist == 'normal':
        yaw = randn() * _g(cfg, 'yaw.std') + _g(cfg, 'yaw.mean')
        pitch = randn() * _g(cfg, 'pitch.std') + _g(cfg, 'pitch.mean')
    elif dist == 'truncnorm':
        yaw = sample_truncnorm((_g(cfg, 'yaw.max') + _g(cfg, 'yaw.min')) * 0.5, _g(cfg, 'yaw.std'), _g(cfg, 'yaw.min'), _g(cfg, 'yaw.max'), batch_size, device).unsqueeze(1)
        pitch = sample_truncnorm((_g(cfg, 'pitch.max') + _g(cfg, 'pitch.min')) * 0.5, _g(cfg, 'pitch.std'), _g(cfg, 'pitch.min'), _g(cfg, 'pitch.max'), batch_size,
                                 device).unsqueeze(1)
    elif dist == 'spherical_uniform':
        yaw_range, yaw_center = _g(cfg, 'yaw.max') - _g(cfg, 'yaw.min'), 0.5 * (_g(cfg, 'yaw.max') + _g(cfg, 'yaw.min'))
        pitch_range, pitch_center = _g(cfg, 'pitch.max') - _g(cfg, 'pitch.min'), 0.5 * (_g(cfg, 'pitch.max') + _g(cfg, 'pitch.min'))
        yaw = (rand() - 0.5) * yaw_range + yaw_center
        v = (rand() - 0.5) * pitch_range + pitch_center
        v = torch.clamp(v / np.pi, 1e-5, 1 - 1e-5)
        pitch = torch.arccos(1 - 2 * v)
    else:
        raise NotImplementedError(f'Unknown distribution: {dist}')
    pitch = torch.clamp(pitch, 1e-5, np.pi - 1e-5)
    return torch.cat([yaw, pitch, torch.zeros_like(yaw)], dim=1)


def sample_bounded_scalar(cfg, batch_size, device):
    """rendering_utils.py:122-132."""
    dist = _g(cfg, 'dist')
    if dist == 'normal':
        assert _g(cfg, 'std') == 0.0, 'Scalar must be bounded'
        return torch.empty(batch_size, device=device, dtype=torch.float32).fill_(_g(cfg, 'mean'))
    if dist == 'truncnorm':
        return sample_truncnorm(_g(cfg, 'mean'), _g(cfg, 'std'), _g(cfg, 'min'), _g(cfg, 'max'), batch_size, device)
    if dist == 'uniform':
        return torch.rand(batch_size, device=device) * (_g(cfg, 'max') - _g(cfg, 'min')) + _g(cfg, 'min')
    raise NotImplementedError(f'Unknown distribution: {dist}')


def sample_camera_params(cfg, batch_size, device='cpu', origin_angles=None):
    """rendering_utils.py:146-152; draw order: origin angles, fov, radius, look-at (angles, radius)."""
    origin_angles = sample_camera_angles(_g(cfg, 'origin.angles'), batch_size, device) if origin_angles is None else origin_angles
    fov = sample_bounded_scalar(_g(cfg, 'fov'), batch_size, device)
    radius = sample_bounded_scalar(_g(cfg, 'origin.radius'), batch_size, device)
    la_angles = sample_camera_angles(_g(cfg, 'look_at.angles'), batch_size, device)
    la_radius = sample_bounded_scalar(_g(cfg, 'look_at.radius'), batch_size, device)
    look_at = torch.cat([la_angles[:, [0, 1]], la_radius.unsqueeze(1)], dim=1)
    return TensorGroup(angles=origin_angles, fov=fov, radius=radius, look_at=look_at)


# ----------------------------------------------------------------------------------------------------------------------
# feature statistics + Frechet distance
# ----------------------------------------------------------------------------------------------------------------------
class _RawMoments:
    """fp64 first and second raw moments (sum of rows, sum of row outer products) of fp32 feature rows.  One block = one
    `rows.sum(0)` and one Gram matrix `rows^T rows` in fp64, added to the running totals: the accumulation order the golden
    `metrics.npz` pins bit for bit (what `metric_utils.py:128-161` computes)."""
    __slots__ = ('s1', 's2')

    def __init__(self, width):
        self.s1 = np.zeros(width, np.float64)
        self.s2 = np.zeros((width, width), np.float64)

    def add_block(self, rows32):
        r = rows32.astype(np.float64)
        self.s1 += r.sum(axis=0)
        self.s2 += r.T @ r

    def central(self, count):
        mu = self.s1 / count
        return mu, self.s2 / count - np.outer(mu, mu)


def _moments_add(rows, s1, s2):
    """s1 += rows.sum(0), s2 += rows^T rows in fp64 for fp32 rows [n, F] on the GPU (tdgp_moments_add: fp64 matrix pipe, contract in
    include/tdgp.h); no read-back, no synchronisation."""
    from . import _lib
    n, width = int(rows.shape[0]), int(rows.shape[1])
    if n == 0:
        return
    ws, need = _lib.byte_workspace('tdgp_moments_workspace_bytes', (n, width), rows.device,
                                   RuntimeError(f'tdgp_moments_add refuses {n} rows of {width} features'))
    with torch.cuda.device(rows.device):
        _lib.call('tdgp_moments_add', rows.data_ptr(), n, width, s1.data_ptr(), s2.data_ptr(), ws.data_ptr(), need, _lib.stream_of(rows))


class _DeviceMoments:
    """`_RawMoments` resident on a GPU: the totals are fp64 tensors there and a block is added by tdgp_moments_add."""
    __slots__ = ('s1', 's2')

    def __init__(self, width, device):
        self.s1 = torch.zeros([width], dtype=torch.float64, device=device)
        self.s2 = torch.zeros([width, width], dtype=torch.float64, device=device)

    def add_block(self, rows32):
        _moments_add(rows32, self.s1, self.s2)

    def central(self, count):
        """The three element-wise fp64 operations of `_RawMoments.central`, one torch op each (nothing fused): equal raw moments give equal bits."""
        count = torch.full([], float(count), dtype=torch.float64, device=self.s1.device)      # a tensor: a Python divisor becomes a multiplication by 1 / count on the GPU
        mu = self.s1 / count
        return mu, self.s2 / count - torch.outer(mu, mu)


class FeatureStats:
    """Feature accumulator of the FID loop; public surface of `metric_utils.py:104-169` (`append`, `append_torch`, `is_full`,
    `get_all`, `get_mean_cov`, `num_items`, `num_features`, `max_items`), written from its behaviour:

    * rows arrive in blocks `[n, F]` and are taken as fp32; F is fixed by the first block;
    * with `max_items` set, a block that would overshoot is cut to the remaining room and later blocks are dropped whole;
    * `capture_all` keeps the accepted rows (in arrival order), `capture_mean_cov` keeps fp64 raw moments (`_RawMoments`);
    * multi-rank: one all-gather per block, rows interleaved rank-major (`distributed.FeatureGatherer`), so that every rank
      accumulates the same sequence and row i of the gathered block came from rank i % world (`metric_utils.py:145-155`).

    `device=None` keeps everything on the host (numpy).  With a GPU device the object lives there: accepted blocks stay device tensors, the raw
    moments are fp64 tensors fed by tdgp_moments_add, and `append_torch` neither copies to the host nor synchronises -- truncation is a slice and
    the counts come from shapes.  The read-outs (`get_all`, `get_mean_cov`, `save`) copy back once; `get_all_torch` / `get_mean_cov_torch`
    return the device tensors.
    """

    def __init__(self, capture_all=False, capture_mean_cov=False, max_items=None, device=None):
        self.capture_all = bool(capture_all)
        self.capture_mean_cov = bool(capture_mean_cov)
        self.max_items = None if max_items is None else int(max_items)
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != 'cuda':
            raise ValueError(f'FeatureStats(device={device!r}): device statistics need a GPU (the moments kernel has no CPU path); device=None is the host object')
        self.num_items = 0
        self.num_features = None
        self._kept = []                  # accepted fp32 blocks (capture_all): numpy arrays, or tensors on `device`
        self._moments = None             # _RawMoments / _DeviceMoments, made when F is known

    # -- bookkeeping --------------------------------------------------------------------------------------------------
    def set_num_features(self, num_features):
        """Fix the feature width F (idempotent; a different F later is an error)."""
        num_features = int(num_features)
        if self.num_features is None:
            self.num_features = num_features
            if self.device is None:
                self._moments = _RawMoments(num_features)
            elif self.capture_mean_cov:
                self._moments = _DeviceMoments(num_features, self.device)
        elif self.num_features != num_features:
            raise AssertionError(f'feature width changed: {self.num_features} -> {num_features}')

    def _room(self):
        return None if self.max_items is None else max(self.max_items - self.num_items, 0)

    def is_full(self):
        return self._room() == 0

    raw_mean = property(lambda self: None if self._moments is None else self._moments.s1)
    raw_cov = property(lambda self: None if self._moments is None else self._moments.s2)

    # -- accumulation -------------------------------------------------------------------------------------------------
    def _append_device(self, rows):
        """`append` for a tensor on `device`: the same cut, count and capture, as a slice and launches on the current stream."""
        if rows.ndim != 2:
            raise AssertionError(f'expected [n, F] feature rows, got shape {tuple(rows.shape)}')
        room = self._room()
        if room is not None and rows.shape[0] > room:
            if room == 0:
                return
            rows = rows[:room]
        source = rows
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        self.set_num_features(rows.shape[1])
        self.num_items += int(rows.shape[0])
        if self.capture_all:
            self._kept.append(rows.clone() if rows.data_ptr() == source.data_ptr() else rows)      # the object owns what it keeps, as the host path's copy does
        if self.capture_mean_cov:
            self._moments.add_block(rows)

    def add_rows(self, x):
        """Accumulate an [N, F] tensor in one call of the moments kernel (real-side statistics from saved features); device statistics only."""
        if self.device is None:
            raise AssertionError('add_rows needs device statistics: FeatureStats(..., device=...)')
        assert isinstance(x, torch.Tensor) and x.ndim == 2
        self._append_device(x)

    def append(self, x):
        if self.device is not None:
            return self._append_device(torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))))
        rows = np.asarray(x, dtype=np.float32)
        if rows.ndim != 2:
            raise AssertionError(f'expected [n, F] feature rows, got shape {rows.shape}')
        room = self._room()
        if room is not None and rows.shape[0] > room:
            if room == 0:
                return                    # already full: the block is dropped before it can fix F
            rows = rows[:room]
        self.set_num_features(rows.shape[1])
        self.num_items += rows.shape[0]
        if self.capture_all:
            self._kept.append(rows)
        if self.capture_mean_cov:
            self._moments.add_block(rows)

    def append_torch(self, x, num_gpus=1, rank=0, gatherer=None):
        """Rows of every rank, interleaved (item i of the gathered block came from rank i % world, :154).  `gatherer`: a
        `distributed.FeatureGatherer` (one all-gather); created on demand when num_gpus > 1."""
        assert isinstance(x, torch.Tensor) and x.ndim == 2
        assert 0 <= rank < num_gpus
        if num_gpus > 1:
            if gatherer is None:
                from .distributed import FeatureGatherer
                gatherer = FeatureGatherer(side_stream=False)
            x = gatherer.gather(x)
        if self.device is not None:
            return self._append_device(x)                 # no host copy, no synchronisation: the fault word is read at the read-outs
        rows = x.cpu().numpy()                            # a synchronisation point: the features are on the host
        if x.is_cuda:
            from . import _lib
            _lib.raise_on_device_fault('the generator forward behind this feature block')
        self.append(rows)

    # -- results ------------------------------------------------------------------------------------------------------
    def _read_back(self, *tensors):
        """Device tensors -> numpy, then the fault word: the copy is the synchronisation point `append_torch` no longer is."""
        out = [t.cpu().numpy() for t in tensors]
        from . import _lib
        _lib.raise_on_device_fault('the generator forwards behind these feature statistics')
        return out

    def get_all_torch(self):
        """metric_utils.py:163-164: the kept rows as one tensor -- on `device` for device statistics, without a copy through the host."""
        if not self.capture_all:
            raise AssertionError('constructed without capture_all')
        if self.device is None:
            return torch.from_numpy(self.get_all())
        return torch.cat(self._kept, dim=0)

    def get_all(self):
        if not self.capture_all:
            raise AssertionError('constructed without capture_all')
        if self.device is not None:
            return self._read_back(self.get_all_torch())[0]
        return np.concatenate(self._kept, axis=0)

    def get_mean_cov_torch(self):
        """(mean, covariance) as fp64 tensors: on `device` for device statistics, nothing read back."""
        if not self.capture_mean_cov:
            raise AssertionError('constructed without capture_mean_cov')
        if self.device is None:
            return tuple(torch.from_numpy(a) for a in self.get_mean_cov())
        return self._moments.central(self.num_items)

    def get_mean_cov(self):
        if not self.capture_mean_cov:
            raise AssertionError('constructed without capture_mean_cov')
        if self.device is not None:
            return tuple(self._read_back(*self._moments.central(self.num_items)))
        return self._moments.central(self.num_items)

    # -- persistence: a neutral container (npz) instead of the reference's pickle of __dict__ ---------------------------
    def save(self, path):
        width = self.num_features or 0
        s1, s2 = (self._moments.s1, self._moments.s2) if self._moments else (np.zeros(width), np.zeros((width, width)))
        if isinstance(s1, torch.Tensor):
            s1, s2 = self._read_back(s1, s2)
        np.savez(path, capture_all=self.capture_all, capture_mean_cov=self.capture_mean_cov, max_items=-1 if self.max_items is None else self.max_items,
                 num_items=self.num_items, raw_mean=s1, raw_cov=s2,
                 all_features=self.get_all() if self.capture_all and self._kept else np.zeros([0, width], np.float32))

    @staticmethod
    def load(path, device=None):
        """`device`: place the loaded totals (and rows) on that GPU; None = the host object."""
        d = np.load(path)
        cap = int(d['max_items'])
        st = FeatureStats(capture_all=bool(d['capture_all']), capture_mean_cov=bool(d['capture_mean_cov']), max_items=None if cap < 0 else cap, device=device)
        st.set_num_features(d['raw_mean'].shape[0])
        st.num_items = int(d['num_items'])
        if st.device is None:
            st._moments.s1[...] = d['raw_mean']
            st._moments.s2[...] = d['raw_cov']
        elif st._moments is not None:
            st._moments.s1.copy_(torch.from_numpy(d['raw_mean']))
            st._moments.s2.copy_(torch.from_numpy(d['raw_cov']))
        if st.capture_all and d['all_features'].size:
            st._kept = [d['all_features'] if st.device is None else torch.from_numpy(d['all_features']).to(st.device)]
        return st


def frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real):
    """frechet_inception_distance.py:35-38."""
    import scipy.linalg
    m = np.square(mu_gen - mu_real).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(sigma_gen, sigma_real), disp=False)
    return float(np.real(m + np.trace(sigma_gen + sigma_real - s * 2)))


def frechet_distance_eigh(mu_gen, sigma_gen, mu_real, sigma_real):
    """The Frechet distance from two symmetric eigenproblems instead of `scipy.linalg.sqrtm` of the non-symmetric product:
    |mu_g - mu_r|^2 + tr S_g + tr S_r - 2 sum_i sqrt(max(lambda_i, 0)), lambda = eigenvalues of S_g^(1/2) S_r S_g^(1/2) (those of S_g S_r).
    S_g^(1/2) comes from one `eigh` with negative eigenvalues clamped to zero; the product is symmetrised before `eigvalsh`.  fp64 tensors or
    arrays; runs on the device of `sigma_gen`.  `frechet_distance` stays the reference's expression and the yardstick."""
    def t(a, device=None):
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))
        return a.to(device=a.device if device is None else device, dtype=torch.float64)
    sg = t(sigma_gen)
    mg, mr, sr = t(mu_gen, sg.device), t(mu_real, sg.device), t(sigma_real, sg.device)
    lam, vec = torch.linalg.eigh(sg)
    root = (vec * lam.clamp_min(0).sqrt()) @ vec.T
    m = root @ sr @ root
    lam2 = torch.linalg.eigvalsh((m + m.T) * 0.5)
    value = (mg - mr).square().sum() + sg.trace() + sr.trace() - 2 * lam2.clamp_min(0).sqrt().sum()
    return float(value)


def _mean_cov_of(stats):
    """(mu, sigma) of a compute_fid argument: a FeatureStats with capture_mean_cov, the path of a saved one, or the pair itself."""
    if isinstance(stats, (str, bytes)) or hasattr(stats, '__fspath__'):
        stats = FeatureStats.load(stats)
    if isinstance(stats, FeatureStats):
        return stats.get_mean_cov_torch() if stats.device is not None else stats.get_mean_cov()
    mu, sigma = stats
    return mu, sigma


def compute_fid(real, gen):
    """frechet_inception_distance.py:20-39 on gathered statistics: `real` / `gen` are FeatureStats with capture_mean_cov, saved paths or
    (mu, sigma) pairs.  Statistics on the host take the reference's expression (`frechet_distance`); when either side is resident on a GPU both
    go there and the distance is `frechet_distance_eigh` on that device, one float read back."""
    (mu_r, sigma_r), (mu_g, sigma_g) = _mean_cov_of(real), _mean_cov_of(gen)
    devices = [a.device for a in (sigma_g, sigma_r) if isinstance(a, torch.Tensor) and a.is_cuda]
    if not devices:
        as_np = lambda a: a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)         # noqa: E731
        return frechet_distance(as_np(mu_g), as_np(sigma_g), as_np(mu_r), as_np(sigma_r))
    on = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))).to(devices[0])      # noqa: E731
    return frechet_distance_eigh(on(mu_g), on(sigma_g), on(mu_r), on(sigma_r))


def iterate_random_conditioning(G, batch_size, device='cpu', camera_cfg=None, dataset=None, frontal_camera=False):
    """metric_utils.py:60-101: endless (c, camera_params) batches.

    Unconditional generator with a parametric camera prior: c is the empty [batch, 0] tensor and cameras come from the prior.
    Otherwise every batch draws `batch_size` dataset indices with `np.random.randint` (one call per item, the reference's draw
    order) and takes labels (`dataset.get_label`) and -- for the 'custom' angle distribution -- camera angles
    (`dataset.get_camera_angles`) from those items.  `dataset` is any object with `__len__`, `get_label`, `get_camera_angles`
    (the reference constructs its ImageFolder dataset here; datasets are out of scope).  `frontal_camera` pins the origin
    angles to (yaw 0, pitch pi/2, roll 0)."""
    camera_cfg = camera_base() if camera_cfg is None else camera_cfg
    custom = _g(camera_cfg, 'origin.angles')['dist'] == 'custom'
    if (G.c_dim != 0 or custom) and dataset is None:
        raise ValueError('a conditional generator / a custom camera distribution draws labels and angles from a dataset')
    frontal = None
    if frontal_camera:
        frontal = torch.stack([torch.zeros(batch_size, device=device), np.pi / 2 + torch.zeros(batch_size, device=device),
                               torch.zeros(batch_size, device=device)], dim=1)
    c0 = torch.zeros([batch_size, 0], device=device) if G.c_dim == 0 else None
    if G.c_dim == 0 and not custom:
        while True:
            yield c0, sample_camera_params(camera_cfg, batch_size, device, origin_angles=frontal)
    while True:
        idx = [np.random.randint(len(dataset)) for _ in range(batch_size)]
        c = c0 if G.c_dim == 0 else torch.from_numpy(np.stack([dataset.get_label(i) for i in idx])).to(device)
        if frontal_camera:
            angles = frontal
        elif custom:
            angles = torch.from_numpy(np.stack([dataset.get_camera_angles(i) for i in idx])).to(device)
        else:
            angles = None
        yield c, sample_camera_params(camera_cfg, len(idx), device, origin_angles=angles)


def _generator_batches(G, batch_gen, camera_cfg, c_sampler, dataset, device, frontal_camera=False):
    """(z, c, camera) batches for the two feature loops below: z first, then the conditioning draw (metric_utils.py:303-307)."""
    if c_sampler is not None:                 # caller-supplied label sampler instead of a dataset
        def cond():
            while True:
                yield c_sampler(batch_gen).to(device), sample_camera_params(camera_base() if camera_cfg is None else camera_cfg, batch_gen, device)
        it = cond()
    else:
        it = iterate_random_conditioning(G, batch_gen, device, camera_cfg, dataset, frontal_camera)
    while True:
        z = torch.randn([batch_gen, G.z_dim], device=device)
        c, camera_params = next(it)
        if getattr(G.synthesis, 'camera_adaptor', None) is not None:
            camera_params = G.synthesis.camera_adaptor(camera_params, z, c)
        yield z, c, camera_params


def resolve_batch_gen(batch_size, batch_gen=None):
    """metric_utils.py:289-290 / :324-325: `min(batch_size, 4) if opts.batch_gen is None else opts.batch_gen`, which must divide batch_size."""
    batch_gen = min(batch_size, 4) if batch_gen is None else int(batch_gen)
    assert batch_gen >= 1 and batch_size % batch_gen == 0
    return batch_gen


def compute_feature_stats_for_generator(G, detector, max_items, batch_size=64, batch_gen=None, camera_cfg=None, c_sampler=None, num_gpus=1, rank=0,
                                        device='cuda', gatherer=None, G_kwargs=None, dataset=None, stats_device=None, **stats_kwargs):
    """metric_utils.py:288-320: generate `batch_size` images per iteration in chunks of `batch_gen`, run the detector, gather the
    feature block across ranks, accumulate.  Conditioning comes from `iterate_random_conditioning` (labels / custom angles from
    `dataset`) or, when given, from `c_sampler(batch) -> c [batch, c_dim]`; cameras come from the prior (`camera_cfg`, default
    camera/base.yaml) and pass through G's camera adaptor when it has one.
    `batch_gen` is the caller's option it is in the reference (MetricOptions.batch_gen, metric_utils.py:26,36): None = the reference's default
    min(batch_size, 4) (:289); 16 generates the same images 8-9 % faster on one MI355X (bench.py --fid-loop prints both).
    `device` is where the draws are made; `stats_device` is FeatureStats' own `device` (None: host statistics, one copy and one
    synchronisation per block; a GPU: the blocks and the moments stay there and the loop never waits for the device)."""
    batch_gen = resolve_batch_gen(batch_size, batch_gen)
    G_kwargs = {} if G_kwargs is None else G_kwargs
    stats = FeatureStats(max_items=max_items, device=stats_device, **stats_kwargs)
    batches = _generator_batches(G, batch_gen, camera_cfg, c_sampler, dataset, device)
    while not stats.is_full():
        images = []
        for _ in range(batch_size // batch_gen):
            z, c, camera_params = next(batches)
            img = G(z, c, camera_params, **G_kwargs)
            images.append((img * 127.5 + 128).clamp(0, 255).to(torch.uint8))
        images = torch.cat(images)
        if images.shape[1] == 1:
            images = images.repeat([1, 3, 1, 1])
        stats.append_torch(detector(images), num_gpus=num_gpus, rank=rank, gatherer=gatherer)
    return stats


def compute_flattened_depth_maps(G, max_items, batch_size=64, batch_gen=None, camera_cfg=None, c_sampler=None, num_gpus=1, rank=0, device='cuda',
                                 gatherer=None, G_kwargs=None, dataset=None, cut_quantile=0.0):
    """metric_utils.py:324-349: frontal-camera depth maps of `max_items` generated samples, flattened to [max_items, h*w]
    (input of the reference's non-flatness score)."""
    batch_gen = resolve_batch_gen(batch_size, batch_gen)
    G_kwargs = {} if G_kwargs is None else G_kwargs
    stats = FeatureStats(max_items=max_items, capture_all=True)
    batches = _generator_batches(G, batch_gen, camera_cfg, c_sampler, dataset, device, frontal_camera=True)
    while not stats.is_full():
        depths = []
        for _ in range(batch_size // batch_gen):
            z, c, camera_params = next(batches)
            out = G(z, c, camera_params, render_opts=dict(return_depth=True, cut_quantile=cut_quantile), **G_kwargs)
            depths.append(out.depth)
        stats.append_torch(torch.cat(depths).flatten(start_dim=1), num_gpus=num_gpus, rank=rank, gatherer=gatherer)
    return torch.from_numpy(stats.get_all())


# ----------------------------------------------------------------------------------------------------------------------
# feature-space metrics: precision / recall, KID, IS (src/metrics/{precision_recall,kernel_inception_distance,inception_score}.py;
# registry entries pr50k3[_full], kid50k[_full], is50k of metric_main.py) on captured feature rows
# ----------------------------------------------------------------------------------------------------------------------
PR_K_STEP = 32                          # halves per K step of the tile loop (csrc/metrics.hip PR_BK): packed rows are padded to a multiple
PR_MAX_NHOOD = 7                        # k + 1 <= 8 sorted entries per lane


class _PackedRows:
    """Feature rows as the k-NN kernels read them: fp16 [N, Fpad] (zero padded) and the fp32 norms of the rounded rows (tdgp_pr_pack)."""
    __slots__ = ('half', 'norms', 'n', 'features')

    def __init__(self, x, what):
        from . import _lib
        _check_rows(x, what)
        _lib.require_cuda(x, what)
        x = _lib.f32c(x)
        self.n, self.features = int(x.shape[0]), int(x.shape[1])
        fpad = -(-self.features // PR_K_STEP) * PR_K_STEP
        self.half = torch.empty([self.n, fpad], dtype=torch.float16, device=x.device)
        self.norms = torch.empty([self.n], dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call('tdgp_pr_pack', x.data_ptr(), self.n, self.features, self.half.data_ptr(), fpad, self.norms.data_ptr(), _lib.stream_of(x))


def _check_rows(x, what):
    if not isinstance(x, torch.Tensor) or x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f'{what}: expected a non-empty [N, F] tensor of feature rows, got {getattr(x, "shape", type(x))}')


def _check_nhood(nhood_size, num_cols):
    nhood_size = int(nhood_size)
    if not 0 <= nhood_size <= PR_MAX_NHOOD:
        raise ValueError(f'nhood_size = {nhood_size} outside [0, {PR_MAX_NHOOD}]')
    if nhood_size + 1 > num_cols:
        raise ValueError(f'nhood_size + 1 = {nhood_size + 1} exceeds the {num_cols} manifold rows (k + 1 > Nc)')
    return nhood_size


def _width(x):
    return x.features if isinstance(x, _PackedRows) else x.shape[1]


def _check_same_width(a, b, what_a, what_b):
    if _width(a) != _width(b):
        raise ValueError(f'feature width mismatch (F): {what_a} has {_width(a)} features, {what_b} has {_width(b)}')


def pack_feature_rows(x, what='features'):
    """Feature rows [N, F] on the GPU -> the packed form the k-NN passes read (fp16 rows and fp32 norms, tdgp_pr_pack).  `compute_distances_kth`
    and `compute_manifold_membership` take it in place of a tensor, so a set used by several calls is packed once."""
    return x if isinstance(x, _PackedRows) else _PackedRows(x, what)


def _pr_kth(manifold, k1):
    from . import _lib
    h = manifold.half
    kth = torch.empty([manifold.n], dtype=torch.float16, device=h.device)
    ws, need = _lib.byte_workspace('tdgp_pr_kth_workspace_bytes', (manifold.n, manifold.n, k1), h.device,
                                   RuntimeError(f'tdgp_pr_kth refuses {manifold.n} rows with k + 1 = {k1}'))
    with torch.cuda.device(h.device):
        _lib.call('tdgp_pr_kth', h.data_ptr(), manifold.norms.data_ptr(), manifold.n, h.data_ptr(), manifold.norms.data_ptr(), manifold.n, h.shape[1], k1,
                  kth.data_ptr(), ws.data_ptr(), need, _lib.stream_of(h))
    return kth


def _pr_member(probes, manifold, kth):
    from . import _lib
    h = probes.half
    member = torch.empty([probes.n], dtype=torch.uint8, device=h.device)
    ws, need = _lib.byte_workspace('tdgp_pr_member_workspace_bytes', (probes.n, manifold.n), h.device,
                                   RuntimeError(f'tdgp_pr_member refuses {probes.n} probes x {manifold.n} manifold rows'))
    with torch.cuda.device(h.device):
        _lib.call('tdgp_pr_member', h.data_ptr(), probes.norms.data_ptr(), probes.n, manifold.half.data_ptr(), manifold.norms.data_ptr(), kth.data_ptr(),
                  manifold.n, h.shape[1], member.data_ptr(), ws.data_ptr(), need, _lib.stream_of(h))
    return member.bool()


def compute_distances_kth(manifold, nhood_size):
    """precision_recall.py:50-54: for every manifold row the (nhood_size + 1)-th smallest fp16 distance to ALL manifold rows (the row itself
    is one of them, duplicates count separately; `dist.kthvalue(nhood_size + 1)`), fp16 [N] on the device.  tdgp_pr_kth: the distances
    live in MFMA accumulators only (contract in include/tdgp.h).  `manifold`: a tensor or `pack_feature_rows` of one."""
    if not isinstance(manifold, _PackedRows):
        _check_rows(manifold, 'manifold')
    nhood_size = _check_nhood(nhood_size, manifold.n if isinstance(manifold, _PackedRows) else manifold.shape[0])
    return _pr_kth(pack_feature_rows(manifold, 'manifold'), nhood_size + 1)


def compute_manifold_membership(probes, manifold, kth):
    """precision_recall.py:55-58: for every probe row whether some manifold row j lies within kth[j] of it, `(dist <= kth).any(dim=1)`;
    bool [Np] on the device (tdgp_pr_member).  `probes` / `manifold`: tensors or `pack_feature_rows` of them."""
    for x, what in ((probes, 'probes'), (manifold, 'manifold')):
        if not isinstance(x, _PackedRows):
            _check_rows(x, what)
    _check_same_width(probes, manifold, 'probes', 'manifold')
    num_cols = manifold.n if isinstance(manifold, _PackedRows) else manifold.shape[0]
    if not isinstance(kth, torch.Tensor) or kth.shape != (num_cols,):
        raise ValueError(f'kth: expected one value per manifold row [{num_cols}], got {getattr(kth, "shape", type(kth))}')
    from . import _lib
    _lib.require_cuda(kth, 'kth')
    return _pr_member(pack_feature_rows(probes, 'probes'), pack_feature_rows(manifold, 'manifold'), kth.to(torch.float16).contiguous())


def compute_pr(real_features, gen_features, nhood_size=3, row_batch_size=None, col_batch_size=None, num_gpus=1, rank=0):
    """precision_recall.py:36-60 on captured feature rows -> (precision, recall): precision is the share of generated rows inside the manifold
    of the real ones (every real row's ball reaches its nhood_size-th neighbour), recall the converse.  GPU only: four tile passes on the
    fp16 matrix pipe, two bytes per row and one byte per probe come out of them, one read-back per value at the end.  `row_batch_size` /
    `col_batch_size` are accepted for the reference's signature and ignored (nothing is materialised, so nothing needs batching).  Rank 0
    computes; the other ranks return NaN as the reference's do."""
    _check_rows(real_features, 'real_features')
    _check_rows(gen_features, 'gen_features')
    _check_same_width(real_features, gen_features, 'real_features', 'gen_features')
    nhood_size = _check_nhood(nhood_size, min(real_features.shape[0], gen_features.shape[0]))
    assert 0 <= rank < num_gpus
    if rank != 0:
        return float('nan'), float('nan')
    real, gen = _PackedRows(real_features, 'real_features'), _PackedRows(gen_features, 'gen_features')
    results = []
    for manifold, probes in ((real, gen), (gen, real)):
        member = _pr_member(probes, manifold, _pr_kth(manifold, nhood_size + 1))
        results.append(member.to(torch.float32).mean())
    precision, recall = (float(v) for v in torch.stack(results).cpu())
    return precision, recall


def _rows_tensor(x, what):
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float32))
    _check_rows(x, what)
    return x.float()


def compute_kid(real_features, gen_features, num_subsets=100, max_subset_size=1000):
    """kernel_inception_distance.py:34-43 on captured feature rows.  The subsets are drawn with `np.random.choice` in the reference's order
    (generated first, then real, per subset), so a seeded host RNG gives the reference's subsets; the three Gram products and the cube are
    fp32 torch ops on the features' device, every sum is taken in fp64, and the total is read back once."""
    real, gen = _rows_tensor(real_features, 'real_features'), _rows_tensor(gen_features, 'gen_features')
    _check_same_width(real, gen, 'real_features', 'gen_features')
    gen = gen.to(real.device)
    n = real.shape[1]
    m = min(min(real.shape[0], gen.shape[0]), int(max_subset_size))
    if m < 2:
        raise ValueError(f'subset size m = {m}: the unbiased estimate divides by m - 1')
    t = torch.zeros([], dtype=torch.float64, device=real.device)
    for _ in range(int(num_subsets)):
        x = gen[torch.from_numpy(np.random.choice(gen.shape[0], m, replace=False)).to(real.device)]
        y = real[torch.from_numpy(np.random.choice(real.shape[0], m, replace=False)).to(real.device)]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum(dtype=torch.float64) - a.diagonal().sum(dtype=torch.float64)) / (m - 1) - b.sum(dtype=torch.float64) * 2 / m
    return float(t.item() / num_subsets / m)


def compute_is(gen_probs, num_splits=10):
    """inception_score.py:30-36 on captured class probabilities [N, classes] -> (mean, std) of exp(mean KL(p(y|x) || p(y))) over `num_splits`
    consecutive parts; the reference's operations in fp64 on the probabilities' device."""
    probs = _rows_tensor(gen_probs, 'gen_probs').double()
    num_gen = probs.shape[0]
    scores = []
    for i in range(int(num_splits)):
        part = probs[i * num_gen // num_splits: (i + 1) * num_gen // num_splits]
        kl = part * (torch.log(part) - torch.log(part.mean(dim=0, keepdim=True)))
        scores.append(torch.exp(kl.sum(dim=1).mean()))
    scores = torch.stack(scores).cpu().numpy()
    return float(np.mean(scores)), float(np.std(scores))


def _real_rows(real):
    """Real-side features of the generator-side wrappers: an [N, F] array / tensor, a FeatureStats with capture_all, or the path of a saved one."""
    if isinstance(real, (str, bytes)) or hasattr(real, '__fspath__'):
        real = FeatureStats.load(real)
    if isinstance(real, FeatureStats):
        real = real.get_all()
    return real if isinstance(real, torch.Tensor) else torch.from_numpy(np.asarray(real, dtype=np.float32))


def _on_generator_device(G, kw):
    """The draws are made where the generator lives, and when that is a GPU the statistics stay there too."""
    kw.setdefault('device', _device_of(G))
    if torch.device(kw['device']).type == 'cuda':
        kw.setdefault('stats_device', kw['device'])


def _checked(G, value):
    """`value` was read back from the device (a synchronisation point): the fault word covers every forward behind it."""
    if _device_of(G).type == 'cuda':
        from . import _lib
        _lib.raise_on_device_fault('the generator forwards behind these feature rows')
    return value


def _generated_rows(G, detector, num_gen, kw):
    _on_generator_device(G, kw)
    stats = compute_feature_stats_for_generator(G, detector, max_items=num_gen, capture_all=True, **kw)
    return stats.get_all_torch()


def fid_for_generator(G, detector, real, num_gen=50000, **kw):
    """'fid50k[_full]' (metric_main.py) for a generator: mean and covariance of the features of `num_gen` generated images
    (`compute_feature_stats_for_generator`, whose keywords `kw` are) against the real-side statistics `real` (a FeatureStats with
    capture_mean_cov, a saved one, or a (mu, sigma) pair) -> the Frechet distance; NaN on ranks other than 0 as in the reference."""
    _on_generator_device(G, kw)
    gen = compute_feature_stats_for_generator(G, detector, max_items=num_gen, capture_mean_cov=True, **kw)
    if kw.get('rank', 0) != 0:
        return float('nan')
    return _checked(G, compute_fid(real, gen))


def pr_for_generator(G, detector, real, num_gen=50000, nhood_size=3, **kw):
    """'pr50k3[_full]' (metric_main.py) for a generator: features of `num_gen` generated images (`compute_feature_stats_for_generator`, whose
    keywords `kw` are) against the captured real features `real` -> (precision, recall).  Datasets are out of scope: `real` is an array or
    a saved FeatureStats."""
    gen = _generated_rows(G, detector, num_gen, kw)
    device = _device_of(G)
    return _checked(G, compute_pr(_real_rows(real).to(device), gen.to(device), nhood_size=nhood_size, num_gpus=kw.get('num_gpus', 1), rank=kw.get('rank', 0)))


def kid_for_generator(G, detector, real, num_gen=50000, num_subsets=100, max_subset_size=1000, **kw):
    """'kid50k[_full]' for a generator -> the KID estimate; NaN on ranks other than 0 as in the reference."""
    gen = _generated_rows(G, detector, num_gen, kw)
    if kw.get('rank', 0) != 0:
        return float('nan')
    device = _device_of(G)
    return _checked(G, compute_kid(_real_rows(real).to(device), gen.to(device), num_subsets=num_subsets, max_subset_size=max_subset_size))


def is_for_generator(G, detector, num_gen=50000, num_splits=10, **kw):
    """'is50k' for a generator whose `detector` returns class probabilities -> (mean, std); NaN on ranks other than 0."""
    probs = _generated_rows(G, detector, num_gen, kw)
    if kw.get('rank', 0) != 0:
        return float('nan'), float('nan')
    return _checked(G, compute_is(probs.to(_device_of(G)), num_splits=num_splits))


# ----------------------------------------------------------------------------------------------------------------------
# non-flatness score (src/metrics/non_flatness_score.py; metric 'nfs256', metric_main.py:118-120)
# ----------------------------------------------------------------------------------------------------------------------
def _depth_histc(depth_maps, bins, lo, hi):
    """[N, pixels] fp32 on the GPU -> [N, bins] int32 counts on the GPU (tdgp_depth_histc: clamp + torch.histc's CPU arithmetic, product before division); no check, no
    read-back."""
    from . import _lib
    _lib.require_cuda(depth_maps, 'depth_maps')
    d = _lib.f32c(depth_maps.flatten(start_dim=1))
    hist = torch.empty([d.shape[0], int(bins)], dtype=torch.int32, device=d.device)
    if d.shape[0]:
        with torch.cuda.device(d.device):
            _lib.call('tdgp_depth_histc', d.data_ptr(), d.shape[0], d.shape[1], float(lo), float(hi), int(bins), hist.data_ptr(), _lib.stream_of(d))
    return hist


def _check_histogram_rows(histograms, pixels, shape):
    """non_flatness_score.py:32-33 with its message: every row must account for every pixel (a NaN or out-of-range depth is in no bin)."""
    counts = histograms.sum(dim=1)
    assert counts.min() == counts.max() == pixels, f"Histograms countain OOB values: {counts.min(), counts.max(), shape}"


@torch.no_grad()
def convert_depth_maps_to_histograms(depth_maps, bins, min, max):       # noqa: A002 (the reference's argument names)
    """non_flatness_score.py:26-35: depth maps [N, pixels] -> fp32 histograms [N, bins] over [min, max], every row checked to sum to `pixels`.
    A CPU tensor takes the reference's own route, one torch.histc per row.  A GPU tensor goes through tdgp_depth_histc in one launch and the
    histograms stay on the device; the kernel applies the score's clamp to [min, max] (non_flatness_score.py:12) itself, so there depths
    outside the range count in the end bins instead of failing the check -- on the clamped maps the score feeds in, the two routes agree
    count for count for any range and bin count the kernel takes (it restates the CPU histc's (x - min) * bins / (max - min) in fp32)."""
    assert depth_maps.ndim == 2, f'Wrong shape: {depth_maps.shape}'
    if depth_maps.is_cuda:
        histograms = _depth_histc(depth_maps, bins, min, max).float()
    else:
        histograms = torch.stack([torch.histc(d, bins, min=min, max=max) for d in depth_maps.float()], dim=0)
    _check_histogram_rows(histograms, depth_maps[0].numel(), depth_maps.shape)
    return histograms


def compute_histogram_entropy(histograms):
    """non_flatness_score.py:39-42, the same three tensor ops on the small [N, bins] fp32 tensor."""
    assert histograms.ndim == 2, f'Wrong shape: {histograms.shape}'
    probs = histograms / histograms.sum(dim=1, keepdim=True)
    return -1.0 * (torch.log(probs + 1e-12) * probs).sum(dim=1)


def _device_of(G):
    params = getattr(G, 'parameters', None)
    p = next(iter(params()), None) if callable(params) else None
    return p.device if p is not None else torch.device(getattr(G, 'device', 'cpu'))


def compute_flatness_score(G, num_gen, min_depth, max_depth, num_bins=64, cut_quantile=0.5, batch_size=64, batch_gen=None, camera_cfg=None, c_sampler=None,
                           dataset=None, num_gpus=1, rank=0, gatherer=None, G_kwargs=None):
    """non_flatness_score.py:9-21: exp(entropy) of the depth histogram of `num_gen` frontal-camera samples rendered with `cut_quantile`, averaged.
    The loop of `compute_flattened_depth_maps` with the same draws in the same order; per batch the depth maps are clamped and reduced to
    histograms where they are (on the GPU: one tdgp_depth_histc launch), and only the [batch, num_bins] block of counts (exact in fp32:
    fewer than 2^24 pixels per map) goes through `FeatureStats.append_torch` -- the rank gather and the host copy."""
    batch_gen = resolve_batch_gen(batch_size, batch_gen)
    G_kwargs = {} if G_kwargs is None else G_kwargs
    device = _device_of(G)
    stats = FeatureStats(max_items=num_gen, capture_all=True)
    batches = _generator_batches(G, batch_gen, camera_cfg, c_sampler, dataset, device, frontal_camera=True)
    pixels = shape = None
    while not stats.is_full():
        depths = []
        for _ in range(batch_size // batch_gen):
            z, c, camera_params = next(batches)
            out = G(z, c, camera_params, render_opts=dict(return_depth=True, cut_quantile=cut_quantile), **G_kwargs)
            depths.append(out.depth)
        depths = torch.cat(depths).flatten(start_dim=1)
        pixels, shape = depths.shape[1], depths.shape
        if depths.is_cuda:
            block = _depth_histc(depths, num_bins, min_depth, max_depth).float()
        else:
            block = torch.stack([torch.histc(d, num_bins, min=min_depth, max=max_depth) for d in depths.float().clamp(min_depth, max_depth)], dim=0)
        stats.append_torch(block, num_gpus=num_gpus, rank=rank, gatherer=gatherer)
    histograms = torch.from_numpy(stats.get_all())
    _check_histogram_rows(histograms, pixels, (histograms.shape[0],) + tuple(shape[1:]))
    return float(compute_histogram_entropy(histograms).exp().mean().item())


def nfs256(G, **kw):
    """The registry entry 'nfs256' (metric_main.py:118-120): 256 samples, depth range = the generator's ray range."""
    return dict(nfs256=compute_flatness_score(G, num_gen=256, min_depth=G.cfg.ray_start, max_depth=G.cfg.ray_end, **kw))


# ----------------------------------------------------------------------------------------------------------------------
# perceptual path length (src/metrics/perceptual_path_length.py; metric 'ppl2_wend', metric_main.py:105-108)
# ----------------------------------------------------------------------------------------------------------------------
def slerp(a, b, t):
    """perceptual_path_length.py:22-31: spherical interpolation of a batch of vectors [B, D] at t [B, 1]; the result has unit length, and
    slerp(a, b, 0) is a / |a|."""
    a = a / a.norm(dim=-1, keepdim=True)
    b = b / b.norm(dim=-1, keepdim=True)
    d = (a * b).sum(dim=-1, keepdim=True)
    p = t * torch.acos(d)
    c = b - d * a
    c = c / c.norm(dim=-1, keepdim=True)
    d = a * torch.cos(p) + c * torch.sin(p)
    return d / d.norm(dim=-1, keepdim=True)


def ppl_ranks(n):
    """(k_lo, k_hi): np.percentile(x, 1, interpolation='lower') is sorted(x)[k_lo] and np.percentile(x, 99, interpolation='higher') is
    sorted(x)[k_hi] for n values -- numpy's float64 virtual index (n - 1) * (q / 100), floored / ceiled."""
    n = int(n)
    assert n >= 1
    k_lo = int(np.floor((n - 1) * (np.float64(1) / 100)))
    k_hi = int(np.ceil((n - 1) * (np.float64(99) / 100)))
    return k_lo, min(k_hi, n - 1)


def _order_statistic(x, k):
    """sorted(x)[k] of a contiguous fp32 GPU vector as a 0-d tensor on the device, exact bits (tdgp_quantile_select with k_lo == k_hi); NaN if
    any element is NaN.  Nothing is read back."""
    from . import _lib, renderer as _renderer
    n = x.numel()
    with torch.cuda.device(x.device):
        need = int(_lib.load().tdgp_quantile_select_workspace_bytes(n))
        if need < 0:
            raise RuntimeError(f'aggregate_ppl: {n} distances outside [1, 2^31 - 1]')
        stream = _lib.stream_of(x)
        ws = _renderer._qs_workspace(x.device, stream, need)
        out = torch.empty(3, dtype=torch.float32, device=x.device)
        _lib.call('tdgp_quantile_select', x.data_ptr(), n, int(k), int(k), 0.0, out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    return out[0]


def aggregate_ppl(dist):
    """perceptual_path_length.py:120-122: the mean of the distances between their 1st percentile (interpolation 'lower') and their 99th
    ('higher'), both ends and every tie with them included.  lo = sorted[k_lo], hi = sorted[k_hi] with `ppl_ranks`; on a GPU tensor the two
    order statistics come from tdgp_quantile_select (exact bits, no sort), the mean is an fp64 masked sum over its count in torch ops on
    the device, and one scalar is read back.  A CPU tensor or array takes the same definition in numpy.
    The reference averages the kept fp32 values in fp32 (`np.mean` of a float32 array); here the mean is taken in fp64.  A NaN distance
    makes the result NaN (np.percentile's answer too)."""
    if isinstance(dist, torch.Tensor) and dist.is_cuda:
        from . import _lib
        d = _lib.f32c(dist.reshape(-1))
        k_lo, k_hi = ppl_ranks(d.numel())
        lo, hi = _order_statistic(d, k_lo), _order_statistic(d, k_hi)
        keep = (d >= lo) & (d <= hi)
        total = torch.where(keep, d.double(), torch.zeros([], dtype=torch.float64, device=d.device)).sum()
        return float((total / keep.sum()).item())
    d = np.asarray(dist.detach().numpy() if isinstance(dist, torch.Tensor) else dist, dtype=np.float32).reshape(-1)
    if np.isnan(d).any():
        return float('nan')
    k_lo, k_hi = ppl_ranks(d.size)
    ordered = np.sort(d)
    lo, hi = ordered[k_lo], ordered[k_hi]
    return float(np.extract(np.logical_and(d >= lo, d <= hi), d).astype(np.float64).mean())


def pair_sqdist(feats, inv_scale, out=None):
    """feats [2n, W] (row i paired with row n + i, what `chunk(2)` splits) -> [n] fp32: sum((a - b)^2) * inv_scale with the difference in fp32
    and its square and the sum in fp64, rounded once (tdgp_pair_sqdist, contract in include/tdgp.h: no full-width temporary, a summation tree
    fixed by W, the same bytes on every run).  `out`: a contiguous fp32 [n] view to write into (any offset into a larger buffer).  A CPU
    tensor takes the same arithmetic in torch ops, in torch's summation order."""
    if not isinstance(feats, torch.Tensor) or feats.ndim != 2 or feats.shape[0] % 2 != 0 or feats.shape[1] < 1:
        raise ValueError(f'pair_sqdist: expected [2n, W] feature rows, got {getattr(feats, "shape", type(feats))}')
    n, width = feats.shape[0] // 2, int(feats.shape[1])
    if out is None:
        out = torch.empty([n], dtype=torch.float32, device=feats.device)
    elif out.shape != (n,) or out.dtype != torch.float32 or out.device != feats.device or not out.is_contiguous():
        raise ValueError(f'pair_sqdist: out must be a contiguous fp32 [{n}] tensor on {feats.device}')
    if not feats.is_cuda:
        a, b = feats.float().chunk(2)
        out.copy_(((a - b).double().square().sum(dim=1) * float(inv_scale)).float())
        return out
    from . import _lib
    feats = _lib.f32c(feats)
    if n == 0:
        return out
    ws, need = _lib.byte_workspace('tdgp_pair_sqdist_workspace_bytes', (n, width), feats.device,
                                   _lib.Unsupported(f'tdgp_pair_sqdist refuses {n} pairs of {width} features'), at_least=16)
    with torch.cuda.device(feats.device):
        _lib.call('tdgp_pair_sqdist', feats.data_ptr(), n, width, float(inv_scale), out.data_ptr(), ws.data_ptr(), need, _lib.stream_of(feats))
    return out


def ppl_image_tail(img, crop, factor):
    """perceptual_path_length.py:71-85 on a CHW image batch in torch ops: centre crop, box mean, [-1, 1] -> [0, 255], grey replicated.  The
    route of a synthesis network that returns images; the renderer's ray-major frames take `renderer.ppl_frames` (one launch)."""
    if crop:
        assert img.shape[2] == img.shape[3]
        c = img.shape[2] // 8
        img = img[:, :, c * 3: c * 7, c * 2: c * 6]
    if factor > 1:
        img = img.reshape([-1, img.shape[1], img.shape[2] // factor, factor, img.shape[3] // factor, factor]).mean([3, 5])
    img = (img + 1) * (255 / 2)
    if img.shape[1] == 1:
        img = img.repeat([1, 3, 1, 1])
    return img


class PPLSampler(torch.nn.Module):
    """perceptual_path_length.py:35-90 for a generator that renders through cameras and sampled rays: one call draws B pairs of latent codes
    epsilon apart and returns their scaled squared detector distances [B] on the device.

    `G`: any module with z_dim, c_dim, img_resolution, img_channels, mapping(z=, c=) and synthesis(ws=, camera_params=, noise_mode=,
    u_coarse=, u_fine=, **G_kwargs); its synthesis exposes `cfg.num_ray_steps` and (optionally) `test_resolution`, which size the renderer
    draws.  The sampler works on a deep copy, so the caller's `noise_const` buffers are never touched.  `detector(img)`: [2B,3,H,W] fp32 in
    [0, 255] -> [2B, W_feat] fp32, built so that the squared L2 distance of two rows is LPIPS (the reference's TorchScript VGG16:
    `lambda x: vgg16(x, resize_images=False, return_lpips=True)`); it stays the caller's.

    Draw order of one call (the reference's, :48-66, then the two this project adds): t; z0, z1; [mapping]; every `.noise_const` buffer in
    named_buffers() order; the camera (when none is passed: one per pair from the prior); u_coarse, u_fine (one set for the B pairs, in
    `renderer.Draws.filled`'s shapes and order).  Both endpoints of a pair are rendered with the same camera and the same draws -- with
    separate draws they would differ by sampling noise, which the division by epsilon^2 turns into the whole result.  The t endpoints and
    the t + epsilon endpoints are rendered as two calls of B images (not one of 2B), so that the two images of a pair pass through the same
    batch position of every kernel: endpoints with bit-identical codes give bit-identical images and a distance of exactly 0.
    `epsilon == 0` (no differential quotient exists) returns the unscaled squared distances."""

    def __init__(self, G, detector, epsilon, space, sampling, crop, camera_cfg=None, G_kwargs=None, target_resolution=256):
        assert space in ['z', 'w']
        assert sampling in ['full', 'end']
        super().__init__()
        import copy
        self.G = copy.deepcopy(G)
        self.detector = detector
        self.epsilon = float(epsilon)
        self.space, self.sampling, self.crop = space, sampling, bool(crop)
        self.camera_cfg = camera_base() if camera_cfg is None else camera_cfg
        self.G_kwargs = {} if G_kwargs is None else dict(G_kwargs)
        self.factor = max(int(self.G.img_resolution) // int(target_resolution), 1)
        opts = self.G_kwargs.get('render_opts', {})
        if float(opts.get('cut_quantile', 0.0)) > 0.0 or any(opts.get(k) for k in ('return_depth', 'return_depth_adapted', 'concat_depth')):
            raise ValueError('PPLSampler renders plain images: no cut_quantile, no depth outputs in G_kwargs["render_opts"]')

    def draw_latents(self, batch, device):
        """:51: z0, z1 = randn([2B, z_dim]).chunk(2)."""
        return torch.randn([batch * 2, self.G.z_dim], device=device).chunk(2)

    def draw(self, c, camera_params=None):
        """Steps 1-6 of a call -> TensorGroup(t [B], z0, ws0, ws1 [B,num_ws,w_dim], camera_params, u_coarse [B,R,S], u_fine [B,R,N])."""
        from . import renderer as _renderer
        G, B, device = self.G, c.shape[0], c.device
        t = torch.rand([B], device=device) * (1 if self.sampling == 'full' else 0)
        z0, z1 = self.draw_latents(B, device)
        if self.space == 'w':
            w0, w1 = G.mapping(z=torch.cat([z0, z1]), c=torch.cat([c, c])).chunk(2)
            ws0 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2))
            ws1 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2) + self.epsilon)
        else:
            zt0 = slerp(z0, z1, t.unsqueeze(1))
            zt1 = slerp(z0, z1, t.unsqueeze(1) + self.epsilon)
            ws0, ws1 = G.mapping(z=torch.cat([zt0, zt1]), c=torch.cat([c, c])).chunk(2)
        for name, buf in G.named_buffers():
            if name.endswith('.noise_const'):
                buf.copy_(torch.randn_like(buf))
        if camera_params is None:
            camera_params = sample_camera_params(self.camera_cfg, B, device)
        if getattr(G.synthesis, 'camera_adaptor', None) is not None:
            camera_params = G.synthesis.camera_adaptor(camera_params, z0, c)
        res = int(getattr(G.synthesis, 'test_resolution', G.img_resolution))
        steps = int(G.synthesis.cfg.num_ray_steps)
        draws = _renderer.Draws(B, res * res).filled(steps, steps, 0.0, device)
        return TensorGroup(t=t, z0=z0, ws0=ws0, ws1=ws1, camera_params=camera_params, u_coarse=draws.t['u_coarse'], u_fine=draws.t['u_fine'])

    def endpoint_images(self, d):
        """Step 7: the 2B detector inputs [2B,3,oh,ow] fp32 in [0, 255], the t endpoints first (`chunk(2)` splits them again)."""
        from . import generator as _generator, renderer as _renderer
        syn = self.G.synthesis
        kw = dict(camera_params=d.camera_params, noise_mode='const', u_coarse=d.u_coarse, u_fine=d.u_fine, **self.G_kwargs)
        if isinstance(syn, _generator.SynthesisNetwork) and d.ws0.is_cuda:
            res = syn.train_resolution if syn.training else syn.test_resolution
            frames = torch.cat([syn(ws=ws, ray_major=True, **kw).rgb for ws in (d.ws0, d.ws1)])
            return _renderer.ppl_frames(frames, res, res, crop=self.crop, factor=self.factor)
        return ppl_image_tail(torch.cat([syn(ws=ws, **kw) for ws in (d.ws0, d.ws1)]), self.crop, self.factor)

    @torch.no_grad()
    def forward(self, c, camera_params=None, out=None):
        d = self.draw(c, camera_params)
        feats = self.detector(self.endpoint_images(d))
        inv_scale = 1.0 / (self.epsilon * self.epsilon) if self.epsilon != 0.0 else 1.0
        return pair_sqdist(feats, inv_scale, out=out)


def compute_ppl(G, detector, num_samples, epsilon, space, sampling, crop, batch_size, camera_cfg=None, c_sampler=None, dataset=None, num_gpus=1, rank=0,
                gatherer=None, device='cuda', G_kwargs=None):
    """perceptual_path_length.py:94-123: `num_samples` path-length samples in batches of `batch_size` pairs per rank -> `aggregate_ppl` of them.
    Labels (and, with them, the cameras of the prior or the dataset's custom angles) come from `iterate_random_conditioning`; with
    `c_sampler(batch) -> c` the sampler draws the cameras itself.  One sampler call per iteration; the [batch] block of every rank is
    appended in rank order (:109-113; `gatherer`: a `distributed.FeatureGatherer`, created on demand when num_gpus > 1) into one preallocated
    device buffer, which is cut to `num_samples` at the end.  Nothing crosses to the host inside the loop; `aggregate_ppl` reads one number
    back.  Ranks other than 0 return NaN."""
    assert 0 <= rank < num_gpus
    num_samples, batch_size = int(num_samples), int(batch_size)
    assert num_samples >= 1 and batch_size >= 1
    device = torch.device(device)
    sampler = PPLSampler(G, detector, epsilon, space, sampling, crop, camera_cfg=camera_cfg, G_kwargs=G_kwargs)
    sampler.eval().requires_grad_(False).to(device)
    if c_sampler is not None:
        def cond():
            while True:
                yield c_sampler(batch_size).to(device), None
        cond = cond()
    else:
        cond = iterate_random_conditioning(G, batch_size, device, camera_cfg, dataset)
    if num_gpus > 1 and gatherer is None:
        from .distributed import FeatureGatherer
        gatherer = FeatureGatherer(side_stream=False)
    step = batch_size * num_gpus
    dist = torch.empty([-(-num_samples // step) * step], dtype=torch.float32, device=device)
    for start in range(0, num_samples, step):
        c, camera_params = next(cond)
        if num_gpus == 1:
            sampler(c, camera_params, out=dist[start:start + batch_size])
            continue
        x = gatherer.gather(sampler(c, camera_params).unsqueeze(1))          # [batch * world, 1], row i from rank i % world
        dist[start:start + step] = x.reshape(batch_size, num_gpus).t().reshape(-1)      # -> the ranks' blocks one after the other
    if rank != 0:
        return float('nan')
    return aggregate_ppl(dist[:num_samples])


def ppl_for_generator(G, detector, num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2, **kw):
    """A perceptual path length of a generator (`compute_ppl`, whose keywords `kw` are), drawn and kept where the generator lives; NaN on
    ranks other than 0 as in the reference."""
    kw.setdefault('device', _device_of(G))
    value = compute_ppl(G, detector, num_samples, epsilon, space, sampling, crop, batch_size, **kw)
    return value if kw.get('rank', 0) != 0 else _checked(G, value)


def ppl2_wend(G, detector, **kw):
    """The registry entry 'ppl2_wend' (metric_main.py:105-108): 50 000 samples, epsilon 1e-4, W space, end points, no crop, 2 pairs per batch."""
    args = dict(num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2)
    args.update(kw)
    return dict(ppl2_wend=ppl_for_generator(G, detector, **args))

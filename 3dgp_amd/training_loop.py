"""The training driver: dataset, networks, phases, ticks, image / network snapshots, metrics and resume.

Follows the reference's `src/training/training_loop.py:70-560` in its order on top of the pieces of `training.py` (`setup_phases`,
`train_iteration`, `update_ema`, `StyleGAN2Loss`, `AdaController`), `augment.AugmentPipe`, `dataset.py` and `step_tail.py`.
`tools/train.py` is its command line.

What differs from the reference, on purpose:
  * a network snapshot is a DIRECTORY `network-snapshot-{kimg:06d}/`: `generator.json` + `generator.npz` hold G_ema in the exported format
    `weights.load_exported` reads (every tool of this repository takes it as it is), `augment_pipe.json` / `.npz` the pipe, and
    `training_state.pt` (one `torch.save`) everything resume needs.  There is no pickle of module objects;
  * the loss statistics of a tick are summed on the device and read back once per tick (the reference's collector synchronises per report);
  * the best-metric bookkeeping acts only on ticks that evaluated a metric (the reference compares inf <= inf on the others and so
    saves a snapshot on every tick of a run without metrics);
  * a generator with `camera_cond=True` is refused at construction: `StyleGAN2Loss.run_G` does not pass camera angles to the mapping
    network, the run would fail -- or silently train another model -- in its first step;
  * not built: path-length regularisation, style mixing, tensorboard, restoring RNG streams on resume (the reference does not either).
"""
import copy
import dataclasses
import json
import os
import shutil
import time
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np
import torch

from . import training as TR
from .config import GeneratorConfig
from .generator import TensorGroup


def _adam():
    return dict(lr=0.002, betas=[0.0, 0.99], eps=1e-8)


@dataclass
class TrainingOptions:
    """Everything a run is defined by; `from_dict` / `to_dict` round-trip through yaml (`tools/train.py --config`)."""
    data: Optional[str] = None                    # directory or zip (dataset.ImageFolderDataset)
    resolution: Optional[int] = None
    use_depth: bool = False
    mirror: bool = False
    max_size: Optional[int] = None
    use_embeddings: bool = False
    embeddings_path: Optional[str] = None
    embeddings_desc_path: Optional[str] = None
    workers: int = 3
    camera: Optional[dict] = None                 # the `camera:` config node (metrics.camera_base() when None)
    generator: Optional[dict] = None              # GeneratorConfig fields (weights.config_from_json layout); None with `resume`
    discriminator: dict = field(default_factory=dict)          # DiscriminatorConfig fields
    resume: Optional[str] = None                  # snapshot directory (or any exported checkpoint directory: fine-tuning)
    resume_whole_state: bool = False
    resume_optim: bool = True
    seed: int = 0
    batch_size: int = 32
    batch_gpu: Optional[int] = None               # per-rank sub-batch; None = batch_size // world
    G_opt: dict = field(default_factory=lambda: dict(_adam(), lr=0.0025))
    D_opt: dict = field(default_factory=_adam)
    G_reg_interval: Optional[int] = None
    D_reg_interval: Optional[int] = 16
    grad_clip: Optional[float] = None
    r1_gamma: float = 10.0
    patch: Optional[dict] = None                  # training.PatchConfig fields; None = whole images
    loss: dict = field(default_factory=dict)      # further StyleGAN2Loss arguments (blur_init_sigma, kd_weight, adv_loss_type, ...)
    learn_camera_dist: bool = False
    camera_reg: Optional[dict] = None             # training.CameraRegConfig fields (prior defaults to `camera`)
    augment: dict = field(default_factory=lambda: dict(mode='noaug'))   # mode noaug | ada | fixed; p, target, interval, kimg, pipe={AugmentPipe arguments}
    ema_kimg: float = 10.0
    ema_rampup: Optional[float] = 0.05
    ema_start_kimg: float = 0.0
    total_kimg: float = 25000
    kimg_per_tick: float = 4
    snap: int = 50                                # network snapshot every `snap` ticks
    image_snap: Optional[int] = 50                # image snapshot every `image_snap` ticks (None: never)
    val_freq: int = 50                            # metrics every `val_freq` ticks
    metrics: Any = field(default_factory=list)    # names (resolved by `resolve_metric`) or a mapping name -> callable(G_ema) -> float
    metric_kwargs: dict = field(default_factory=dict)          # name -> keyword arguments, e.g. {'nfs256': {'num_gen': 64}}
    grid: list = field(default_factory=lambda: [8, 4])         # image snapshot grid (columns, rows), cut to the dataset's size
    num_videos: int = 16
    video_frames: int = 32
    test_batch_gpu: int = 4
    fused_step_tail: bool = True                  # step_tail.FusedStepTail / fused_update_ema instead of optimizer_step / update_ema
    device: str = 'cuda'

    def to_dict(self):
        d = dataclasses.asdict(self)
        if not isinstance(self.metrics, (list, tuple)):
            d['metrics'] = list(self.metrics)                  # callables do not serialise: their names
        return d

    @classmethod
    def from_dict(cls, d):
        known = {f.name for f in dataclasses.fields(cls)}
        unknown = sorted(set(d) - known)
        if unknown:
            raise KeyError(f'unknown training option(s): {unknown}')
        return cls(**copy.deepcopy(dict(d)))

    def to_yaml(self):
        import yaml
        return yaml.safe_dump(self.to_dict(), sort_keys=False)

    @classmethod
    def from_yaml(cls, text):
        import yaml
        return cls.from_dict(yaml.safe_load(text) or {})


def apply_overrides(d, overrides):
    """`key=value` / `key.sub=value` strings (values parsed as yaml) onto a nested dict; a top-level key TrainingOptions does not have is an error."""
    import yaml
    known = {f.name for f in dataclasses.fields(TrainingOptions)}
    for item in overrides:
        key, sep, value = item.partition('=')
        if not sep:
            raise ValueError(f'override {item!r} is not key=value')
        path = key.split('.')
        if path[0] not in known:
            raise KeyError(f'unknown training option: {path[0]}')
        node = d
        for k in path[:-1]:
            if not isinstance(node.get(k), dict):
                node[k] = {}
            node = node[k]
        node[path[-1]] = yaml.safe_load(value)
    return d


# ----------------------------------------------------------------------------------------------------------------------
# the parts of a run (module-level so that a test can put a stub in the place of any of them)
# ----------------------------------------------------------------------------------------------------------------------
def camera_cfg_of(opts):
    from .metrics import camera_base
    return camera_base() if opts.camera is None else opts.camera


def build_training_set(opts, rank, world, c_dim):
    """training_loop.py:95-100: dataset, sampler sharded by rank, batches of batch_size // world."""
    from . import dataset as DS
    ds = DS.ImageFolderDataset(opts.data, resolution=opts.resolution, use_depth=opts.use_depth, max_size=opts.max_size, mirror=opts.mirror, c_dim=c_dim,
                               use_embeddings=opts.use_embeddings, embeddings_path=opts.embeddings_path, embeddings_desc_path=opts.embeddings_desc_path,
                               camera_cfg=camera_cfg_of(opts), random_seed=opts.seed)
    sampler = DS.InfiniteSampler(ds, rank=rank, num_replicas=world, seed=opts.seed)
    return ds, DS.batch_iterator(ds, sampler, opts.batch_size // world, workers=opts.workers, pin_memory=str(opts.device).startswith('cuda'))


def generator_config(opts):
    """GeneratorConfig of the run: `opts.generator`, or the resumed checkpoint's; `camera_cond` is refused here, before anything is built."""
    from . import weights
    if opts.generator is not None:
        cfg = opts.generator if isinstance(opts.generator, GeneratorConfig) else weights.config_from_json(opts.generator)
    elif opts.resume is not None:
        cfg = weights.load_exported(opts.resume)[0]
    else:
        raise ValueError('TrainingOptions needs `generator` (a GeneratorConfig as a dict) or `resume`')
    if cfg.camera_cond:
        raise NotImplementedError('training a generator with camera_cond=True is not built: StyleGAN2Loss.run_G does not pass camera angles to the '
                                  'mapping network')
    patch = opts.patch or {}
    if patch.get('enabled', bool(opts.patch)):
        cfg = dataclasses.replace(cfg, patch_resolution=int(patch['resolution']))
    return cfg


def build_networks(opts, cfg, training_set, device):
    """training_loop.py:108-127: G, D, G_ema; resumed parameters when `opts.resume` names a snapshot."""
    from . import weights
    from .discriminator import Discriminator, DiscriminatorConfig
    from .generator import Generator
    if training_set.resolution != cfg.img_resolution:
        raise ValueError(f'dataset resolution {training_set.resolution} != generator resolution {cfg.img_resolution}')
    patch = opts.patch or {}
    patched = patch.get('enabled', bool(opts.patch))
    dcfg = DiscriminatorConfig(**dict(dict(c_dim=cfg.c_dim, patch_params_cond=patched), **opts.discriminator))
    if patched and 'mbstd_group_size' not in opts.discriminator and 'mbstd_group_size' in patch:
        dcfg.mbstd_group_size = int(patch['mbstd_group_size'])
    G = Generator(cfg, img_resolution=training_set.resolution, img_channels=training_set.num_channels)
    D = Discriminator(dcfg, input_resolution=int(patch['resolution']) if patched else training_set.resolution,
                      img_channels=training_set.num_channels + (1 if opts.use_depth else 0))
    G_ema = None
    state = None
    if opts.resume is not None:
        _, sd = weights.load_exported(opts.resume)
        G.load_numpy_state_dict(sd)
        G_ema = copy.deepcopy(G)
        sp = os.path.join(opts.resume, 'training_state.pt')
        if os.path.exists(sp):
            state = torch.load(sp, map_location='cpu', weights_only=False)
            _load_state(G, state['G'])
            _load_state(D, state['D'])
        elif opts.resume_whole_state:
            raise FileNotFoundError(f'{sp}: resume_whole_state needs a snapshot written by training_loop')
    G = G.train().requires_grad_(False).to(device)
    D = D.train().requires_grad_(False).to(device)
    G_ema = (copy.deepcopy(G) if G_ema is None else G_ema.to(device)).eval().requires_grad_(False)
    return G, D, G_ema, state


def _load_state(module, sd):
    """`load_state_dict` that takes a tensor whose shape differs only by unit dimensions (the depth adaptor's `progress_coef` is registered as
    [1] and becomes a scalar on its first progressive_update, as in the reference)."""
    own = module.state_dict()
    module.load_state_dict({k: (v.reshape(own[k].shape) if k in own and v.shape != own[k].shape and v.numel() == own[k].numel() else v) for k, v in sd.items()})


def build_augment(opts, device, state):
    """training_loop.py:159-171 -> (pipe, controller) or (None, None)."""
    a = dict(opts.augment or {})
    mode = a.get('mode', 'noaug')
    if mode == 'noaug':
        return None, None
    if mode not in ('ada', 'fixed'):
        raise ValueError(f'augment.mode must be noaug, ada or fixed, got {mode!r}')
    from .augment import AugmentPipe
    pipe = AugmentPipe(**a.get('pipe', {})).train().requires_grad_(False).to(device)
    pipe.p.copy_(torch.as_tensor(float(a.get('p', 0.0))))
    if state is not None and opts.resume_whole_state and state.get('augment_p') is not None:
        pipe.p.copy_(torch.as_tensor(state['augment_p']))
    ada = TR.AdaController(pipe, target=a.get('target', 0.6), interval=a.get('interval', 4), kimg=a.get('kimg', 500)) if mode == 'ada' else None
    return pipe, ada


def build_loss(opts, G, D, pipe, device):
    patch_cfg = TR.PatchConfig(**opts.patch) if opts.patch else None
    reg = None
    if opts.learn_camera_dist:
        reg = TR.CameraRegConfig(**dict(dict(prior=camera_cfg_of(opts)), **(opts.camera_reg or {})))
    return TR.StyleGAN2Loss(G, D, device, r1_gamma=opts.r1_gamma, patch_cfg=patch_cfg, use_depth=opts.use_depth, learn_camera_dist=opts.learn_camera_dist,
                            camera_reg=reg, augment_pipe=pipe, **opts.loss)


class TickStats(dict):
    """`loss.stats` for the driver: the SUM of every value the loss reports is kept on the device (one reduction and one add per report,
    nothing copied either way), its COUNT -- a property of the shape -- on the host; `collect` reads the sums back with one copy per tick
    and clears them."""

    def __init__(self):
        super().__init__()
        self.sums, self.counts = {}, {}

    def __setitem__(self, key, value):
        super().__setitem__(key, value)
        if isinstance(value, torch.Tensor):
            total, n = value.detach().sum(dtype=torch.float32), value.numel()
        else:
            total, n = float(value), 1
        self.sums[key] = total if key not in self.sums else self.sums[key] + total
        self.counts[key] = self.counts.get(key, 0) + n

    def collect(self):
        keys = sorted(self.sums)
        on_device = [k for k in keys if isinstance(self.sums[k], torch.Tensor)]
        host = {k: float(self.sums[k]) for k in keys if k not in on_device}
        if on_device:
            device = self.sums[on_device[0]].device
            host.update(zip(on_device, torch.stack([self.sums[k].to(device) for k in on_device]).cpu().tolist()))      # the one read-back of the tick
        out = {k: dict(num=self.counts[k], mean=(host[k] / self.counts[k] if self.counts[k] else float('nan'))) for k in keys}
        self.sums, self.counts = {}, {}
        return out


def fetch(opts, iterator, training_set, G, phases, device):
    """training_loop.py:293-320: one real batch and `len(phases) * batch_size` generator inputs."""
    from .metrics import _g, sample_camera_params
    batch = next(iterator)
    to = lambda t: t.to(device, non_blocking=True)                     # noqa: E731
    real = TensorGroup(img=to(batch['image']).to(torch.float32) / 127.5 - 1.0, c=to(batch['label']).to(torch.float32),
                       camera_angles=to(batch['camera_angles']), depth=to(batch['depth']).to(torch.float32) / 65536 * 2.0 - 1.0,
                       embs=to(batch['embedding']).to(torch.float32))
    n = len(phases) * opts.batch_size
    z = torch.randn([n, G.z_dim], device=device)
    idx = [np.random.randint(len(training_set)) for _ in range(n)]
    c = torch.from_numpy(np.stack([training_set.get_label(i) for i in idx])).to(device)
    cam = camera_cfg_of(opts)
    angles = None
    if _g(cam, 'origin.angles')['dist'] == 'custom':
        angles = torch.from_numpy(np.stack([training_set.get_camera_angles(i) for i in idx])).to(device)
    return real, TensorGroup(z=z, c=c, camera_params=sample_camera_params(cam, n, device, origin_angles=angles))


def run_batch(opts, loss, phases, real, gen, G, G_ema, batch_idx, cur_nimg, world, ada):
    """training_loop.py:319-367: the phases, then the EMA update (with the fused tail: four launches per phase and one for the EMA)."""
    TR.train_iteration(loss, phases, real, gen, batch_idx=batch_idx, cur_nimg=cur_nimg, batch_size=opts.batch_size,
                       batch_gpu=opts.batch_gpu or opts.batch_size // world, world=world, grad_clip=opts.grad_clip, ada=ada,
                       step_tail=bool(opts.fused_step_tail))
    kw = dict(ema_kimg=opts.ema_kimg, ema_rampup=opts.ema_rampup, ema_start_kimg=opts.ema_start_kimg)
    if opts.fused_step_tail:
        from .step_tail import fused_update_ema
        return fused_update_ema(G_ema, G, cur_nimg, opts.batch_size, **kw)
    return TR.update_ema(G_ema, G, cur_nimg, opts.batch_size, **kw)


def resolve_metric(name, opts, training_set):
    """A registry name -> callable(G_ema) -> float.  'nfs256' is metrics.nfs256's loop with an overridable `num_gen`."""
    if name == 'nfs256':
        from .metrics import compute_flatness_score
        kw = dict(dict(num_gen=256, batch_gen=opts.test_batch_gpu), **opts.metric_kwargs.get(name, {}))

        def nfs(G_ema):
            with torch.no_grad():
                return compute_flatness_score(G_ema, min_depth=G_ema.cfg.ray_start, max_depth=G_ema.cfg.ray_end, camera_cfg=camera_cfg_of(opts),
                                              dataset=training_set, **kw)
        return nfs
    raise KeyError(f'unknown metric {name!r}: pass a callable in TrainingOptions.metrics')


# ----------------------------------------------------------------------------------------------------------------------
# snapshots
# ----------------------------------------------------------------------------------------------------------------------
def image_grid_u8(images, gw, gh):
    """uint8 [N, C, H, W] (N <= gw * gh, C 1 or 3) -> [1, gh * H, gw * W, 3], row-major tiles, missing tiles black."""
    images = np.asarray(images)
    N, C, H, W = images.shape
    if C == 1:
        images = np.repeat(images, 3, axis=1)
    out = np.zeros([gh * H, gw * W, 3], dtype=np.uint8)
    for i in range(min(N, gw * gh)):
        y, x = divmod(i, gw)
        out[y * H:(y + 1) * H, x * W:(x + 1) * W] = images[i].transpose(1, 2, 0)
    return out[None]


def setup_snapshot_grid(opts, training_set, G, device):
    """The fixed visualisation inputs (training_loop.py:226-236): a seeded choice of real items, one z per item, their labels permuted, their
    camera angles under the 'custom' distribution and prior draws otherwise."""
    from .metrics import _g, sample_camera_params
    gw, gh = (int(v) for v in opts.grid)
    rnd = np.random.RandomState(opts.seed)
    order = np.arange(len(training_set))
    rnd.shuffle(order)
    idx = [int(order[i % len(order)]) for i in range(min(gw * gh, len(order)))]
    gh = -(-len(idx) // gw)
    items = [training_set[i] for i in idx]
    cam = camera_cfg_of(opts)
    angles = None
    if _g(cam, 'origin.angles')['dist'] == 'custom':
        angles = torch.from_numpy(np.stack([it['camera_angles'] for it in items]))
    labels = np.stack([it['label'] for it in items])
    vis = dict(grid_size=[gw, gh], z=torch.randn([len(idx), G.z_dim], device=device).cpu(), c=torch.from_numpy(rnd.permutation(labels)),
               camera_params=dict(sample_camera_params(cam, len(idx), 'cpu', origin_angles=angles)))
    reals = np.stack([it['image'] for it in items])
    depth = np.stack([it['depth'] for it in items]) if opts.use_depth else None
    return vis, reals, depth


def save_image_snapshot(opts, run_dir, name, vis, G_ema, device):
    """fakes grid (+ depth when the generator returns one) and the video grid of the first `num_videos` samples."""
    from . import inference
    gw, gh = vis['grid_size']
    z, c = vis['z'].to(device), vis['c'].to(device)
    cp = TensorGroup(**{k: v.to(device) for k, v in vis['camera_params'].items()})
    tiles = []
    with torch.no_grad():
        for b0 in range(0, len(z), opts.test_batch_gpu):
            sl = slice(b0, b0 + opts.test_batch_gpu)
            img = G_ema(z[sl], c[sl], cp[sl], noise_mode='const')
            img = img.img if isinstance(img, TensorGroup) else img
            tiles.append((img[:, :3] * 127.5 + 128).clamp(0, 255).to(torch.uint8))
        inference.save_video(image_grid_u8(torch.cat(tiles).cpu().numpy(), gw, gh), os.path.join(run_dir, f'{name}.png'))
        nv = min(int(opts.num_videos), len(z))
        if nv > 0:
            traj = dict(inference.SNAPSHOT_TRAJECTORY, num_frames=int(opts.video_frames))
            cams = inference.generate_camera_params(G_ema, z[:nv], c[:nv], traj, camera_cfg=camera_cfg_of(opts))
            ws = G_ema.mapping(z[:nv], c[:nv])
            grid = inference.render_video_grid(G_ema, ws, cams.to(device), plane_batch=opts.test_batch_gpu)
            inference.save_video(grid, os.path.join(run_dir, f'{name}_video.gif'))


def snapshot_dir(run_dir, nimg):
    return os.path.join(run_dir, f'network-snapshot-{int(nimg) // 1000:06d}')


def save_network_snapshot(path, opts, G, D, G_ema, pipe, G_opt, D_opt, stats, vis):
    """generator.json / generator.npz (G_ema, the exported format), augment_pipe.json / .npz, training_state.pt."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, 'generator.json'), 'w') as f:
        json.dump(G_ema.cfg.to_dict(), f, indent=1)
    np.savez(os.path.join(path, 'generator.npz'), **{k: v.detach().cpu().numpy() for k, v in G_ema.state_dict().items()})
    if pipe is not None:
        args = ('xflip', 'rotate90', 'xint', 'xint_max', 'scale', 'rotate', 'aniso', 'xfrac', 'scale_std', 'rotate_max', 'aniso_std', 'xfrac_std',
                'brightness', 'contrast', 'lumaflip', 'hue', 'saturation', 'brightness_std', 'contrast_std', 'hue_max', 'saturation_std',
                'imgfilter', 'imgfilter_bands', 'imgfilter_std', 'noise', 'cutout', 'noise_std', 'cutout_size')
        with open(os.path.join(path, 'augment_pipe.json'), 'w') as f:
            json.dump({k: (list(getattr(pipe, k)) if k == 'imgfilter_bands' else float(getattr(pipe, k))) for k in args}, f, indent=1)
        np.savez(os.path.join(path, 'augment_pipe.npz'), **{k: v.detach().cpu().numpy() for k, v in pipe.state_dict().items()})
    cpu = lambda sd: {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}      # noqa: E731
    torch.save(dict(G=cpu(G.state_dict()), D=cpu(D.state_dict()), G_opt=G_opt.state_dict(), D_opt=D_opt.state_dict(), stats=dict(stats), vis=vis,
                    augment_p=None if pipe is None else float(pipe.p), options=opts.to_dict()), os.path.join(path, 'training_state.pt'))
    return path


def _is_regular(tick, snap):
    return snap is not None and snap > 0 and tick % snap == 0


# ----------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------
def training_loop(opts, run_dir, rank=0, world=1, abort_fn=None, progress_fn=None, on_setup=None):
    """Runs until `total_kimg` (or `abort_fn()` at a tick) and returns the final `stats` dict (cur_nimg, cur_tick, batch_idx,
    best_metric_value / _tick / _nimg).  Rank 0 writes `run_dir`.  `on_setup(run)` is called once before the first batch with a namespace
    of the run's objects (G, D, G_ema, pipe, ada, loss, phases, G_opt, D_opt, stats, training_set)."""
    from .distributed import rank_seed
    start_time = time.time()
    device = torch.device('cuda', torch.cuda.current_device()) if str(opts.device) == 'cuda' else torch.device(opts.device)      # (the launcher set the rank's device)
    np.random.seed(rank_seed(opts.seed, rank, world))
    torch.manual_seed(rank_seed(opts.seed, rank, world))
    if opts.batch_size % world != 0 or (opts.batch_gpu or 1) < 1 or (opts.batch_size // world) % (opts.batch_gpu or opts.batch_size // world) != 0:
        raise ValueError('batch_size must be a multiple of world * batch_gpu')
    os.makedirs(run_dir, exist_ok=True)

    cfg = generator_config(opts)                                             # refuses camera_cond before anything is built
    training_set, iterator = build_training_set(opts, rank, world, cfg.c_dim)
    G, D, G_ema, state = build_networks(opts, cfg, training_set, device)
    whole = bool(opts.resume_whole_state and state is not None)
    stats = dict(cur_nimg=0, cur_tick=0, batch_idx=0, best_metric_value=float('inf'), best_metric_tick=0, best_metric_nimg=0)
    if whole:
        stats.update(state['stats'])
    pipe, ada = build_augment(opts, device, state if whole else None)
    for module in (G, D, G_ema, pipe):
        TR.broadcast_module(module)
    loss = build_loss(opts, G, D, pipe, device)
    loss.stats = tick_stats = TickStats()
    phases = TR.setup_phases(G, D, opts.G_opt, opts.D_opt, G_reg_interval=opts.G_reg_interval, D_reg_interval=opts.D_reg_interval)
    G_opt = next(p['opt'] for p in phases if p['name'] in ('Gall', 'Gmain'))
    D_opt = next(p['opt'] for p in phases if p['name'] in ('Dall', 'Dmain'))
    if whole and opts.resume_optim:
        G_opt.load_state_dict(state['G_opt'])
        D_opt.load_state_dict(state['D_opt'])
    metrics = opts.metrics if isinstance(opts.metrics, dict) else {m: None for m in (opts.metrics or [])}
    metrics = {name: (fn if callable(fn) else resolve_metric(name, opts, training_set)) for name, fn in metrics.items()}

    if on_setup is not None:
        import types
        on_setup(types.SimpleNamespace(G=G, D=D, G_ema=G_ema, pipe=pipe, ada=ada, loss=loss, phases=phases, G_opt=G_opt, D_opt=D_opt, stats=dict(stats),
                                       training_set=training_set))
    cur_nimg, cur_tick, batch_idx = int(stats['cur_nimg']), int(stats['cur_tick']), int(stats['batch_idx'])
    G.progressive_update(cur_nimg / 1000)
    loss.progressive_update(cur_nimg / 1000)
    vis = None
    if rank == 0 and opts.image_snap is not None:
        from . import inference
        if whole and state.get('vis') is not None:
            vis, name = state['vis'], f'fakes_resume_{cur_nimg:06d}'
        else:
            vis, reals, depth = setup_snapshot_grid(opts, training_set, G, device)
            gw, gh = vis['grid_size']
            inference.save_video(image_grid_u8(reals, gw, gh), os.path.join(run_dir, 'reals.png'))
            if depth is not None:
                inference.save_video(image_grid_u8((depth // 256).clip(0, 255).astype(np.uint8), gw, gh), os.path.join(run_dir, 'reals_depth.png'))
            name = 'fakes_init'
        save_image_snapshot(opts, run_dir, name, vis, G_ema, device)
    stats_jsonl = open(os.path.join(run_dir, 'stats.jsonl'), 'at' if whole else 'wt') if rank == 0 else None

    tick_start_nimg, tick_start_time = cur_nimg, time.time()
    maintenance_time = tick_start_time - start_time
    if progress_fn is not None:
        progress_fn(0, opts.total_kimg)
    try:
        while True:
            real, gen = fetch(opts, iterator, training_set, G, phases, device)
            run_batch(opts, loss, phases, real, gen, G, G_ema, batch_idx, cur_nimg, world, ada)
            cur_nimg += opts.batch_size
            batch_idx += 1
            G.progressive_update(cur_nimg / 1000)
            loss.progressive_update(cur_nimg / 1000)

            # training_loop.py:384-386
            done = cur_nimg >= opts.total_kimg * 1000
            if not done and cur_tick != 0 and cur_nimg < tick_start_nimg + opts.kimg_per_tick * 1000:
                continue

            tick_end_time = time.time()
            line = {k: v for k, v in tick_stats.collect().items()}
            one = lambda v: dict(num=1, mean=float(v))                  # noqa: E731
            line['Progress/tick'], line['Progress/kimg'] = one(cur_tick), one(cur_nimg / 1e3)
            line['Progress/augment'] = one(float(pipe.p) if pipe is not None else 0.0)
            line['Timing/total_sec'], line['Timing/sec_per_tick'] = one(tick_end_time - start_time), one(tick_end_time - tick_start_time)
            line['Timing/sec_per_kimg'] = one((tick_end_time - tick_start_time) / max(cur_nimg - tick_start_nimg, 1) * 1e3)
            line['Timing/maintenance_sec'] = one(maintenance_time)
            peak = torch.cuda.max_memory_allocated(device) / 2 ** 30 if device.type == 'cuda' else 0.0
            line['Resources/peak_gpu_mem_gb'] = one(peak)
            if device.type == 'cuda':
                torch.cuda.reset_peak_memory_stats(device)
                from . import _lib
                _lib.raise_on_device_fault('training_loop tick')
            if rank == 0:
                d_loss = line.get('Loss/D/loss', {}).get('mean', float('nan'))
                print(f"tick {cur_tick:<5d} kimg {cur_nimg / 1e3:<8.1f} sec/tick {line['Timing/sec_per_tick']['mean']:<7.1f} "
                      f"sec/kimg {line['Timing/sec_per_kimg']['mean']:<7.2f} gpumem {peak:<6.2f} augment {line['Progress/augment']['mean']:.3f} Dloss {d_loss:<4.3f}", flush=True)
            if not done and abort_fn is not None and abort_fn():
                done = True

            if rank == 0 and vis is not None and (done or cur_tick % opts.image_snap == 0):
                save_image_snapshot(opts, run_dir, f'fakes{cur_nimg // 1000:06d}', vis, G_ema, device)

            # metrics (training_loop.py:460-472), then the snapshot (:473-497)
            main_value = None
            if metrics and cur_tick % opts.val_freq == 0:
                for i, (name, fn) in enumerate(metrics.items()):
                    value = float(fn(G_ema))
                    if i == 0:
                        main_value = value
                    line[f'Metrics/{name}'] = one(value)
                    if rank == 0:
                        with open(os.path.join(run_dir, f'metric-{name}.jsonl'), 'at') as f:
                            f.write(json.dumps(dict(results={name: value}, metric=name, snapshot=os.path.basename(snapshot_dir(run_dir, cur_nimg)),
                                                    tick=cur_tick, kimg=cur_nimg / 1e3, timestamp=time.time())) + '\n')
            is_best = main_value is not None and main_value <= stats['best_metric_value']
            now = dict(cur_nimg=cur_nimg, cur_tick=cur_tick, batch_idx=batch_idx)
            if is_best:
                prev = snapshot_dir(run_dir, stats['best_metric_nimg'])
                keep = _is_regular(stats['best_metric_tick'], opts.snap) or prev == snapshot_dir(run_dir, cur_nimg)
                if rank == 0 and not keep and os.path.isdir(prev):
                    shutil.rmtree(prev)                                     # the previous best, unless it is a regular snapshot
                now.update(best_metric_value=main_value, best_metric_tick=cur_tick, best_metric_nimg=cur_nimg)
            stats.update(now)
            if rank == 0 and (done or _is_regular(cur_tick, opts.snap) or is_best):
                save_network_snapshot(snapshot_dir(run_dir, cur_nimg), opts, G, D, G_ema, pipe, G_opt, D_opt, stats, vis)

            if stats_jsonl is not None:
                stats_jsonl.write(json.dumps(dict(line, timestamp=time.time())) + '\n')
                stats_jsonl.flush()
            if progress_fn is not None:
                progress_fn(cur_nimg // 1000, opts.total_kimg)

            cur_tick += 1
            stats['cur_tick'] = cur_tick
            tick_start_nimg, tick_start_time = cur_nimg, time.time()
            maintenance_time = tick_start_time - tick_end_time
            if done:
                break
    finally:
        if stats_jsonl is not None:
            stats_jsonl.close()
        iterator.close()
        training_set.close()
    return stats

"""The training driver end to end on the GPU (3dgp_amd/training_loop.py): six iterations of the tiny generator with a depth adaptor on the
six-image dataset tests/test_dataset.py writes, patch-wise, ADA on, lazy R1, the fused step tail, `nfs256` on 8 samples; then the snapshot
round trip, resume of the whole state, the eager arm and the refusal of camera-conditioned generators."""
import json
import os

import numpy as np
import pytest
import torch

from test_dataset import write_fixture

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _require_native(tdgp):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()


def options(tdgp, data, **fields):
    cfg = tdgp.config.configs_adaptor_goldens()[0][1]                       # 'a': config_tiny + depth adaptor (+ camera adaptor), 16^2 images
    base = dict(data=data, use_depth=True, generator=cfg.to_dict(), discriminator=dict(cbase=256, cmax=16), batch_size=4, batch_gpu=2, D_reg_interval=2,
                patch=dict(resolution=8, min_scale_trg=0.5, mbstd_group_size=2), r1_gamma=2.0,
                augment=dict(mode='ada', p=0.2, target=0.6, interval=2, kimg=0.1, pipe=dict(xflip=1, rotate90=1, xint=1, scale=1, brightness=1)),
                kimg_per_tick=0.008, total_kimg=0.024, snap=2, image_snap=2, val_freq=2, metrics=['nfs256'], metric_kwargs=dict(nfs256=dict(num_gen=8)),
                grid=[3, 2], num_videos=2, video_frames=4, fused_step_tail=True, workers=2)
    return tdgp.training_loop.TrainingOptions(**dict(base, **fields))


@pytest.fixture(scope='module')
def run(tdgp, tmp_path_factory):
    """The one training run the tests below share: -> dict(dir, data, stats, setup namespace, G's initial parameters)."""
    root = tmp_path_factory.mktemp('train')
    data = write_fixture(root)[0]
    out = dict(dir=str(root / 'run'), data=data)

    def on_setup(ns):
        out['ns'] = ns
        out['G0'] = [p.detach().clone() for p in ns.G.parameters()]
    out['stats'] = tdgp.training_loop.training_loop(options(tdgp, data), out['dir'], on_setup=on_setup)
    return out


def test_run_ends_by_itself_and_reports_its_ticks(run):
    assert run['stats']['cur_nimg'] == 24 and run['stats']['batch_idx'] == 6 and run['stats']['cur_tick'] == 4
    with open(os.path.join(run['dir'], 'stats.jsonl')) as f:
        lines = [json.loads(ln) for ln in f]
    assert [int(ln['Progress/kimg']['mean'] * 1000 + 0.5) for ln in lines] == [4, 12, 20, 24]
    for ln in lines:
        assert np.isfinite(ln['Loss/D/loss']['mean']) and np.isfinite(ln['Loss/G/loss']['mean']) and ln['Loss/D/loss']['num'] > 0
        assert ln['Resources/peak_gpu_mem_gb']['mean'] > 0 and ln['Progress/augment']['mean'] >= 0
    assert lines[1]['Loss/D/loss']['num'] == 2 * 4 and 'Loss/D/r1_penalty' in lines[1]            # two batches of four; Dreg ran on an even batch
    assert [('Metrics/nfs256' in ln) for ln in lines] == [True, False, True, False]
    assert 1.0 <= lines[0]['Metrics/nfs256']['mean'] <= 64.0
    ns = run['ns']
    assert any(not torch.equal(a, b) for a, b in zip(run['G0'], ns.G.parameters()))               # G moved
    assert any(not torch.equal(a, b) for a, b in zip(ns.G_ema.parameters(), ns.G.parameters()))   # and G_ema is not G
    assert all(bool(torch.isfinite(p).all()) for p in list(ns.G.parameters()) + list(ns.D.parameters()))
    assert ns.D.img_channels == 4 and ns.D.img_resolution == 8
    assert all(p['step_tail'].record['launches'] == 4 for p in ns.phases)                          # every phase went through the fused tail
    for name in ('reals.png', 'reals_depth.png', 'fakes_init.png', 'fakes_init_video.gif', 'fakes000000.png', 'metric-nfs256.jsonl'):
        assert os.path.exists(os.path.join(run['dir'], name)), name


def test_last_snapshot_is_an_exported_checkpoint(tdgp, run):
    snap = os.path.join(run['dir'], 'network-snapshot-000000')
    assert sorted(os.listdir(snap)) == ['augment_pipe.json', 'augment_pipe.npz', 'generator.json', 'generator.npz', 'training_state.pt']
    cfg, sd = tdgp.weights.load_exported(snap)
    G2 = tdgp.generator.Generator(cfg)
    G2.load_numpy_state_dict(sd)
    G2 = G2.to(DEV).eval()
    kw, psd = tdgp.weights.load_exported_augment_pipe(snap)
    assert kw['xflip'] == 1.0 and float(psd['p']) == float(run['ns'].pipe.p)
    z = torch.randn(2, cfg.z_dim, generator=torch.Generator().manual_seed(5)).to(DEV)
    c = torch.zeros(2, 0, device=DEV)
    torch.manual_seed(3)
    cam = tdgp.metrics.sample_camera_params(tdgp.metrics.camera_base(), 2, DEV)
    imgs = []
    with torch.no_grad():
        for G in (G2, run['ns'].G_ema):
            torch.manual_seed(11)                                           # the renderer's draws
            out = G(z, c, cam, noise_mode='const')
            imgs.append(out.img if isinstance(out, dict) else out)
    assert imgs[0].shape[-1] == 16 and torch.equal(imgs[0], imgs[1])


def test_resume_whole_state_then_one_more_iteration(tdgp, run, tmp_path):
    snap = os.path.join(run['dir'], 'network-snapshot-000000')
    saved = torch.load(os.path.join(snap, 'training_state.pt'), weights_only=False)
    assert saved['stats']['cur_nimg'] == 24 and saved['stats']['batch_idx'] == 6
    seen = {}

    def on_setup(ns):
        seen['stats'], seen['p'] = dict(ns.stats), ns.pipe.p.detach().cpu().clone()
        for name, opt in (('G_opt', ns.G_opt), ('D_opt', ns.D_opt)):
            seen[name] = {i: s['exp_avg_sq'].detach().cpu().clone() for i, s in opt.state_dict()['state'].items()}
    opts = options(tdgp, run['data'], resume=snap, resume_whole_state=True, total_kimg=0.028, metrics=[], image_snap=None)
    stats = tdgp.training_loop.training_loop(opts, str(tmp_path / 'resumed'), on_setup=on_setup)
    assert seen['stats']['cur_nimg'] == 24 and seen['stats']['batch_idx'] == 6 and seen['stats']['cur_tick'] == saved['stats']['cur_tick']
    assert np.float32(saved['augment_p']).tobytes() == seen['p'].numpy().astype(np.float32).tobytes()
    for name in ('G_opt', 'D_opt'):
        assert len(seen[name]) == len(saved[name]['state']) > 0
        for i, s in saved[name]['state'].items():
            assert torch.equal(s['exp_avg_sq'].cpu().view(torch.int32), seen[name][i].view(torch.int32)), (name, i)
    assert stats['cur_nimg'] == 28 and stats['batch_idx'] == 7                                    # one further iteration ran


def test_eager_arm_completes(tdgp, run, tmp_path):
    opts = options(tdgp, run['data'], fused_step_tail=False, metrics=[], image_snap=None)
    seen = {}
    stats = tdgp.training_loop.training_loop(opts, str(tmp_path / 'eager'), on_setup=lambda ns: seen.update(ns=ns))
    assert stats['cur_nimg'] == 24 and all('step_tail' not in p for p in seen['ns'].phases)
    with open(tmp_path / 'eager' / 'stats.jsonl') as f:
        assert all(np.isfinite(json.loads(ln)['Loss/D/loss']['mean']) for ln in f)


def test_camera_cond_is_refused_before_any_step(tdgp, run, tmp_path):
    cfg = tdgp.config.configs_adaptor_goldens()[0][1]
    cfg.camera_cond = True
    with pytest.raises(NotImplementedError, match='camera_cond'):
        tdgp.training_loop.training_loop(options(tdgp, run['data'], generator=cfg.to_dict()), str(tmp_path / 'refused'))
    assert not os.path.exists(tmp_path / 'refused' / 'stats.jsonl')

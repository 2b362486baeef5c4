"""3dgp_amd/training_loop.py on the CPU: tick / snapshot / metric logic with the networks stubbed by tiny modules and the training
iteration by a counter, the options' yaml round trip, and the refusal of camera-conditioned generators."""
import copy
import json
import os

import pytest
import torch


@pytest.fixture(scope='module')
def TL(tdgp):
    return tdgp.training_loop


class _Set:
    resolution, num_channels = 16, 3

    def __len__(self):
        return 6

    def close(self):
        pass


def _batches():
    while True:
        yield None


class _G(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg, self.z_dim, self.c_dim = cfg, cfg.z_dim, cfg.c_dim
        self.fc = torch.nn.Linear(4, 3)
        self.seen_kimg = []

    def progressive_update(self, kimg):
        self.seen_kimg.append(kimg)


class _Loss:
    def __init__(self):
        self.stats = {}

    def progressive_update(self, kimg):
        pass


def stub_run(TL, tdgp, monkeypatch, **fields):
    """TrainingOptions on the CPU with every device-touching part of the driver replaced; -> (opts, log)."""
    log = dict(batches=[], images=[], loss=None)
    cfg = tdgp.config.config_tiny()

    def build_networks(opts, cfg_, training_set, device):
        G = _G(cfg_)
        return G, torch.nn.Linear(3, 1), copy.deepcopy(G), None

    def build_loss(opts, G, D, pipe, device):
        log['loss'] = _Loss()
        return log['loss']

    def run_batch(opts, loss, phases, real, gen, G, G_ema, batch_idx, cur_nimg, world, ada):
        log['batches'].append((batch_idx, cur_nimg))
        loss.stats['Loss/D/loss'] = torch.tensor([1.0, 3.0]) * (batch_idx + 1)          # two values per batch
        loss.stats['Loss/scores/real'] = torch.tensor([0.5])

    monkeypatch.setattr(TL, 'build_training_set', lambda opts, rank, world, c_dim: (_Set(), _batches()))
    monkeypatch.setattr(TL, 'build_networks', build_networks)
    monkeypatch.setattr(TL, 'build_loss', build_loss)
    monkeypatch.setattr(TL, 'fetch', lambda *a, **k: (None, None))
    monkeypatch.setattr(TL, 'run_batch', run_batch)
    monkeypatch.setattr(TL, 'setup_snapshot_grid', lambda opts, ts, G, device: (dict(grid_size=[1, 1]), torch.zeros(1, 3, 16, 16, dtype=torch.uint8).numpy(), None))
    monkeypatch.setattr(TL, 'save_image_snapshot', lambda opts, run_dir, name, vis, G_ema, device: log['images'].append(name))
    opts = TL.TrainingOptions(**dict(dict(generator=cfg.to_dict(), device='cpu', batch_size=8, D_reg_interval=None), **fields))
    return opts, log


def _lines(run_dir):
    with open(os.path.join(run_dir, 'stats.jsonl')) as f:
        return [json.loads(ln) for ln in f]


def _snapshots(run_dir):
    return sorted(d for d in os.listdir(run_dir) if d.startswith('network-snapshot-'))


def test_tick_boundaries_cadence_and_stats(TL, tdgp, monkeypatch, tmp_path):
    calls = []
    opts, log = stub_run(TL, tdgp, monkeypatch, kimg_per_tick=0.016, total_kimg=0.08, snap=2, image_snap=3, val_freq=2,
                         metrics={'fake': lambda G_ema: calls.append(1) or 7.0 + len(calls)})
    saved = []
    real_save = TL.save_network_snapshot
    monkeypatch.setattr(TL, 'save_network_snapshot', lambda path, *a: saved.append(a[-2]['cur_tick']) or real_save(path, *a))
    stats = TL.training_loop(opts, str(tmp_path))
    # training_loop.py:384-386 for batch 8, 16 images per tick: tick 0 ends with the first batch, then every 16 images, then at the end
    lines = _lines(tmp_path)
    assert [int(ln['Progress/kimg']['mean'] * 1000 + 0.5) for ln in lines] == [8, 24, 40, 56, 72, 80]
    assert [ln['Progress/tick']['mean'] for ln in lines] == [0, 1, 2, 3, 4, 5]
    assert log['batches'] == [(i, 8 * i) for i in range(10)]
    assert stats['cur_nimg'] == 80 and stats['batch_idx'] == 10 and stats['cur_tick'] == 6
    for ln in lines:
        for key in ('Loss/D/loss', 'Loss/scores/real', 'Progress/tick', 'Progress/kimg', 'Progress/augment', 'Timing/sec_per_tick', 'Timing/sec_per_kimg',
                    'Resources/peak_gpu_mem_gb'):
            assert set(ln[key]) == {'num', 'mean'}, key
        assert 'timestamp' in ln
    # mean and count over the tick: tick 1 holds batches 1 and 2 -> values (2, 6, 3, 9)
    assert lines[0]['Loss/D/loss'] == dict(num=2, mean=2.0) and lines[1]['Loss/D/loss'] == dict(num=4, mean=5.0) and lines[1]['Loss/scores/real']['num'] == 2
    assert lines[5]['Loss/D/loss']['num'] == 2
    # cadence: network snapshots at ticks 0, 2, 4 and at the end; images at the start, ticks 0, 3 and the end; metrics at ticks 0, 2, 4
    assert saved == [0, 2, 4, 5]
    assert log['images'] == ['fakes_init', 'fakes000000', 'fakes000000', 'fakes000000']
    assert len(calls) == 3 and ['Metrics/fake' in ln for ln in lines] == [True, False, True, False, True, False]
    with open(tmp_path / 'metric-fake.jsonl') as f:
        rows = [json.loads(ln) for ln in f]
    assert [r['tick'] for r in rows] == [0, 2, 4] and rows[0]['results'] == {'fake': 8.0}
    assert os.path.exists(tmp_path / 'reals.png')
    state = torch.load(tmp_path / 'network-snapshot-000000' / 'training_state.pt', weights_only=False)
    assert sorted(state) == ['D', 'D_opt', 'G', 'G_opt', 'augment_p', 'options', 'stats', 'vis'] and state['stats']['cur_nimg'] == 80
    assert state['options']['kimg_per_tick'] == 0.016 and state['options']['metrics'] == ['fake']


def test_best_snapshot_bookkeeping(TL, tdgp, monkeypatch, tmp_path):
    """Ticks end at 500, 1500, ..., 5500 and 6000 images; the scripted metric makes ticks 0, 1, 3 and 5 a new best.  Tick 0 and 4 are regular
    snapshots (snap 4): the best of tick 0 survives, those of ticks 1 and 3 are deleted when a better one comes."""
    values = iter([5.0, 4.0, 4.5, 3.0, 9.0, 2.0, 8.0])
    seen = []
    opts, log = stub_run(TL, tdgp, monkeypatch, batch_size=500, kimg_per_tick=1, total_kimg=6, snap=4, image_snap=None, val_freq=1,
                         metrics={'m': lambda G_ema: next(values)})
    real_save = TL.save_network_snapshot
    monkeypatch.setattr(TL, 'save_network_snapshot', lambda path, *a: real_save(path, *a) and seen.append(_snapshots(str(tmp_path))))
    stats = TL.training_loop(opts, str(tmp_path))
    n = 'network-snapshot-00000'
    assert seen == [[n + '0'], [n + '0', n + '1'], [n + '0', n + '3'], [n + '0', n + '3', n + '4'], [n + '0', n + '4', n + '5'], [n + '0', n + '4', n + '5', n + '6']]
    assert stats['best_metric_value'] == 2.0 and stats['best_metric_tick'] == 5 and stats['best_metric_nimg'] == 5500
    assert log['images'] == [] and not os.path.exists(tmp_path / 'reals.png')
    assert len(_lines(tmp_path)) == 7
    cfg, sd = tdgp.weights.config_from_json(json.load(open(tmp_path / (n + '5') / 'generator.json'))), None
    assert cfg.img_resolution == 16


def test_abort_fn_stops_at_a_tick(TL, tdgp, monkeypatch, tmp_path):
    asked = []
    opts, log = stub_run(TL, tdgp, monkeypatch, kimg_per_tick=0.016, total_kimg=1.0, snap=100, image_snap=None)
    stats = TL.training_loop(opts, str(tmp_path), abort_fn=lambda: asked.append(1) or len(asked) == 3)
    assert len(asked) == 3 and stats['cur_nimg'] == 40 and stats['cur_tick'] == 3 and len(_lines(tmp_path)) == 3
    assert _snapshots(str(tmp_path)) == ['network-snapshot-000000']                     # the end of a run is always saved


def test_options_yaml_round_trip_and_unknown_keys(TL, tdgp):
    opts = TL.TrainingOptions(data='x.zip', generator=tdgp.config.configs_adaptor_goldens()[0][1].to_dict(), patch=dict(resolution=8, mbstd_group_size=2),
                              augment=dict(mode='ada', target=0.6, interval=2, pipe=dict(xflip=1, rotate90=1)), metrics=['nfs256'],
                              metric_kwargs=dict(nfs256=dict(num_gen=8)), total_kimg=0.024, G_reg_interval=None)
    text = opts.to_yaml()
    back = TL.TrainingOptions.from_yaml(text)
    # (yaml has no tuples: the camera ranges of the generator node come back as lists, everything else as it went in)
    assert back.to_yaml() == text and TL.TrainingOptions.from_yaml(back.to_yaml()) == back
    assert {k: v for k, v in back.to_dict().items() if k != 'generator'} == {k: v for k, v in opts.to_dict().items() if k != 'generator'}
    assert tdgp.weights.config_from_json(back.generator) == tdgp.weights.config_from_json(opts.generator)
    assert tdgp.weights.config_from_json(back.generator).depth_adaptor.hid_dim == 16
    with pytest.raises(KeyError, match='no_such_option'):
        TL.TrainingOptions.from_yaml(text + 'no_such_option: 1\n')
    d = TL.apply_overrides(opts.to_dict(), ['total_kimg=3', 'augment.mode=fixed', 'patch.resolution=16', 'G_opt.betas=[0.5, 0.9]'])
    o2 = TL.TrainingOptions.from_dict(d)
    assert o2.total_kimg == 3 and o2.augment['mode'] == 'fixed' and o2.augment['interval'] == 2 and o2.patch['resolution'] == 16 and o2.G_opt['betas'] == [0.5, 0.9]
    with pytest.raises(KeyError):
        TL.apply_overrides(opts.to_dict(), ['nonsense.x=1'])
    assert TL.TrainingOptions().fused_step_tail in (True, False)


def test_camera_cond_is_refused_before_anything_is_built(TL, tdgp, tmp_path):
    cfg = tdgp.config.config_tiny()
    cfg.camera_cond = True
    opts = TL.TrainingOptions(data=str(tmp_path / 'does-not-exist'), generator=cfg.to_dict(), device='cpu')
    with pytest.raises(NotImplementedError, match='camera_cond'):
        TL.training_loop(opts, str(tmp_path / 'run'))
    assert not os.path.exists(tmp_path / 'run' / 'stats.jsonl')


def test_train_tool_reads_yaml_and_overrides(TL, tdgp, monkeypatch, tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_tool', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'train.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    opts, log = stub_run(TL, tdgp, monkeypatch, kimg_per_tick=0.016, total_kimg=1.0, snap=100, image_snap=None)
    cfg_path = tmp_path / 'run.yaml'
    cfg_path.write_text(opts.to_yaml())
    stats = tool.main(['--config', str(cfg_path), '--outdir', str(tmp_path / 'out'), 'total_kimg=0.024'])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert stats['cur_nimg'] == 24 and line['cur_nimg'] == 24 and line['run_dir'] == str(tmp_path / 'out') and line['best_metric_value'] is None
    assert TL.TrainingOptions.from_yaml((tmp_path / 'out' / 'options.yaml').read_text()).total_kimg == 0.024
    with pytest.raises(KeyError):
        tool.main(['--config', str(cfg_path), 'bogus=1'])

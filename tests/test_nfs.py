"""Non-flatness score (src/metrics/non_flatness_score.py): histograms, entropy, score, the device route and the rank gather.

Golden `nfs.npz` (tools/gen_goldens.py:gen_nfs): 16 depth maps the reference rendered with cut_quantile = 0.5 plus 8 planted rows that sit
on and one ulp either side of every edge of the 64-bin grid, with the reference's own histograms, entropies and scores for 64 and 16 bins.
"""
import dataclasses
import importlib
import importlib.util
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
HOST_TOL = 1e-6           # same torch ops on the host; exactness is tied to the torch build (the bound of the other host-arithmetic goldens)


def _rel(a, b):
    """Largest elementwise relative error; an entry that is 0 in the golden (the entropy of a flat map) must be 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    return float(np.where(d == 0, 0.0, d / np.maximum(np.abs(b), 1e-300)).max())


# ------------------------------------------------------------------------------------------------ host
@pytest.mark.parametrize('bins', [64, 16])
def test_host_route_matches_the_reference(tdgp, bins):
    M = tdgp.metrics
    g = load_golden('nfs')
    lo, hi = (float(v) for v in g['range'])
    d = torch.from_numpy(g['depth_maps']).clamp(lo, hi)
    h = M.convert_depth_maps_to_histograms(d, bins, lo, hi)
    assert h.dtype == torch.float32
    np.testing.assert_array_equal(h.numpy().astype(np.int64), g[f'hist_{bins}'])
    e = M.compute_histogram_entropy(h)
    assert _rel(e.numpy(), g[f'entropy_{bins}']) <= HOST_TOL
    assert _rel(float(e.exp().mean()), g[f'score_{bins}']) <= HOST_TOL


def test_nan_row_raises_the_reference_message(tdgp):
    g = load_golden('nfs')
    lo, hi = (float(v) for v in g['range'])
    d = torch.from_numpy(g['depth_maps']).clamp(lo, hi)
    d[3, 17] = float('nan')
    with pytest.raises(AssertionError, match='Histograms countain OOB values'):
        tdgp.metrics.convert_depth_maps_to_histograms(d, 64, lo, hi)


def test_quantile_ranks_restate_torch_quantile(tdgp):
    """The host half of tdgp_quantile_select: lerp(sorted[k_lo], sorted[k_hi], weight) is torch.quantile bit for bit (<= 2^24 elements), and
    `_quantile`'s own sort + lerp above."""
    R = tdgp.renderer
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 3, 7, 256, 1025, 65537, 1048579):
        x = torch.nn.functional.softplus(torch.randn(n, generator=g) * 4 - 3)
        xs = torch.sort(x).values
        for q in (0.5, 0.3, 0.4, 0.9, 0.123, 1.0):
            k_lo, k_hi, w = R.quantile_ranks(q, n)
            assert 0 <= k_lo <= k_hi <= min(k_lo + 1, n - 1)
            got = torch.lerp(xs[k_lo], xs[k_hi], torch.tensor(w))
            assert got.view(torch.int32) == R._quantile(x, q).view(torch.int32), (n, q)
    n = (1 << 24) + 5
    for q in (0.5, 0.3, 0.123, 1.0):
        pos = q * (n - 1)
        assert R.quantile_ranks(q, n) == (int(pos), min(int(pos) + 1, n - 1), float(np.float32(pos - int(pos))))
    assert R.quantile_ranks(0.5, 1) == (0, 0, 0.0)


# ------------------------------------------------------------------------------------------------ two gloo ranks
class _StandInG:
    """A CPU generator that returns fixed depth maps, row by row: enough to drive the loop, the histograms and the gather."""
    z_dim, c_dim, device = 4, 0, 'cpu'

    class synthesis:
        camera_adaptor = None

    def __init__(self, rows, side):
        self.rows, self.side, self.at = rows, side, 0

    def __call__(self, z, c, camera_params, render_opts=None):
        assert render_opts['return_depth'] and render_opts['cut_quantile'] == 0.5
        n = z.shape[0]
        d = self.rows[self.at:self.at + n].reshape(n, 1, self.side, self.side)
        self.at += n

        class Out:
            depth = d
        return Out


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _nfs_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    tdgp = importlib.import_module('3dgp_amd')
    M = tdgp.metrics
    g = load_golden('nfs')
    lo, hi = (float(v) for v in g['range'])
    rows = torch.from_numpy(g['depth_maps']).clamp(lo, hi)                # 24 rows of 16^2
    mine = rows[rank::world]                                              # rank r generates rows r, r + world, ...: interleaved = the golden's order
    # one batch of 12 per rank in chunks of 4: the gathered [24, 64] block must come back rank-interleaved, as FID features do
    captured = []
    real_append = M.FeatureStats.append

    def spy(self, x):
        captured.append(np.array(x))
        return real_append(self, x)
    M.FeatureStats.append = spy
    score = M.compute_flatness_score(_StandInG(mine, 16), num_gen=24, min_depth=lo, max_depth=hi, num_bins=64, batch_size=12, batch_gen=4,
                                     num_gpus=world, rank=rank)
    ok = len(captured) == 1 and captured[0].shape == (24, 64) and bool((captured[0].astype(np.int64) == g['hist_64']).all())
    ok = ok and abs(score - float(g['score_64'])) <= HOST_TOL * float(g['score_64'])
    # max_items cuts the interleaved block, not the local one
    score20 = M.compute_flatness_score(_StandInG(mine, 16), num_gen=20, min_depth=lo, max_depth=hi, num_bins=64, batch_size=12, batch_gen=4,
                                       num_gpus=world, rank=rank)
    want20 = float(M.compute_histogram_entropy(torch.from_numpy(g['hist_64'][:20]).float()).exp().mean())
    ok = ok and score20 == want20
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_histogram_block_gather_world2():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_nfs_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res == [(0, True), (1, True)]


# ------------------------------------------------------------------------------------------------ device
def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _histc_rows(d, bins, lo, hi):
    return torch.stack([torch.histc(r, bins, min=lo, max=hi) for r in d]).numpy().astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize('bins', [64, 16])
def test_depth_histc_golden_rows(tdgp, bins):
    tdgp._lib.load()
    g = load_golden('nfs')
    lo, hi = (float(v) for v in g['range'])
    h = tdgp.metrics.convert_depth_maps_to_histograms(T(g['depth_maps']), bins, lo, hi)         # unclamped rows: the kernel clamps
    assert h.is_cuda and h.dtype == torch.float32
    np.testing.assert_array_equal(h.cpu().numpy().astype(np.int64), g[f'hist_{bins}'])


@pytest.mark.gpu
@pytest.mark.parametrize('pixels', [1, 63, 64, 65, 1024, 65536])
def test_depth_histc_row_lengths(tdgp, pixels):
    """Cropped / tiled golden rows against torch.histc on the CPU copy; one block's run is 4096 pixels, so 65 536 is 16 blocks per image.
    Over the golden's own range [0.75, 1.25] the bin arithmetic is exact whatever its order (the width is a power of two), so every bin
    count is also taken over [0.7, 1.3], where it is not."""
    g = load_golden('nfs')
    lo, hi = (float(v) for v in g['range'])
    rows = np.tile(g['depth_maps'], (1, -(-pixels // g['depth_maps'].shape[1])))[:, :pixels].copy()
    if pixels >= 64:
        rows[0, :3] = [lo - 0.5, hi + 0.5, np.float32(hi)]                # outside the range: the end bins after the clamp
        rows[1] = rows[1, 0]                                              # a flat map: every pixel in one bin
    d = torch.from_numpy(rows)
    for a, b in ((lo, hi), (0.7, 1.3)):
        for bins in (64, 16, 1000):
            h = tdgp.metrics._depth_histc(T(rows), bins, a, b)
            assert h.dtype == torch.int32
            np.testing.assert_array_equal(h.cpu().numpy().astype(np.int64), _histc_rows(d.clamp(a, b), bins, a, b))
    if pixels >= 64:
        h = tdgp.metrics._depth_histc(T(rows), 64, lo, hi).cpu().numpy()
        below, above = (rows[0] <= lo).sum(), (rows[0] >= np.float32(hi)).sum()
        assert h[0, 0] >= below >= 1 and h[0, 63] >= above >= 2
        rows[2, 5] = np.nan
        h = tdgp.metrics._depth_histc(T(rows), 64, lo, hi).cpu().numpy()
        assert h[2].sum() == pixels - 1 and (h.sum(1)[[0, 1, 3]] == pixels).all()               # a NaN depth is in no bin
        with pytest.raises(AssertionError, match='Histograms countain OOB values'):
            tdgp.metrics.convert_depth_maps_to_histograms(T(rows), 64, lo, hi)


def _edge_rows(lo, hi, bins, rows=4, pixels=8192, seed=0):
    """[rows, pixels] fp32: every edge lo + k (hi - lo) / bins of the grid with its two fp32 neighbours (3 (bins + 1) values, cycled through
    the rows), the rest uniform over a range 5 % wider than [lo, hi] on either side."""
    e = (lo + np.arange(bins + 1, dtype=np.float64) * (hi - lo) / bins).astype(np.float32)
    planted = np.concatenate([np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))])
    assert planted.size <= rows * pixels // 2
    pad = 0.05 * (hi - lo)
    out = np.random.default_rng(seed).uniform(lo - pad, hi + pad, rows * pixels).astype(np.float32)
    out[:planted.size] = planted
    return out.reshape(pixels, rows).T.copy()                             # the planted values spread over every row


@pytest.mark.gpu
@pytest.mark.parametrize('lo,hi,bins', [(0.1, 0.7, 100), (0.1, 0.7, 1000), (0.88, 1.12, 50), (2.25, 3.3, 1000), (-1.3, 0.9, 7), (0.1, 0.7, 1023),
                                        (0.1, 0.7, 1024), (0.75, 1.25, 1000)])
def test_depth_histc_general_ranges_and_bins(tdgp, lo, hi, bins):
    """Ranges and bin counts of which neither is a power of two, the values that decide it planted: on every bin edge and one ulp either
    side.  CPU torch.histc computes (x - lo) * bins / (hi - lo) in fp32, the product rounded before the division; dividing first agrees only
    where `bins` or `hi - lo` is a power of two (the last two cases) and is 4 ... 400 counts away on the others.  Equality is exact: both
    sides are the same three fp32 operations on the same floats."""
    rows = _edge_rows(lo, hi, bins)
    h = tdgp.metrics._depth_histc(T(rows), bins, lo, hi).cpu().numpy().astype(np.int64)
    want = _histc_rows(torch.from_numpy(rows).clamp(lo, hi), bins, lo, hi)
    assert (want.sum(1) == rows.shape[1]).all()
    print(f'[{lo}, {hi}] {bins} bins: L1 = {int(np.abs(h - want).sum())}')
    np.testing.assert_array_equal(h, want)
    got = tdgp.metrics.convert_depth_maps_to_histograms(T(rows), bins, lo, hi)                  # the public route: same counts, as fp32
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), want)


@pytest.mark.gpu
def test_depth_histc_refuses_bad_arguments(tdgp):
    d = torch.zeros(2, 64, device=DEV)
    for bins in (1, 1025):
        with pytest.raises(RuntimeError, match='bins'):
            tdgp.metrics._depth_histc(d, bins, 0.0, 1.0)
    with pytest.raises(RuntimeError, match='range'):
        tdgp.metrics._depth_histc(d, 64, 1.0, 1.0)


def _tiny_generator(tdgp):
    cfg = tdgp.config.config_tiny()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=21, exercise_all=True))
    return cfg, G.to(DEV).eval()


@pytest.mark.gpu
def test_flatness_score_equals_the_host_loop(tdgp):
    """compute_flatness_score against the same loop written out: compute_flattened_depth_maps (every depth map to the host) + clamp + CPU
    torch.histc + the entropy formula, the draws fixed by seed: same histograms, same score bits."""
    M = tdgp.metrics
    cfg, G = _tiny_generator(tdgp)
    lo, hi = cfg.ray_start, cfg.ray_end
    kw = dict(batch_size=8, batch_gen=4)

    def seed():
        torch.manual_seed(5)
        np.random.seed(5)
    seed()
    depth = M.compute_flattened_depth_maps(G, 20, device=DEV, cut_quantile=0.5, **kw).clamp(lo, hi)
    assert depth.shape == (20, cfg.img_resolution ** 2)
    for bins in (64, 16):
        want_h = torch.stack([torch.histc(r, bins, min=lo, max=hi) for r in depth])
        want = float((-1.0 * (torch.log(want_h / want_h.sum(1, keepdim=True) + 1e-12) * (want_h / want_h.sum(1, keepdim=True))).sum(1)).exp().mean().item())
        captured = []
        real_append = M.FeatureStats.append
        try:
            M.FeatureStats.append = lambda self, x: captured.append(np.array(x)) or real_append(self, x)
            seed()
            got = M.compute_flatness_score(G, 20, lo, hi, num_bins=bins, cut_quantile=0.5, **kw)
        finally:
            M.FeatureStats.append = real_append
        assert all(c.shape == (8, bins) for c in captured)                # only [batch, bins] blocks cross to the host
        np.testing.assert_array_equal(np.concatenate(captured)[:20], want_h.numpy())
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (got, want)
    seed()
    assert M.nfs256(G, batch_size=64, batch_gen=16)['nfs256'] > 1.0


@pytest.mark.gpu
def test_histogram_of_the_e2e_depth_against_the_reference_depth(tdgp):
    """The histogram of this package's cut_quantile depth for the e2e_tiny golden inputs vs the histogram of the reference's `depth_cut`:
    the depths agree to 1e-5 of the range (test_e2e_tiny_cut_quantile), so only the m golden pixels within that distance of a bin edge may
    change bins, each moving one count out of one bin and into another: L1 <= 2 m.  m is counted here and must stay under 5 % of the pixels,
    so that the bound cannot swallow a broken kernel (measured when the golden was made: 1 of 512 for 64 bins, 0 for 16)."""
    cfg, G = _tiny_generator(tdgp)
    g = load_golden('e2e_tiny')
    lo, hi = cfg.ray_start, cfg.ray_end
    cam = {k[4:]: T(v) for k, v in g.items() if k.startswith('cam_')}
    out = G.synthesis(T(g['ws']), camera_params=cam, noise_mode='const', render_opts=dict(return_depth=True, cut_quantile=0.5),
                      u_coarse=T(g['u_coarse']), u_fine=T(g['u_fine']))
    ref = g['depth_cut'].reshape(g['depth_cut'].shape[0], -1)
    tol = 1e-5 * np.abs(ref).max()
    for bins in (64, 16):
        edges = lo + np.arange(1, bins, dtype=np.float64) * (hi - lo) / bins       # interior edges: at lo / hi both sides fall in the end bin (clamp)
        m = int((np.abs(ref.astype(np.float64)[..., None] - edges).min(-1) <= tol).sum())
        assert m <= 0.05 * ref.size, (m, ref.size)
        h = tdgp.metrics._depth_histc(out.depth.flatten(start_dim=1), bins, lo, hi).cpu().numpy().astype(np.int64)
        want = _histc_rows(torch.from_numpy(ref).clamp(lo, hi), bins, lo, hi)
        l1 = int(np.abs(h - want).sum())
        print(f'bins {bins}: m = {m}, L1 = {l1}')
        assert l1 <= 2 * m, (bins, l1, m)


# ------------------------------------------------------------------------------------------------ tools/calc_nfs.py
def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_calc_nfs_command_line_and_labels():
    cli = _tool('calc_nfs')
    a = cli.build_parser().parse_args(['--ckpt', 'some_dir'])
    assert (a.ckpt, a.num_gen, a.batch_gen, a.seed) == ('some_dir', 256, 4, 0)
    a = cli.build_parser().parse_args(['--ckpt', 'd', '--num-gen', '32', '--batch-gen', '16', '--seed', '7'])
    assert (a.num_gen, a.batch_gen, a.seed) == (32, 16, 7)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args([])                                 # --ckpt is required
    ds = cli.UniformLabels(5)
    assert len(ds) == 5
    for i in range(5):
        label = ds.get_label(i)
        assert label.dtype == np.float32 and label.shape == (5,) and label[i] == 1.0 and label.sum() == 1.0
    assert ds.get_camera_angles(3).shape == (3,)


@pytest.mark.gpu
@pytest.mark.parametrize('c_dim', [0, 3])
def test_calc_nfs_on_an_exported_checkpoint_directory(tdgp, tmp_path, capsys, c_dim):
    """tools/calc_nfs.py on a directory laid out as tools/export_reference_checkpoint.py writes it (generator.json + generator.npz), run in
    this process: one JSON line, and the score of the same loop called directly with the same seed, bit for bit.  c_dim 3 draws classes
    through the tool's uniform-label stand-in."""
    cli = _tool('calc_nfs')
    cfg = dataclasses.replace(tdgp.config.config_tiny(), c_dim=c_dim)
    sd = tdgp.weights.random_state_dict(cfg, seed=21, exercise_all=True)
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **sd)
    cli.main(['--ckpt', str(tmp_path), '--num-gen', '8', '--batch-gen', '4', '--seed', '3'])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res['num_gen'] == 8 and res['batch_gen'] == 4 and res['seed'] == 3 and res['ckpt'] == str(tmp_path)
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(sd)
    G = G.to(DEV).eval()
    torch.manual_seed(3)
    np.random.seed(3)
    with torch.no_grad():
        want = tdgp.metrics.compute_flatness_score(G, 8, cfg.ray_start, cfg.ray_end, batch_gen=4, dataset=cli.UniformLabels(c_dim) if c_dim else None)
    assert 1.0 <= want <= 64.0
    assert np.float64(res['nfs8']).tobytes() == np.float64(want).tobytes(), (res, want)

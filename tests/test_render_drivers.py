"""The pieces the render drivers share (3dgp_amd/renderer.py): `Draws`, the carrier of a call's explicit random draws, and `Gather`, which
reassembles the results of a call made in pieces -- on plain CPU tensors -- and a forward split while explicit density-noise draws are in
play, on the GPU.  A wrong reshape of a draw does not crash: it hands a ray another ray's numbers, so every element here names its ray."""
import importlib
import itertools

import numpy as np
import pytest
import torch

B, R, S, N = 3, 8, 4, 3
gpu = pytest.mark.gpu


def _sources():
    """One arange per draw, in the canonical [B,R,k] shape: element value = (b * R + r) * k + j."""
    ar = lambda k, off: torch.arange(B * R * k, dtype=torch.float32).reshape(B, R, k) + off          # noqa: E731
    return dict(u_coarse=ar(S, 0.0), u_fine=ar(N, 1000.0), n_coarse=ar(S, 2000.0), n_fine=ar(N, 3000.0))


# every layout the callers pass (renderer.Draws)
LAYOUTS = dict(u_coarse=[lambda t: t, lambda t: t.reshape(B, R, S, 1)], u_fine=[lambda t: t.reshape(B * R, N), lambda t: t],
               n_coarse=[lambda t: t.reshape(B, R * S, 1), lambda t: t.reshape(B, R * S)], n_fine=[lambda t: t.reshape(B, R * N, 1), lambda t: t.reshape(B, R * N)])


@pytest.mark.parametrize('pick', list(itertools.product((0, 1), repeat=4)), ids=lambda p: ''.join(map(str, p)))
def test_draws_layouts(tdgp, pick):
    src = _sources()
    given = {k: LAYOUTS[k][i](src[k]) for (k, i) in zip(src, pick)}
    o = tdgp.renderer.Draws(B, R, **given).take(slice(1, 3), slice(2, 6)).opts()
    assert list(o) == ['u_coarse', 'u_fine', 'n_coarse', 'n_fine'] and all(t.is_contiguous() for t in o.values())
    assert o['u_coarse'].shape == (2, 4, S) and torch.equal(o['u_coarse'], src['u_coarse'][1:3, 2:6])
    assert o['u_fine'].shape == (8, N)
    for i in range(8):                                                # row i = sample 1 + i // 4, ray 2 + i % 4
        assert torch.equal(o['u_fine'][i], src['u_fine'][1 + i // 4, 2 + i % 4]), i
    assert o['n_coarse'].shape == (2, 4 * S, 1) and torch.equal(o['n_coarse'].reshape(2, 4, S), src['n_coarse'][1:3, 2:6])
    assert o['n_fine'].shape == (2, 4 * N, 1) and torch.equal(o['n_fine'].reshape(2, 4, N), src['n_fine'][1:3, 2:6])


def test_draws_whole_range_is_the_same_storage(tdgp):
    src = _sources()
    given = dict(u_coarse=src['u_coarse'], u_fine=src['u_fine'].reshape(B * R, N), n_coarse=None, n_fine=src['n_fine'].reshape(B, R * N, 1))
    d = tdgp.renderer.Draws(B, R, **given)
    for part in (d, d.take(slice(0, B)), d.take(slice(0, B), slice(0, R)), d.take(slice(0, B)).take(slice(None), slice(0, R))):
        o = part.opts()
        assert part.t['n_coarse'] is None and o['n_coarse'] is None
        for k in ('u_coarse', 'u_fine', 'n_fine'):
            assert part.t[k].data_ptr() == given[k].data_ptr() and o[k].data_ptr() == given[k].data_ptr(), k
            assert o[k].shape == given[k].shape, k
    empty = tdgp.renderer.Draws(B, R).take(slice(1, 2), slice(0, 3)).opts()
    assert empty == dict(u_coarse=None, u_fine=None, n_coarse=None, n_fine=None)


@pytest.mark.parametrize('seed', [0, 7])
def test_draws_filled_draws_what_the_autograd_node_drew(tdgp, seed):
    """`filled` against the calls `_RenderFunction.forward` made inline: same seed, same order, same shapes -> the same numbers."""
    D = tdgp.renderer.Draws
    torch.manual_seed(seed)
    want = dict(u_coarse=torch.rand([B, R, S, 1], device='cpu'), u_fine=torch.rand([B * R, N], device='cpu'),
                n_coarse=torch.randn([B, R * S, 1], device='cpu'), n_fine=torch.randn([B, R * N, 1], device='cpu'))
    torch.manual_seed(seed)
    o = D(B, R).filled(S, N, 0.4, 'cpu').opts()
    assert o['u_coarse'].shape == (B, R, S) and o['u_fine'].shape == (B * R, N) and o['n_coarse'].shape == (B, R * S, 1) and o['n_fine'].shape == (B, R * N, 1)
    for k in want:
        assert torch.equal(o[k].reshape(-1), want[k].reshape(-1)), k
    # no density noise: only the uniform draws, the same two
    torch.manual_seed(seed)
    o = D(B, R).filled(S, N, 0.0, 'cpu').opts()
    assert o['n_coarse'] is None and o['n_fine'] is None
    assert torch.equal(o['u_coarse'].reshape(-1), want['u_coarse'].reshape(-1)) and torch.equal(o['u_fine'], want['u_fine'])
    # no fine pass: u_coarse, then n_coarse directly after it
    torch.manual_seed(seed)
    uc, nc = torch.rand([B, R, S, 1]), torch.randn([B, R * S, 1])
    torch.manual_seed(seed)
    o = D(B, R).filled(S, 0, 0.4, 'cpu').opts()
    assert o['u_fine'] is None and o['n_fine'] is None and torch.equal(o['u_coarse'].reshape(-1), uc.reshape(-1)) and torch.equal(o['n_coarse'], nc)
    # what the caller supplied is kept as given, and takes no number from the stream
    src = _sources()
    torch.manual_seed(seed)
    uf, nf = torch.rand([B * R, N]), torch.randn([B, R * N, 1])
    torch.manual_seed(seed)
    o = D(B, R, u_coarse=src['u_coarse'], n_coarse=src['n_coarse']).filled(S, N, 0.4, 'cpu').opts()
    assert o['u_coarse'].data_ptr() == src['u_coarse'].data_ptr() and o['n_coarse'].data_ptr() == src['n_coarse'].data_ptr()
    assert torch.equal(o['u_fine'], uf) and torch.equal(o['n_fine'], nf)


def test_gather(tdgp):
    rgb = torch.arange(B * R * 3, dtype=torch.float32).reshape(B, R, 3)
    status = torch.arange(B * R, dtype=torch.int32).reshape(B, R)
    g = tdgp.renderer.Gather(B, R)
    for bs in (slice(0, 2), slice(2, 3)):                              # 2 x 3 pieces, the last of each axis smaller
        for rs in (slice(0, 3), slice(3, 6), slice(6, 8)):
            g.put(bs, rs, rgb=rgb[bs, rs].clone(), status=status[bs, rs].clone())
    got_rgb, got_status = g.result()
    assert got_rgb.dtype == torch.float32 and got_status.dtype == torch.int32
    assert torch.equal(got_rgb, rgb) and torch.equal(got_status, status)
    g = tdgp.renderer.Gather(B, R)
    g.put(slice(0, B), slice(0, R), rgb=rgb, status=status)
    got_rgb, got_status = g.result()
    assert got_rgb.data_ptr() == rgb.data_ptr() and got_status.data_ptr() == status.data_ptr()


def test_views_per_sample(tdgp):
    v = tdgp.renderer.views_per_sample
    assert v(12, 3, 'x') == 4 and v(3, 3, 'x') == 1
    for cams, samples in ((7, 3), (2, 3), (4, 0)):
        with pytest.raises(ValueError, match=f'{cams} cameras are not a multiple of the {samples} samples'):
            v(cams, samples, f'{samples} samples')


@gpu
def test_forward_split_with_explicit_density_noise():
    """A training-mode forward with explicit density-noise draws, split by images (2 + 1) and by runs of 4 whole rows: every ray keeps its own
    u_* and n_* draws, so image and depth equal the unsplit call's, bit for bit."""
    tdgp = importlib.import_module('3dgp_amd')
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    tdgp._lib.load()
    dev = 'cuda:0'
    cfg = tdgp.config.config_tiny()                                    # 16 x 16 rays, 8 + 8 samples
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=5, exercise_all=True))
    G = G.to(dev)
    syn = G.synthesis.train()
    syn.nerf_noise_std = 0.4
    nb, rays, steps = 3, 256, 8
    inp = tdgp.weights.synthetic_inputs(cfg, batch=nb, seed=6)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)          # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(6)
    kw = dict(camera_params={k: T(v) for k, v in inp['camera'].items()}, noise_mode='const', render_opts=dict(return_depth=True),
              u_coarse=torch.rand([nb, rays, steps], device=dev, generator=gen), u_fine=torch.rand([nb * rays, steps], device=dev, generator=gen),
              n_coarse=torch.randn([nb, rays * steps, 1], device=dev, generator=gen), n_fine=torch.randn([nb, rays * steps, 1], device=dev, generator=gen))
    ws = G.mapping(T(inp['z']), T(inp['c']))
    whole = syn(ws, **kw)
    assert whole.img.shape == (nb, 3, 16, 16) and whole.depth.shape == (nb, 1, 16, 16)
    bound = tdgp.generator.FIELD_POINTS_MAX
    try:
        tdgp.generator.FIELD_POINTS_MAX = 2 * rays * steps             # two images per call: 2 + 1
        by_images = syn(ws, **kw)
        tdgp.generator.FIELD_POINTS_MAX = 6 * 16 * steps               # six rows per call -> runs of 4 whole rows
        by_rows = syn(ws, **kw)
    finally:
        tdgp.generator.FIELD_POINTS_MAX = bound
    for name, split in (('images', by_images), ('rows', by_rows)):
        assert torch.equal(split.img, whole.img), name
        assert torch.equal(split.depth, whole.depth), name
    no_noise = syn(ws, **dict(kw, n_coarse=torch.zeros_like(kw['n_coarse']), n_fine=torch.zeros_like(kw['n_fine'])))
    assert not torch.equal(no_noise.img, whole.img)                    # the draws do reach the image

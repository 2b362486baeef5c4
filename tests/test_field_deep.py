"""The deep field kernels (3- and 4-layer tri-plane decoders), the parts that need no GPU: which decoders take the deep route, the three
entry points in the header and in the binding, and the fixture captured from the reference."""
import os
import re

import numpy as np
import torch

from conftest import REPO, load_golden

_VARIANTS = dict(n3=dict(F=8, hid=16, n=3, view=False, marcher='classical'), n4mip=dict(F=8, hid=16, n=4, view=False, marcher='mip'),
                 view=dict(F=8, hid=3, n=2, view=True, marcher='classical'), odd=dict(F=12, hid=20, n=2, view=False, marcher='mip'))
NEW_SYMBOLS = ('tdgp_triplane_field_deep', 'tdgp_triplane_field_deep_grad_workspace_bytes', 'tdgp_triplane_field_deep_grad')


def _variant(tdgp, g, tag):
    v = _VARIANTS[tag]
    mlp = tdgp.renderer.TriPlaneMLP(v['F'], v['hid'], out_dim=3, ray_marcher_type=v['marcher'], n_layers=v['n'], has_view_cond=v['view'])
    mlp.load_state_dict({f'model.{i}.{kind}': torch.from_numpy(g[f'{tag}_{kind[0]}{i}']) for i in range(v['n']) for kind in ('weight', 'bias')}, strict=True)
    return mlp


def test_deep_form_selects_three_and_four_layer_decoders(tdgp):
    R = tdgp.renderer
    g = load_golden('mlp_variants')
    for tag in ('n3', 'n4mip'):
        mlp = _variant(tdgp, g, tag)
        assert R.deep_form(mlp) and not R.fused_form(mlp)
        ws, bs, marcher = R._mlp_params_deep(mlp)
        assert len(ws) == len(bs) == _VARIANTS[tag]['n'] and marcher == _VARIANTS[tag]['marcher']
        assert [tuple(w.shape) for w in ws] == [(16, 8)] + [(16, 16)] * (len(ws) - 2) + [(4, 16)]
    for tag in ('view', 'odd'):
        mlp = _variant(tdgp, g, tag)
        assert not R.deep_form(mlp) and not R.fused_form(mlp)
    two = R.TriPlaneMLP(32, 64, n_layers=2)
    assert R.fused_form(two) and not R.deep_form(two)
    ident = R.TriPlaneMLP(4, 8, n_layers=0)
    assert not R.fused_form(ident) and not R.deep_form(ident)
    wide = R.TriPlaneMLP(32, 128, n_layers=3)                 # two hidden layers' operands at 128 do not fit the LDS: eager
    assert not R.fused_form(wide) and not R.deep_form(wide)
    five = R.TriPlaneMLP(32, 64, n_layers=5)
    assert not R.fused_form(five) and not R.deep_form(five)
    for n in (3, 4):
        assert R.deep_form(R.TriPlaneMLP(32, 64, n_layers=n)) and R.deep_form(R.TriPlaneMLP(64, 64, n_layers=n))
    for mlp in (ident, wide, five):
        try:
            R._mlp_params_deep(mlp)
        except NotImplementedError:
            continue
        raise AssertionError('_mlp_params_deep took a decoder outside the deep form')


def test_deep_form_on_a_module_shaped_like_the_reference(tdgp):
    """Any module with `.model[i].weight / .bias` and the marcher under `.cfg`, as the reference's TriPlaneMLP keeps them."""
    class FC(torch.nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.weight, self.bias = torch.nn.Parameter(torch.randn(o, i)), torch.nn.Parameter(torch.zeros(o))

    class RefLike(torch.nn.Module):
        def __init__(self, dims):
            super().__init__()
            self.cfg = type('Cfg', (), dict(ray_marcher_type='mip'))()
            self.model = torch.nn.Sequential(*[FC(a, b) for a, b in zip(dims[:-1], dims[1:])])

    R = tdgp.renderer
    assert R.deep_form(RefLike([32, 64, 64, 4])) and R.deep_form(RefLike([16, 32, 32, 32, 4]))
    assert R._mlp_params_deep(RefLike([32, 64, 64, 4]))[2] == 'mip'
    assert not R.deep_form(RefLike([32, 64, 32, 4]))          # hidden layers are hid x hid
    assert not R.deep_form(RefLike([32, 64, 64, 5]))
    assert R.fused_form(RefLike([32, 64, 4])) and not R.deep_form(RefLike([32, 64, 4]))


def test_header_and_binding_list_the_new_entry_points(tdgp):
    header = open(os.path.join(REPO, 'include', 'tdgp.h')).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'\b' + sym + r'\s*\(', header), f'{sym} is not declared in include/tdgp.h'
        assert sym in tdgp._lib.EXPORTS
    assert 'field_deep.hip' in tdgp.build.SOURCES


def test_fixture_holds_numeric_arrays_only():
    g = load_golden('field_deep')
    assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', 'field_deep.npz')) < 1 << 20
    for k, a in g.items():
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), k
    for tag, n in (('small_n3', 3), ('hot_n4', 4)):
        assert all(f'{tag}_{kind}{i}' in g for i in range(n) for kind in 'wb')
        for marcher in ('classical', 'mip'):
            names = ['rgb', 'sigma', 'd_planes', 'd_coords'] + [f'd_{kind}{i}' for i in range(n) for kind in 'wb']
            for name in names:
                a, d = g[f'{tag}_{marcher}_{name}'], g[f'{tag}_{marcher}_{name}_f64m32']     # fp32 run; float64 run minus fp32 run
                assert a.dtype == np.float32 and d.dtype == np.float32 and a.shape == d.shape
                assert 0 < np.abs(d).max() <= 1e-5 * max(1.0, np.abs(a).max()), (tag, marcher, name)
    outside = np.abs(g['hot_n4_coords']).max(-1) > 0.5
    assert 0.25 < outside.mean() < 0.45                       # a third of the hot points leave the cube
    assert g['hot_n4_coords'].shape[1] == 32 * 5 + 7 and g['small_n3_coords'].shape[1] == 200
    assert all(k in g for k in ('r_planes', 'r_ray_o', 'r_ray_d', 'r_u_coarse', 'r_u_fine', 'r_d_rgb', 'r_d_depth', 'r_rgb', 'r_d_planes', 'r_d_w2', 'r_d_b2'))

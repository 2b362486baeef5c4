"""Mesh components without a GPU: the numpy reference against scipy, `select` on CPU tensors, the tools' new flags, argument validation."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_components_reference as CR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_mc_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_meshes():
    rs3 = np.random.RandomState(3)
    yield 'soup', CR.soup(3000, 2500, 5), 3000
    yield 'strip descending', *CR.strip(5000, numbering=np.arange(5002)[::-1])
    yield 'strip random', *CR.strip(5000, numbering=rs3.permutation(5002))
    yield 'strip with singletons', *CR.strip(257, V=1025)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_labels_agree_with_scipy():
    sp = pytest.importorskip('scipy.sparse')
    from scipy.sparse.csgraph import connected_components
    for name, t, V in random_meshes():
        lab = CR.labels(t, V)
        t64 = t.astype(np.int64)
        i = np.concatenate([t64[:, 0], t64[:, 1]])
        j = np.concatenate([t64[:, 1], t64[:, 2]])
        n, sc = connected_components(sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(V, V)), directed=False)
        # same partition: scipy's label <-> the reference's min-index label is a bijection, and the label is the minimum of its class
        pairs = np.unique(np.stack([sc, lab], 1), axis=0)
        assert len(pairs) == n == len(np.unique(lab)) == len(np.unique(sc)), name
        for k in range(n):
            assert lab[np.flatnonzero(sc == k)[0]] == np.flatnonzero(sc == k).min(), name
        comp, K = CR.component_ids(lab)
        roots = np.flatnonzero(lab == np.arange(V))
        assert K == n and np.array_equal(comp[roots], np.arange(K)) and (comp >= 0).all(), name


def test_reference_properties_on_small_cases():
    assert CR.labels(np.zeros((0, 3), np.int32), 5).tolist() == [0, 1, 2, 3, 4]
    assert CR.labels([[0, 1, 2], [2, 3, 4]], 5).tolist() == [0] * 5                      # one shared vertex joins
    assert CR.labels([[0, 1, 2], [3, 4, 5]], 7).tolist() == [0, 0, 0, 3, 3, 3, 6]
    assert CR.labels([[4, 4, 1], [3, 3, 3], [4, 4, 1]], 5).tolist() == [0, 1, 2, 3, 1]    # degenerate and duplicate triangles
    comp, K = CR.component_ids([0, 0, 0, 3, 3, 3, 6])
    assert K == 3 and comp.tolist() == [0, 0, 0, 1, 1, 1, 2]
    s = CR.stats(CR.CUBE_V, CR.CUBE_T, np.zeros(8, np.int32), 1)
    assert s['area'][0] == 6.0 and abs(s['volume'][0] - 1.0) < 1e-15 and s['triangles'][0] == 12 and s['vertices'][0] == 8
    assert CR.edges_used_twice(CR.CUBE_T) and not CR.edges_used_twice(CR.CUBE_T[:-1])
    v, t, (a,), vmap = CR.compact(CR.CUBE_V[:6], [[0, 1, 2], [3, 4, 5]], [0, 0, 0, 1, 1, 1], [False, True], [np.arange(6, dtype=np.float32)[:, None]])
    assert t.tolist() == [[0, 1, 2]] and vmap.tolist() == [-1, -1, -1, 0, 1, 2] and a[:, 0].tolist() == [3, 4, 5] and np.array_equal(v, CR.CUBE_V[3:6])


# ------------------------------------------------------------------------------------------------ select
def comps(tdgp, triangles, area=None):
    K = len(triangles)
    area = np.asarray(triangles, np.float64) if area is None else np.asarray(area, np.float64)
    return tdgp.mesh_components.Components(torch.zeros(0, dtype=torch.int32), torch.tensor(triangles, dtype=torch.int64), torch.ones(K, dtype=torch.int64),
                                           torch.tensor(area), torch.zeros(K, dtype=torch.float64), torch.zeros(K, 3), torch.zeros(K, 3))


def test_select(tdgp):
    sel = lambda c, **kw: tdgp.mesh_components.select(c, **kw).tolist()             # noqa: E731
    c = comps(tdgp, [10, 0, 300, 40, 0, 7], area=[9.0, 0.0, 2.0, 5.0, 0.0, 1.0])
    assert tdgp.mesh_components.select(c).dtype == torch.bool
    assert sel(c) == [False, False, True, False, False, False]                       # keep=1 by triangles
    assert sel(c, keep=2) == [False, False, True, True, False, False]
    assert sel(c, keep=99) == sel(c, keep='all') == [True, False, True, True, False, True]          # zero-triangle components never kept
    assert sel(c, by='area') == [True, False, False, False, False, False]            # area disagrees with triangles
    assert sel(c, keep=2, by='area') == [True, False, False, True, False, False]
    # min_triangles: inclusive edge
    assert sel(c, keep='all', min_triangles=10) == [True, False, True, True, False, False]
    assert sel(c, keep='all', min_triangles=11) == [False, False, True, True, False, False]
    # min_fraction of the largest measure: inclusive edge (40 / 300 and 5 / 9)
    assert sel(c, keep='all', min_fraction=40 / 300) == [False, False, True, True, False, False]
    assert sel(c, keep='all', min_fraction=np.nextafter(40 / 300, 1)) == [False, False, True, False, False, False]
    assert sel(c, keep='all', by='area', min_fraction=1.0) == [True, False, False, False, False, False]
    # the thresholds come on top of the count: the largest by area has too few triangles, so nothing is left
    assert sel(c, keep=1, by='area', min_triangles=11) == [False] * 6
    # exact ties go to the lower id
    tie = comps(tdgp, [5, 9, 9, 5, 9])
    assert sel(tie) == [False, True, False, False, False]
    assert sel(tie, keep=2) == [False, True, True, False, False]
    assert sel(tie, keep=4) == [True, True, True, False, True]
    assert sel(comps(tdgp, [])) == [] and sel(comps(tdgp, [0, 0])) == [False, False] and sel(c, keep=0) == [False] * 6
    for bad in (dict(by='volume'), dict(keep=-1), dict(keep=1.5), dict(keep=True), dict(min_fraction=1.5), dict(min_triangles=-1)):
        with pytest.raises(ValueError):
            tdgp.mesh_components.select(c, **bad)


# ------------------------------------------------------------------------------------------------ the tools
def test_cli_flags_default_off():
    cli = _tool('extract_geometry')
    a = cli.parse_args(['--num-seeds', '1'])
    assert cli.component_options(a) is None and not hasattr(a, 'keep_components')
    a = cli.parse_args(['--num-seeds', '1', '--keep-components', '2', '--component-by', 'area', '--min-component-triangles', '50'])
    assert cli.component_options(a) == dict(keep=2, by='area', min_triangles=50)
    assert cli.component_options(cli.parse_args(['--num-seeds', '1', '--min-component-triangles', '8'])) == dict(keep='all', by='triangles', min_triangles=8)
    assert cli.component_options(cli.parse_args(['--num-seeds', '1', '--keep-components', 'all'])) == dict(keep='all', by='triangles', min_triangles=0)
    rt = _tool('render_trajectory')
    p = rt.build_parser()
    a = p.parse_args(['--ckpt', 'x', '--out', 'y.gif', '--vis', 'mesh_grid'])
    assert a.keep_components is None and a.min_component_triangles is None and rt.component_options(a) is None and rt.mesh_options(a)['components'] is None
    a = p.parse_args(['--ckpt', 'x', '--out', 'y.gif', '--vis', 'mesh_grid', '--keep-components', '1'])
    assert rt.mesh_options(a)['components'] == dict(keep=1, by='triangles', min_triangles=0)
    for tool, base in ((cli, ['--num-seeds', '1']), (rt, ['--ckpt', 'x', '--out', 'y.gif'])):
        for bad in (['--keep-components', '0'], ['--component-by', 'volume'], ['--min-component-triangles', 'x']):
            with pytest.raises(SystemExit):
                tool.build_parser().parse_args(base + bad)


# ------------------------------------------------------------------------------------------------ validation
def test_entry_points_and_refusals(tdgp):
    M = tdgp.mesh_components
    names = ('tdgp_mesh_labels_workspace_bytes', 'tdgp_mesh_labels', 'tdgp_mesh_component_ids_workspace_bytes', 'tdgp_mesh_component_ids', 'tdgp_mesh_component_stats',
             'tdgp_mesh_component_sums', 'tdgp_mesh_compact_workspace_bytes', 'tdgp_mesh_compact_count', 'tdgp_mesh_compact_emit')
    for name in names:
        assert name in tdgp._lib.EXPORTS
    lib = tdgp._lib.load()
    assert lib.tdgp_mesh_labels_workspace_bytes(10, 1000) >= 4000 and lib.tdgp_mesh_labels_workspace_bytes(-1, 5) == -1 and lib.tdgp_mesh_labels_workspace_bytes(5, 2 ** 31) == -1
    assert lib.tdgp_mesh_compact_workspace_bytes(0, 0) >= 16 and lib.tdgp_mesh_component_ids_workspace_bytes(0) >= 8
    # null pointers and bad sizes are refused before any launch (no GPU here: a launch would fail differently)
    assert lib.tdgp_mesh_labels(None, 5, 5, None, None, 0, None) == -1 and b'mesh_labels' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_component_stats(None, None, -1, 5, None, 1, None, None, None, None, None, None, None, None) == -1
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        M.clean_mesh(v, t)
    with pytest.raises(RuntimeError, match='GPU'):
        M.components(v, t)
    with pytest.raises(RuntimeError, match='GPU'):
        M.vertex_labels(t, 4)
    with pytest.raises(RuntimeError, match='GPU'):
        M.clean_mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    for bad_v, bad_t in ((v.double(), t), (torch.zeros(4, 2), t), (v, t.long()), (v, torch.zeros(2, 4, dtype=torch.int32)), (v, torch.zeros(6, dtype=torch.int32))):
        with pytest.raises(ValueError):
            M.clean_mesh(bad_v, bad_t)
    with pytest.raises(TypeError):
        M.components(v.numpy(), t)
    with pytest.raises(ValueError):
        M.vertex_labels(t, -1)

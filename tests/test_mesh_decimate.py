"""Mesh decimation without a GPU: the properties of the restatement (tests/mesh_decimate_reference.py) that make it worth being the yardstick
-- a closed oriented surface stays one, a box keeps its corners and faces, the rim of an open mesh is untouched, the selected edges of a
round are independent, a soup does no harm -- and the host logic of 3dgp_amd/mesh_decimate.py: argument validation before any launch,
`check_options`, the key's tie-break, the `decimate=` option of the drivers, the two command lines' usage errors, the ABI."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import mesh_components_reference as CR
import mesh_decimate_reference as R
import mesh_raster_reference as MR
import mesh_simplify_reference as SIMP
import mesh_surface_reference as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ['tdgp_mesh_decimate_quadrics', 'tdgp_mesh_decimate_candidates', 'tdgp_mesh_decimate_claim', 'tdgp_mesh_decimate_select_workspace_bytes',
       'tdgp_mesh_decimate_select', 'tdgp_mesh_decimate_apply', 'tdgp_mesh_decimate_gather_workspace_bytes', 'tdgp_mesh_decimate_gather_count',
       'tdgp_mesh_decimate_gather']


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_decimate_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def valid(d, V, T):
    """Triangles index [0, V'), none repeats an index, triangle_map ascends inside [0, T), vertex_map is onto [0, V')."""
    t = np.asarray(d.triangles)
    assert t.dtype == np.int32 and t.shape == (len(d.triangle_map), 3) and d.vertices.dtype == F and d.vertices.shape == (len(d.vertices), 3)
    if len(t):
        assert t.min() >= 0 and t.max() < len(d.vertices)
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
        m = np.asarray(d.triangle_map, np.int64)
        assert (np.diff(m) > 0).all() and m[0] >= 0 and m[-1] < T
    vm = np.asarray(d.vertex_map, np.int64)
    assert vm.shape == (V,) and (V == 0 or (vm.min() >= 0 and vm.max() < len(d.vertices)))
    assert sorted(set(vm.tolist())) == list(range(len(d.vertices)))                             # every output vertex is somebody's
    assert d.stopped in ('target', 'exhausted', 'max_rounds')


@functools.lru_cache(maxsize=None)
def ico_80():
    v, t = MR.icosphere(2)[:2]
    attr = np.random.RandomState(3).rand(len(v), 3).astype(F)
    return v, t, attr, R.decimate(v, t, target_triangles=80, attributes=(attr,))


def test_icosphere_stays_a_closed_oriented_sphere():
    v, t, attr, d = ico_80()
    valid(d, len(v), len(t))
    r = np.linalg.norm(d.vertices.astype(np.float64), axis=1)
    print(f'icosphere(2) -> {len(d.triangles)} triangles, {len(d.vertices)} vertices in {d.rounds} rounds ({d.stopped}); radii [{r.min():.4f}, {r.max():.4f}]')
    assert len(t) == 320 and len(d.triangles) in (80, 79) and d.stopped == 'target'
    assert R.directed_edges_matched(d.triangles)
    assert R.euler(len(d.vertices), d.triangles) == 2
    assert r.min() >= 0.99 and r.max() <= 1.06
    assert R.signed_volume(d.vertices, d.triangles) > 0
    a = d.attributes[0]
    assert a.shape == (len(d.vertices), 3) and a.dtype == F and a.min() >= attr.min() and a.max() <= attr.max()        # convex combinations


def test_the_cache_of_the_restatement_changes_nothing():
    """An edge whose neighbourhood no collapse touched keeps its verdict: re-evaluating every edge every round gives the same bytes."""
    v, t, attr, d = ico_80()
    e = R.decimate(v, t, target_triangles=80, attributes=(attr,), cache=False)
    assert (d.rounds, d.stopped) == (e.rounds, e.stopped)
    for a, b in zip(list(d[:2]) + [d.attributes[0]] + list(d[3:5]), list(e[:2]) + [e.attributes[0]] + list(e[3:5])):
        assert a.tobytes() == b.tobytes()
    v, t, _ = SR.lattice(6)
    a, b = R.decimate(v, t, max_error=0.5), R.decimate(v, t, max_error=0.5, cache=False)
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.triangles.tobytes() == b.triangles.tobytes() and a.rounds == b.rounds


def test_box_comes_down_to_its_twelve_triangles():
    """box(12): every collapse on a face or along an edge costs exactly nothing, and the link condition, the no-flip test and the pinned
    valence keep the eight corners: 1728 -> 12 triangles.  The planes are exact in fp32, so a placed vertex is the exact point rounded once;
    2 ulps of the largest coordinate are allowed, the bound of test_mesh_simplify.py for the same Jacobi."""
    v, t, lo, hi = SIMP.box(12)
    d = R.decimate(v, t, target_triangles=12)
    valid(d, len(v), len(t))
    ulp = float(np.spacing(F(np.abs(np.concatenate([lo, hi])).max())))
    dist = SIMP.box_surface_distance(d.vertices, lo, hi)
    print(f'box(12) -> {len(d.triangles)} triangles in {d.rounds} rounds ({d.stopped}); worst distance from the box {dist.max():.3g}, ulp {ulp:.3g}')
    assert len(t) == 1728 and len(d.triangles) == 12 and len(d.vertices) == 8 and R.directed_edges_matched(d.triangles)
    corners = {(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])}
    assert {tuple(float(c) for c in p) for p in d.vertices} == corners
    assert dist.max() <= 2 * ulp


def test_tetrahedron_and_cube():
    d = R.decimate(SR.TETRA_V, SR.TETRA_T, target_triangles=0)
    assert d.stopped == 'exhausted' and d.rounds == 1                                          # the round that selects nothing is counted
    assert d.vertices.tobytes() == SR.TETRA_V.tobytes() and d.triangles.tobytes() == SR.TETRA_T.tobytes()
    assert d.vertex_map.tolist() == [0, 1, 2, 3] and d.triangle_map.tolist() == [0, 1, 2, 3]
    c = R.decimate(CR.CUBE_V, CR.CUBE_T, target_triangles=0)
    valid(c, 8, 12)
    assert len(c.triangles) == 4 and len(c.vertices) == 4 and c.stopped == 'exhausted' and R.directed_edges_matched(c.triangles)
    assert R.signed_volume(c.vertices, c.triangles) > 0
    same = R.decimate(CR.CUBE_V, CR.CUBE_T, target_triangles=12)
    assert same.rounds == 0 and same.stopped == 'target' and same.vertices.tobytes() == CR.CUBE_V.tobytes() and same.triangles.tobytes() == CR.CUBE_T.tobytes()
    assert R.decimate(CR.CUBE_V, CR.CUBE_T, target_triangles=0, max_rounds=1).stopped == 'max_rounds'


def test_the_rim_of_an_open_lattice_is_pinned():
    v, t, border = SR.lattice(6)
    d = R.decimate(v, t, target_triangles=0)
    valid(d, len(v), len(t))
    print(f'lattice(6): {len(t)} -> {len(d.triangles)} triangles in {d.rounds} rounds')
    assert len(d.triangles) < len(t) and d.stopped == 'exhausted'
    rim = np.flatnonzero(border)
    assert len(set(d.vertex_map[rim].tolist())) == len(rim)                                    # none merged into another
    assert d.vertices[d.vertex_map[rim]].tobytes() == v[rim].tobytes()                         # none moved
    assert (np.bincount(d.vertex_map, minlength=len(d.vertices))[d.vertex_map[rim]] >= 1).all()
    free = R.decimate(v, t, target_triangles=0, fix_boundary=False)
    assert len(free.triangles) <= len(d.triangles)


def test_mix_is_a_bijection_and_matches_the_module(tdgp):
    D = tdgp.mesh_decimate
    sample = list(range(2 ** 15)) + [2 ** 32 - 1 - i * 65521 for i in range(2 ** 15)]
    out = [R.mix(h) for h in sample]
    assert len(set(sample)) == len(set(out)) == 2 ** 16 and all(0 <= o < 2 ** 32 for o in out)
    assert out == [D.mix(h) for h in sample]
    assert R.mix(0) == 0 and len({R.mix(k) >> 28 for k in range(64)}) >= 12                    # neighbouring ids scatter over the high bits
    for T, target in ((320, 80), (321, 80), (81, 80), (80, 80), (10, 0), (5, 9)):
        assert D.max_collapses(T, target) == R.max_collapses(T, target) == max(0, -((target - T) // 2))


def test_selected_edges_are_independent_and_trimming_keeps_the_cheapest():
    v, t = MR.icosphere(3)[:2]
    trace = []
    R.decimate(v, t, target_triangles=0, max_rounds=3, trace=trace)
    assert len(trace) == 3
    for rec in trace:
        N, sel = rec['N'], rec['selected']
        assert len(sel) >= 4 and len({s[5] for s in rec['all']}) == len(rec['all'])
        for i, (_, a, b, c, d, _) in enumerate(sel):
            ring = {a, b} | N[a] | N[b]
            for j, (_, a2, b2, c2, d2, _) in enumerate(sel):
                if i != j:
                    assert not ring & {a2, b2, c2, d2}
        print(f'round: T = {rec["T"]}, {len(sel)} edges selected ({200.0 * len(sel) / rec["T"]:.1f} % of the triangles leave)')
    # the trim: 1280 -> 1270 takes 5 collapses, and they are the 5 smallest keys of what round 0 selected
    trace2 = []
    d = R.decimate(v, t, target_triangles=1270, trace=trace2)
    assert d.rounds == 1 and len(d.triangles) == 1270 and d.stopped == 'target'
    everything = sorted(s[5] for s in trace2[0]['all'])
    assert sorted(s[5] for s in trace2[0]['all']) == sorted(s[5] for s in trace[0]['all']) and len(everything) > 5
    assert sorted(s[5] for s in trace2[0]['selected']) == everything[:5]


def test_a_soup_does_no_harm():
    v, t, (p, q) = R.soup()
    used = sum(1 for x in t if p in x and q in x)
    assert used == 3
    trace = []
    d = R.decimate(v, t, target_triangles=0, trace=trace)
    valid(d, len(v), len(t))
    print(f'soup: {len(t)} -> {len(d.triangles)} triangles, {len(v)} -> {len(d.vertices)} vertices in {d.rounds} rounds ({d.stopped})')
    kept = set(d.triangle_map.tolist())
    bad = [i for i, x in enumerate(t) if min(x) < 0 or max(x) >= len(v) or len(set(x.tolist())) < 3]
    assert len(bad) >= 6 and not kept & set(bad)
    for rec in trace:
        assert not any({a, b} == {p, q} for _, a, b, _, _, _ in rec['selected'])
    assert d.vertex_map[p] != d.vertex_map[q]                                                  # the edge three triangles use is still there
    assert sum(1 for x in d.triangles if d.vertex_map[p] in x and d.vertex_map[q] in x) == 3
    assert (np.diff(d.triangle_map) > 0).all()
    assert R.decimate(v, t, target_triangles=10 ** 6).triangle_map.tolist() == [i for i in range(len(t)) if i not in bad]


def test_arguments_are_checked_before_any_launch(tdgp):
    D = tdgp.mesh_decimate
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    bad = [lambda: D.decimate(v, t), lambda: D.decimate(v, t, target_triangles=-1), lambda: D.decimate(v, t, target_triangles=1.5),
           lambda: D.decimate(v, t, target_triangles=True), lambda: D.decimate(v, t, max_error=0.0), lambda: D.decimate(v, t, max_error=-1.0),
           lambda: D.decimate(v, t, max_error=float('nan')), lambda: D.decimate(v, t, max_error=float('inf')), lambda: D.decimate(v, t, 10, max_rounds=-1),
           lambda: D.decimate(v, t, 10, max_rounds=2.0), lambda: D.decimate(v, t, 10, rank_tol=-1.0), lambda: D.decimate(v, t, 10, rank_tol=float('nan')),
           lambda: D.decimate(v.double(), t, 10), lambda: D.decimate(v[:, :2], t, 10), lambda: D.decimate(v, t.long(), 10), lambda: D.decimate(v, t.reshape(6), 10),
           lambda: D.check_options(dict()), lambda: D.check_options(dict(target_triangles=10, colour='red')), lambda: D.check_options(dict(max_error=-2.0)),
           lambda: D.check_options(dict(target_triangles=1.5)), lambda: D.check_options(dict(target_triangles=10, max_rounds=-1)),
           lambda: tdgp.geometry.extract_geometry(None, None, decimate=dict(target_triangles=-5)),
           lambda: tdgp.mesh_build.check_stages(None, None, None, None, dict(cell=2.0))]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'call {k} did not raise')
    for call in (lambda: D.check_options(2.0), lambda: D.decimate(v, t, max_error='wide'), lambda: D.decimate(v, t, 10, fix_boundary=1), lambda: D.decimate([0], t, 10),
                 lambda: D.check_options(dict(target_triangles=10, rank_tol='small'))):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError, match="unknown options \\['colour'\\]; known: .*'fix_boundary', 'max_error', 'max_rounds', 'rank_tol', 'target_triangles'"):
        D.check_options(dict(colour=1))
    for call in (lambda: D.decimate(v, t, 10), lambda: D.decimate(v, t, max_error=0.5), lambda: D.apply(v, t, dict(target_triangles=1))):
        with pytest.raises(RuntimeError, match='GPU'):                                            # well-formed, on the host: the kernels have no CPU path
            call()
    opts = dict(target_triangles=100, max_error=0.5, max_rounds=7, rank_tol=1e-2, fix_boundary=False)
    assert D.check_options(opts) == opts and D.check_options(opts) is not opts and D.check_options(dict(max_error=1)) == dict(max_error=1)
    st = tdgp.mesh_build.check_stages(None, None, None, None)
    assert st.decimate is None and st._fields[-1] == 'decimate' and tdgp.mesh_build.check_stages(None, None, None, None, decimate=opts).decimate == opts
    assert tdgp.mesh_build.Stages(1, 2, 3, 4, 5) == (1, 2, 3, 4, 5, None)                       # the trailing field has a default
    c = tdgp.geometry.MeshCount(7, 9, 30)
    assert c.decimate is None and c == (7, 9) and c.triangles_before == 30


def test_tools_usage_errors(capsys):
    ex, rt = _tool('extract_geometry'), _tool('render_trajectory')
    base = ['--seeds', '0']
    a = ex.parse_args(base)
    assert ex.decimate_options(a) is None and not any(k.startswith('decimate') for k in vars(a))
    assert ex.decimate_options(ex.parse_args(base + ['--decimate-triangles', '5000'])) == dict(target_triangles=5000)
    assert ex.decimate_options(ex.parse_args(base + ['--decimate-max-error', '0.25'])) == dict(max_error=0.25)
    assert ex.decimate_options(ex.parse_args(base + ['--decimate-triangles', '0', '--decimate-max-error', '0.5', '--simplify-cell', '2'])) == dict(target_triangles=0, max_error=0.5)
    for extra in (['--decimate-triangles', '-4'], ['--decimate-triangles', '2.5'], ['--decimate-max-error', '0'], ['--decimate-max-error', 'nan'], ['--decimate-max-error', 'inf']):
        with pytest.raises(SystemExit):
            ex.parse_args(base + extra)
    p = rt.build_parser()
    base = ['--ckpt', 'x', '--out', 'y.npy']
    a = p.parse_args(base + ['--vis', 'mesh_grid', '--mesh-decimate-triangles', '300'])
    assert rt.mesh_options(a)['decimate'] == dict(target_triangles=300) and 'decimate' not in rt.mesh_options(p.parse_args(base + ['--vis', 'mesh_strips']))
    for extra in (['--mesh-decimate-triangles', '20'], ['--vis', 'shape_grid', '--mesh-decimate-triangles', '20'], ['--vis', 'mesh_grid', '--mesh-decimate-triangles', '-1'],
                  ['--vis', 'mesh_strips', '--mesh-decimate-triangles', '1.5']):
        with pytest.raises(SystemExit):
            p.parse_args(base + extra)
    capsys.readouterr()


def test_entry_points_are_declared_bound_and_refuse_what_they_cannot_index(tdgp):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'tdgp.h')).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf'\b{name}\s*\(', header) and name in tdgp._lib.EXPORTS
    assert sorted(n for n in tdgp._lib.EXPORTS if n.startswith('tdgp_mesh_decimate')) == sorted(NEW)
    assert 'mesh_decimate.hip' in tdgp.build.SOURCES and 'quadric_solve.h' in tdgp.build.HEADERS
    for f in ('mesh_simplify.hip', 'mesh_decimate.hip'):                                          # one Jacobi, in the header both compile
        src = open(os.path.join(REPO, '3dgp_amd', 'csrc', f)).read()
        assert '#include "quadric_solve.h"' in src and 'quadric_minimise(' in src and 'void jacobi_rotate' not in src
    lib = tdgp._lib.load()
    assert lib.tdgp_mesh_decimate_select_workspace_bytes(2 ** 31 // 3 + 1) == -1 and lib.tdgp_mesh_decimate_select_workspace_bytes(-1) == -1
    assert lib.tdgp_mesh_decimate_gather_workspace_bytes(2 ** 31 - 1) == -1 and lib.tdgp_mesh_decimate_gather_workspace_bytes(-1) == -1
    assert lib.tdgp_mesh_decimate_gather_workspace_bytes(0) == 64 and lib.tdgp_mesh_decimate_gather_workspace_bytes(257) == 128
    assert lib.tdgp_mesh_decimate_select_workspace_bytes(86) == 128 and lib.tdgp_mesh_decimate_select_workspace_bytes(2 ** 31 // 3) > 0
    # the argument checks of the C side come before any launch: they answer without a device
    assert lib.tdgp_mesh_decimate_quadrics(None, None, 2 ** 31 // 3 + 1, 4, None, None, None, None, None, None) == -1 and b'2^31 - 1' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_quadrics(None, None, 4, 4, None, None, None, None, None, None) == -1 and b'null pointer' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_candidates(None, None, None, None, None, 4, 4, None, None, -1.0, 1e-3, None, None, None, None) == -1 and b'max_error' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_candidates(None, None, None, None, None, 4, 4, None, None, 0.0, float('nan'), None, None, None, None) == -1 and b'rank_tol' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_candidates(None, None, None, None, None, 4, 4, None, None, 0.5, 1e-3, None, None, None, None) == -1 and b'null pointer' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_claim(None, None, 4, 2 ** 31 - 1, None, None, None, None) == -1 and b'2^31 - 2' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_select(None, None, None, None, 4, 4, None, None, None, 0, None) == -1 and b'null workspace' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_apply(None, 13, None, 4, 4, None, None, None, None, None, None, 0, None, None) == -1 and b'K' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_apply(None, 3, None, 4, 4, None, None, None, None, None, None, 5000, None, None) == -1 and b'channels' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_gather(None, None, 0, None, 4, 1, None, 0, None, 5, None, None, None) == -1 and b'V_out' in lib.tdgp_last_error()
    assert lib.tdgp_mesh_decimate_gather(None, None, 0, None, 4, -1, None, 0, None, 2, None, None, None) == -1 and b'max_hops' in lib.tdgp_last_error()
    # empty inputs are no-ops that need no device
    assert lib.tdgp_mesh_decimate_quadrics(None, None, 0, 0, None, None, None, None, None, None) == 0
    assert lib.tdgp_mesh_decimate_candidates(None, None, None, None, None, 0, 0, None, None, 0.0, 1e-3, None, None, None, None) == 0
    assert lib.tdgp_mesh_decimate_apply(None, 0, None, 4, 4, None, None, None, None, None, None, 0, None, None) == 0

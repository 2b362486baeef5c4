"""Mesh components on the GPU: labels, dense ids, per-component measurements and the compaction against the numpy reference
(tests/mesh_components_reference.py) -- integers exactly, fp64 sums to the summation bound and bit-identical between runs -- and the
`components=` option of geometry.extract_geometry / mesh.render_mesh_frames on a seeded config_tiny scene, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import mesh_components_reference as CR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32


def T(a):
    if isinstance(a, np.ndarray) and not a.flags.writeable:              # the shared, read-only test meshes
        a = a.copy()
    return torch.as_tensor(a).to(DEV)


def H(t):
    return t.detach().cpu().numpy()


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        first = tuple(bad[0]) if len(bad) else ()
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}')


def device_labels(tdgp, tris, V):
    return H(tdgp.mesh_components.vertex_labels(T(np.asarray(tris, np.int32).reshape(-1, 3)), V))


@functools.lru_cache(maxsize=None)
def named_mesh(name):
    """(triangles int32 [T,3], V, reference labels): computed once, shared, never written."""
    if name == 'descending':
        t, V = CR.strip(5000, numbering=np.arange(5002)[::-1])
    elif name == 'random':
        t, V = CR.strip(5000, numbering=np.random.RandomState(3).permutation(5002))
    elif name == 'soup':
        t, V = CR.soup(3000, 2500, 5), 3000
    elif name == 'sparse soup':                                # below the giant-component threshold: many small components with triangles
        t, V = CR.soup(3000, 700, 9), 3000
    else:
        raise KeyError(name)
    lab = CR.labels(t, V)
    for a in (t, lab):
        a.setflags(write=False)
    return t, V, lab


def check_label_properties(lab, tris, V):
    lab = lab.astype(np.int64)
    assert lab.shape == (V,) and (lab <= np.arange(V)).all() and (lab >= 0).all()
    assert np.array_equal(lab[lab], lab)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    if len(t):
        assert (lab[t[:, 0]] == lab[t[:, 1]]).all() and (lab[t[:, 1]] == lab[t[:, 2]]).all()


# ------------------------------------------------------------------------------------------------ labels
EDGE_CASES = {
    'nothing': ([], 0),
    'five singletons': ([], 5),
    'one triangle': ([(0, 1, 2)], 3),
    'two disjoint': ([(0, 1, 2), (3, 4, 5)], 6),
    'sharing one vertex': ([(0, 1, 2), (2, 3, 4)], 5),
    'degenerate and duplicate': ([(4, 4, 1), (3, 3, 3), (4, 4, 1), (0, 6, 0), (6, 0, 6)], 8),
    'unreferenced between referenced': ([(0, 2, 4), (6, 8, 10), (10, 4, 4)], 12),
}


@pytest.mark.parametrize('name', list(EDGE_CASES))
def test_labels_edge_cases(tdgp, name):
    tris, V = EDGE_CASES[name]
    got = device_labels(tdgp, tris, V)
    same_bytes(got, CR.labels(tris, V), name)
    check_label_properties(got, tris, V)


def test_labels_edge_cases_hold_what_they_say(tdgp):
    assert device_labels(tdgp, *EDGE_CASES['five singletons']).tolist() == [0, 1, 2, 3, 4]
    assert device_labels(tdgp, *EDGE_CASES['two disjoint']).tolist() == [0, 0, 0, 3, 3, 3]
    assert device_labels(tdgp, *EDGE_CASES['sharing one vertex']).tolist() == [0] * 5
    assert device_labels(tdgp, *EDGE_CASES['degenerate and duplicate']).tolist() == [0, 1, 2, 3, 1, 5, 0, 7]
    assert device_labels(tdgp, *EDGE_CASES['unreferenced between referenced']).tolist() == [0, 1, 0, 3, 0, 5, 0, 7, 0, 9, 0, 11]


def test_labels_at_block_edges(tdgp):
    """256 triangles / vertices per block: one less, exactly, one more (and four blocks of vertices likewise); the tail vertices are singletons."""
    for nt in (255, 256, 257):
        for V in (1023, 1024, 1025):
            tris, _ = CR.strip(nt, V=V)
            got = device_labels(tdgp, tris, V)
            want = np.arange(V, dtype=np.int32)
            want[:nt + 2] = 0
            same_bytes(got, want, f'strip T={nt} V={V}')


@pytest.mark.parametrize('name', ['descending', 'random', 'soup', 'sparse soup'])
def test_labels_deep_chains_and_soup(tdgp, name):
    """The strips are the inputs on which parent chains get long and compare-and-swap retries pile up (5 000 triangles, vertices numbered
    against the strip / at random); the soup (3 000 vertices, 2 500 random triples) is one giant component next to 244 unreferenced vertices."""
    tris, V, want = named_mesh(name)
    got, retries = tdgp.mesh_components.vertex_labels(T(tris), V, return_retries=True)
    print(f'{name}: {len(np.unique(want))} components, {retries} compare-and-swap retries')
    same_bytes(H(got), want, name)
    check_label_properties(H(got), tris, V)
    assert retries >= 0
    if 'soup' not in name:
        assert (want == 0).all()
    else:
        assert 100 < len(np.unique(want)) < V


@pytest.mark.parametrize('name', ['random', 'soup', 'sparse soup'])
def test_label_invariances(tdgp, name):
    tris, V, want = named_mesh(name)
    rs = np.random.RandomState(11)
    same_bytes(device_labels(tdgp, tris[rs.permutation(len(tris))], V), want, 'permuted triangles')
    same_bytes(device_labels(tdgp, tris[:, [2, 0, 1]], V), want, 'rotated corners')
    perm = rs.permutation(V).astype(np.int32)                 # vertex v becomes perm[v]
    got = device_labels(tdgp, perm[tris], V)
    check_label_properties(got, perm[tris], V)
    pairs = np.unique(np.stack([want, got[perm]], 1), axis=0)  # the same partition: the two labellings are in bijection
    assert len(pairs) == len(np.unique(want)) == len(np.unique(got))


# ------------------------------------------------------------------------------------------------ marching-cubes input
@pytest.fixture(scope='module')
def mc_mesh(tdgp):
    verts, tris = tdgp.geometry.marching_cubes(T(CR.speck_volume(24)), 0.0)
    return verts, tris


def reference_components(verts, tris):
    lab = CR.labels(H(tris), verts.shape[0])
    comp, K = CR.component_ids(lab)
    return comp, K, CR.stats(H(verts), H(tris), comp, K)


def test_marching_cubes_volume_has_five_closed_components(tdgp, mc_mesh):
    verts, tris = mc_mesh
    M = tdgp.mesh_components
    c = M.components(verts, tris)
    comp, K, want = reference_components(verts, tris)
    assert K == 5 and c.triangles.shape[0] == 5
    same_bytes(H(c.component), comp, 'component')
    t = H(tris)
    for k in range(K):
        assert CR.edges_used_twice(t[comp[t[:, 0]] == k]), f'component {k} is not closed'
    assert sorted(H(c.triangles).tolist())[:3] == [8, 8, 8]                       # a single voxel above the level is an octahedron
    big = int(H(M.select(c, keep=1)).nonzero()[0][0])
    lo, hi = H(c.bbox_min)[big], H(c.bbox_max)[big]
    centre, r = np.array([7.2, 7.9, 8.1]), 5.3                                     # the larger sphere of speck_volume
    assert np.abs((lo + hi) / 2 - centre).max() < 0.5 and np.abs((hi - lo) / 2 - r).max() < 0.5
    assert (H(c.volume) > 0).all()                                                # blobs of high density: positive under marching cubes' winding
    assert abs(H(c.volume)[big] - 4 / 3 * np.pi * r ** 3) < 0.05 * 4 / 3 * np.pi * r ** 3


# ------------------------------------------------------------------------------------------------ stats
def check_stats(c, want, what):
    same_bytes(H(c.triangles), want['triangles'], 'triangle counts ' + what)
    same_bytes(H(c.vertices), want['vertices'], 'vertex counts ' + what)
    same_bytes(H(c.bbox_min), want['bbox_min'], 'bbox_min ' + what)
    same_bytes(H(c.bbox_max), want['bbox_max'], 'bbox_max ' + what)
    n = want['triangles'].astype(np.float64)
    worst = 0.0
    for name in ('area', 'volume'):
        got = H(getattr(c, name))
        assert got.dtype == np.float64
        bound = (n + 8) * 2.0 ** -52 * want['abs_' + name]
        err = np.abs(got - want[name])
        with np.errstate(divide='ignore', invalid='ignore'):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))) if len(err) else 0.0)
        assert (err <= bound).all(), f'{name} {what}: {int((err > bound).sum())} components beyond (n + 8) 2^-52 sum|term|, worst {float((err - bound).max()):.3e}'
    print(f'{what}: worst |got - want| / bound = {worst:.3f}')


def test_stats_exact_cubes(tdgp):
    M = tdgp.mesh_components
    c = M.components(T(CR.CUBE_V), T(CR.CUBE_T))
    assert H(c.area).tolist() == [6.0] and H(c.volume).tolist() == [1.0] and H(c.triangles).tolist() == [12] and H(c.vertices).tolist() == [8]
    c = M.components(T(CR.CUBE_V), T(np.ascontiguousarray(CR.CUBE_T[:, ::-1])))
    assert H(c.area).tolist() == [6.0] and H(c.volume).tolist() == [-1.0]
    off = np.array([3.0, -1.0, 0.5], F)
    v2 = np.concatenate([CR.CUBE_V, CR.CUBE_V * 2 + off]).astype(F)
    t2 = np.concatenate([CR.CUBE_T, CR.CUBE_T + 8]).astype(np.int32)
    c = M.components(T(v2), T(t2))
    assert H(c.component).tolist() == [0] * 8 + [1] * 8 and H(c.triangles).tolist() == [12, 12] and H(c.vertices).tolist() == [8, 8]
    same_bytes(H(c.bbox_min), np.array([[0, 0, 0], off], F), 'bbox_min')
    same_bytes(H(c.bbox_max), np.array([[1, 1, 1], off + 2], F), 'bbox_max')
    # dyadic coordinates: every product and sum is exact in fp64, and the division by 6 is applied once to the exact sum
    assert H(c.area).tolist() == [6.0, 24.0] and H(c.volume).tolist() == [1.0, 8.0]


def test_stats_marching_cubes_volume(tdgp, mc_mesh):
    verts, tris = mc_mesh
    c = tdgp.mesh_components.components(verts, tris)
    check_stats(c, reference_components(verts, tris)[2], 'mc volume')
    again = tdgp.mesh_components.components(verts, tris)
    same_bytes(H(again.area), H(c.area), 'area, second run')
    same_bytes(H(again.volume), H(c.volume), 'volume, second run')


@pytest.mark.parametrize('name', ['soup', 'sparse soup'])
def test_stats_random_soup(tdgp, name):
    tris, V, lab = named_mesh(name)
    verts = (np.random.RandomState(6).randn(V, 3) * 3).astype(F)
    comp, K = CR.component_ids(lab)
    c = tdgp.mesh_components.components(T(verts), T(tris))
    same_bytes(H(c.component), comp, 'component')
    check_stats(c, CR.stats(verts, tris, comp, K), name)
    again = tdgp.mesh_components.components(T(verts), T(tris))
    same_bytes(H(again.area), H(c.area), 'area, second run')
    same_bytes(H(again.volume), H(c.volume), 'volume, second run')
    assert int(H(c.triangles).sum()) == len(tris) and int(H(c.vertices).sum()) == V


# ------------------------------------------------------------------------------------------------ compaction
def check_compaction(tdgp, verts, tris, mask, attributes, what):
    M = tdgp.mesh_components
    tv, tt = T(verts), T(tris)
    comps = M.components(tv, tt)
    got_v, got_t, got_a, got_map = M.keep_components(tv, tt, comps, T(mask), attributes=tuple(T(a) for a in attributes))
    want_v, want_t, want_a, want_map = CR.compact(verts, tris, H(comps.component), mask, attributes)
    same_bytes(H(got_v).view(np.uint32), want_v.view(np.uint32), 'vertices ' + what)
    same_bytes(H(got_t), want_t, 'triangles ' + what)
    same_bytes(H(got_map), want_map, 'vertex_map ' + what)
    assert len(got_a) == len(attributes)
    for i, (g, w) in enumerate(zip(got_a, want_a)):
        same_bytes(H(g).view(np.uint32), w.view(np.uint32), f'attribute {i} {what}')
    kept = want_map[want_map >= 0]
    assert np.array_equal(kept, np.arange(len(kept)))                             # order preserved: the map is increasing over the kept vertices
    return got_v, got_t, comps


def test_compaction_soup_and_trivial_masks(tdgp):
    tris, V, lab = named_mesh('sparse soup')
    rs = np.random.RandomState(8)
    verts = rs.randn(V, 3).astype(F)
    attrs = [rs.rand(V, 3).astype(F), rs.rand(V, 1).astype(F)]
    K = len(np.unique(lab))
    assert len(np.unique(lab[tris[:, 0]])) > 100                                  # over a hundred components with triangles, 1 to 441 each
    mask = rs.rand(K) < 0.5
    got_v, got_t, comps = check_compaction(tdgp, verts, tris, mask, attrs, 'soup, random half')
    assert 0 < got_v.shape[0] < V and 0 < got_t.shape[0] < len(tris)
    # kept triangles keep their order: re-indexed back, they are the kept rows of the input in sequence
    vmap = CR.compact(verts, tris, H(comps.component), mask)[3]
    back = np.flatnonzero(vmap >= 0)[H(got_t)]
    assert np.array_equal(back, tris[mask[H(comps.component)[tris[:, 0]]]])
    all_v, all_t, _ = check_compaction(tdgp, verts, tris, np.ones(K, bool), attrs, 'soup, all ones')
    same_bytes(H(all_v).view(np.uint32), verts.view(np.uint32), 'all ones returns the vertices')
    same_bytes(H(all_t), tris, 'all ones returns the triangles')
    none_v, none_t, _ = check_compaction(tdgp, verts, tris, np.zeros(K, bool), attrs, 'soup, all zeros')
    assert tuple(none_v.shape) == (0, 3) and tuple(none_t.shape) == (0, 3)


def test_compaction_at_block_edges(tdgp):
    for V in (1023, 1024, 1025):
        for nt in (255, 256, 257):
            rs = np.random.RandomState(V + nt)
            tris = CR.soup(V, nt, V * 7 + nt)
            verts = rs.randn(V, 3).astype(F)
            K = CR.component_ids(CR.labels(tris, V))[1]
            check_compaction(tdgp, verts, tris, rs.rand(K) < 0.6, [rs.rand(V, 2).astype(F)], f'V={V} T={nt}')


def test_more_than_1024_blocks_of_vertices(tdgp):
    """The one-block scan of the block sums takes runs of 2 sums per thread from 1025 blocks on: a strip of 257 triangles on 1024 * 256 + 257
    vertices is 1026 blocks of vertices, nearly all of them singletons.  Every expectation is written down directly."""
    M = tdgp.mesh_components
    nt, V = 257, 1024 * 256 + 257
    assert -(-V // 256) == 1026
    tris, _ = CR.strip(nt, V=V)
    v = np.arange(V, dtype=np.int32)
    same_bytes(device_labels(tdgp, tris, V), np.where(v < nt + 2, 0, v).astype(np.int32), 'labels')
    verts = np.random.RandomState(11).randn(V, 3).astype(F)
    attr = np.random.RandomState(12).rand(V, 2).astype(F)
    tv, tt = T(verts), T(tris)
    comps = M.components(tv, tt)
    K = V - (nt + 1)
    want_ids = np.where(v < nt + 2, 0, v - (nt + 1)).astype(np.int32)
    same_bytes(H(comps.component), want_ids, 'dense ids')
    assert tuple(comps.triangles.shape) == (K,) and int(comps.triangles[0]) == nt and int(comps.vertices[0]) == nt + 2
    for first in (0, 1):                                        # the strip's component kept with every other singleton, then dropped
        mask = (np.arange(K) % 2 == first)
        kept = mask[want_ids]
        vmap = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int32)
        want_t = vmap[tris] if mask[0] else np.zeros((0, 3), np.int32)
        got_v, got_t, (got_a,), got_map = M.keep_components(tv, tt, comps, T(mask), attributes=(T(attr),))
        what = f'mask {first}::2'
        assert (got_v.shape[0], got_t.shape[0]) == (int(kept.sum()), len(want_t)), what
        same_bytes(H(got_map), vmap, 'vertex_map ' + what)
        same_bytes(H(got_v).view(np.uint32), verts[kept].view(np.uint32), 'vertices ' + what)
        same_bytes(H(got_a).view(np.uint32), attr[kept].view(np.uint32), 'attribute ' + what)
        same_bytes(H(got_t), want_t, 'triangles ' + what)


def test_clean_mesh_keeps_the_larger_sphere_and_passes_empty_meshes(tdgp, mc_mesh):
    M = tdgp.mesh_components
    verts, tris = mc_mesh
    colours = torch.rand(verts.shape[0], 3, device=DEV)
    v, t, (a,), vmap, comps, mask = M.clean_mesh(verts, tris, attributes=(colours,), return_components=True, keep=1)
    big = int(H(mask).nonzero()[0][0])
    assert int(mask.sum()) == 1 and v.shape[0] == int(comps.vertices[big]) and t.shape[0] == int(comps.triangles[big])
    assert torch.equal(v, verts[vmap >= 0]) and torch.equal(a, colours[vmap >= 0]) and CR.edges_used_twice(H(t))
    again = M.components(v, t)
    assert again.triangles.shape[0] == 1 and torch.equal(again.area, comps.area[big:big + 1])      # the same terms in the same order
    v2, t2, a2, vmap2 = M.clean_mesh(verts, tris, keep=2, min_triangles=9)
    assert M.components(v2, t2).triangles.shape[0] == 2 and a2 == ()
    e_v, e_t = torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV)
    v, t, a, vmap = M.clean_mesh(e_v, e_t, attributes=(torch.empty(0, 2, device=DEV),))
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and tuple(a[0].shape) == (0, 2) and tuple(vmap.shape) == (0,) and t.dtype == torch.int32
    v, t, a, vmap = M.clean_mesh(verts[:7], e_t)                                   # isolated vertices only: never kept
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and H(vmap).tolist() == [-1] * 7


def test_index_out_of_range_raises_before_any_launch(tdgp):
    M = tdgp.mesh_components
    v = torch.zeros(4, 3, device=DEV)
    good = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    for bad in ([[0, 1, 4]], [[0, -1, 2]], [[0, 1, 2], [2 ** 31 - 1, 0, 1]]):
        t = torch.tensor(bad, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match='outside'):
            M.components(v, t)
        with pytest.raises(ValueError, match='outside'):
            M.vertex_labels(t, 4)
        with pytest.raises(ValueError, match='outside'):
            M.clean_mesh(v, t)
    comps = M.components(v, good)
    with pytest.raises(ValueError, match='mask'):
        M.keep_components(v, good, comps, torch.ones(5, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match='attribute'):
        M.clean_mesh(v, good, attributes=(torch.zeros(3, 2, device=DEV),))


# ------------------------------------------------------------------------------------------------ wiring
B, NV, VOL = 2, 3, 24


@pytest.fixture(scope='module')
def scene(tdgp):
    """config_tiny, seeded weights, 2 samples x 3 cameras, volume_res 24 over the whole field.  The level is picked from the density grids: the
    first of a few quantiles at which every sample's level set has at least two components with triangles; if there is none, `specks` (added
    to sigma through a monkeypatch of the two density-grid functions) makes some."""
    cfg = tdgp.config.config_tiny()
    G = tdgp.generator.Generator(cfg)
    G.load_numpy_state_dict(tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    G = G.to(DEV).eval()
    inp = tdgp.weights.synthetic_inputs(cfg, batch=B, seed=12)
    ws = G.mapping(T(inp['z']), T(inp['c']))
    cam_np = tdgp.weights.synthetic_inputs(cfg, batch=B * NV, seed=13)['camera']
    cams = tdgp.generator.TensorGroup(**{k: T(v) for k, v in cam_np.items()})
    box = 2.0 * cfg.cube_scale
    with torch.no_grad():
        grid = tdgp.geometry.density_grid(G, ws, volume_res=VOL, cube_size=box)

    def pieces(vol, level):
        v, t = tdgp.geometry.marching_cubes(vol, level)
        return int((tdgp.mesh_components.components(v, t).triangles > 0).sum()) if v.shape[0] else 0

    level, specks = None, None
    for q in (0.5, 0.6, 0.7, 0.8, 0.9, 0.4, 0.3):
        cand = float(grid.flatten().quantile(q))
        if all(pieces(grid[b], cand) >= 2 for b in range(B)):
            level = cand
            break
    if level is None:
        level = float(grid.median())
        specks = torch.zeros(VOL, VOL, VOL, device=DEV)
        lift = float(grid.max() - grid.min()) + 1.0
        below = (grid < level).all(dim=0)                                   # voxels below the level in every sample, and so are their six neighbours
        low = below[1:-1, 1:-1, 1:-1]
        for shift, axis in ((1, 0), (-1, 0), (1, 1), (-1, 1), (1, 2), (-1, 2)):
            low = low & below.roll(shift, axis)[1:-1, 1:-1, 1:-1]
        idx = low.nonzero()[:3] + 1
        assert len(idx) >= 1, 'no room for a speck'
        for d, h, w in idx.tolist():
            specks[d, h, w] = lift
    return dict(G=G, ws=ws, cams=cams, level=level, specks=specks, box=box, res=G.synthesis.test_resolution)


@pytest.fixture
def patched(tdgp, scene, monkeypatch):
    """The scene, with the speck volume added to every density grid the product builds when the scene needed one."""
    if scene['specks'] is not None:
        g = tdgp.geometry
        grid_fn, planes_fn = g.density_grid, g.density_grid_from_planes
        monkeypatch.setattr(g, 'density_grid', lambda *a, **k: grid_fn(*a, **k) + scene['specks'])
        monkeypatch.setattr(g, 'density_grid_from_planes', lambda *a, **k: planes_fn(*a, **k) + scene['specks'])
    return scene


def test_extract_geometry_with_components(tdgp, patched):
    g, M = tdgp.geometry, tdgp.mesh_components
    sc = patched
    kw = dict(volume_res=VOL, cube_size=sc['box'], thresh_value=sc['level'], crop=None)
    cleaned = g.extract_geometry(sc['G'], sc['ws'], components=dict(keep=1), **kw)
    world = g.extract_geometry(sc['G'], sc['ws'], components=dict(keep=1), units='world', **kw)
    plain = g.extract_geometry(sc['G'], sc['ws'], **kw)
    none = g.extract_geometry(sc['G'], sc['ws'], components=None, **kw)
    assert len(cleaned) == B and cleaned[0]._fields == ('vertices', 'triangles', 'sigma')
    for b in range(B):
        for f in ('vertices', 'triangles', 'sigma'):
            assert torch.equal(getattr(plain[b], f), getattr(none[b], f)), f
        sigma = g.density_grid(sc['G'], sc['ws'][b:b + 1], VOL, (0.0, 0.0, 0.0), sc['box'])[0]
        v, t = g.marching_cubes(sigma, sc['level'])
        assert (M.components(v, t).triangles > 0).sum() >= 2
        cv, ct, _, _ = M.clean_mesh(v, t, keep=1)
        assert 0 < ct.shape[0] < t.shape[0] and M.components(cv, ct).triangles.shape[0] == 1
        diag = (cv.max(dim=0).values - cv.min(dim=0).values).norm()
        assert torch.equal(cleaned[b].vertices, cv / diag) and torch.equal(cleaned[b].triangles, ct) and torch.equal(cleaned[b].sigma, sigma)
        assert torch.equal(world[b].vertices, g.grid_to_world(cv, VOL, (0.0, 0.0, 0.0), sc['box'], None)) and torch.equal(world[b].triangles, ct)
        assert plain[b].triangles.shape[0] == t.shape[0]


def test_render_mesh_frames_with_components(tdgp, patched):
    g, M, Me = tdgp.geometry, tdgp.mesh_components, tdgp.mesh
    sc = patched
    G, res = sc['G'], sc['res']
    kw = dict(level=sc['level'], volume_res=VOL)
    frames, counts = Me.render_mesh_frames(G, sc['ws'], sc['cams'], components=dict(keep=1), return_counts=True, **kw)
    raw, raw_counts = Me.render_mesh_frames(G, sc['ws'], sc['cams'], return_counts=True, **kw)
    none = Me.render_mesh_frames(G, sc['ws'], sc['cams'], components=None, **kw)
    for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
        assert torch.equal(getattr(raw, k), getattr(none, k)), k
    planes = G.synthesis.tri_planes(sc['ws'], noise_mode='const')
    for b in range(B):
        pb = tdgp.renderer.HWCPlanes(planes.t[b:b + 1])
        sigma = g.density_grid_from_planes(G, pb, VOL, (0.0, 0.0, 0.0), sc['box'])[0]
        v, t = g.marching_cubes(sigma, sc['level'])
        cv, ct, _, _ = M.clean_mesh(v, t, keep=1)
        assert counts[b] == (cv.shape[0], ct.shape[0]) and raw_counts[b] == (v.shape[0], t.shape[0]) and counts[b][1] < raw_counts[b][1]
        world = g.grid_to_world(cv, VOL, (0.0, 0.0, 0.0), sc['box'], None)
        want = Me.render_mesh_views(world, ct, Me._camera_slice(sc['cams'], DEV, b * NV, (b + 1) * NV), res, G=G)
        for k in ('rgb', 'depth', 'normal', 'status', 'tri'):
            assert torch.equal(getattr(frames, k)[b * NV:(b + 1) * NV], getattr(want, k)), (b, k)
    assert int(frames.status.sum()) > 0
    grid = Me.render_mesh_video_grid(G, sc['ws'], sc['cams'], components=dict(keep=1), **kw)                 # passed through **kw
    assert grid.dtype == torch.uint8 and grid.shape[0] == NV


# ------------------------------------------------------------------------------------------------ the tools
def _tool(name):
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('tool_mc_gpu_' + name, os.path.join(repo, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_take_the_component_flags(tdgp, tmp_path, capsys):
    """Both command lines on a seeded config_tiny checkpoint: the extraction tool writes the cleaned mesh and, verbose, reports components found /
    kept and triangles dropped; the trajectory tool draws the cleaned meshes and names the filter in its JSON line."""
    import json
    import re
    cfg = tdgp.config.config_tiny()
    with open(tmp_path / 'generator.json', 'w') as f:
        json.dump(cfg.to_dict(), f)
    np.savez(tmp_path / 'generator.npz', **tdgp.weights.random_state_dict(cfg, seed=33, exercise_all=True))
    ex = _tool('extract_geometry')
    common = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--volume-res', '24', '--cube-size', str(2.0 * cfg.cube_scale), '--thresh-value', '0.0', '--save-ply', '--no-save-mrc']
    ex.main(common + ['--output-dir', str(tmp_path / 'raw')])
    raw_out = capsys.readouterr().out
    ex.main(common + ['--output-dir', str(tmp_path / 'clean'), '--keep-components', '1'])
    out = capsys.readouterr().out
    assert 'components' not in raw_out
    raw_tris = {m.group(1): int(m.group(2)) for m in re.finditer(r'^(\d{4}): \d+ vertices, (\d+) triangles$', raw_out, flags=re.M)}
    tris = {m.group(1): int(m.group(2)) for m in re.finditer(r'^(\d{4}): \d+ vertices, (\d+) triangles$', out, flags=re.M)}
    reports = {m.group(1): tuple(int(x) for x in m.groups()[1:]) for m in re.finditer(r'^(\d{4}): (\d+) components found, (\d+) kept, (\d+) triangles dropped$', out, flags=re.M)}
    assert set(raw_tris) == set(tris) == {'0000', '0001'} and sum(raw_tris.values()) > 0
    for name, n in raw_tris.items():
        if n == 0:
            assert tris[name] == 0 and name not in reports
            continue
        found, kept, dropped = reports[name]
        assert found >= 1 and kept == 1 and dropped == n - tris[name] and 0 < tris[name] <= n and (found == 1) == (dropped == 0)
        header = open(tmp_path / 'clean' / f'{name}.ply', 'rb').read(400).decode('latin1')
        assert f'element face {tris[name]}\n' in header
    rt = _tool('render_trajectory')
    base = ['--ckpt', str(tmp_path), '--seeds', '0,1', '--trajectory', 'front_circle', '--num-frames', '2', '--level', '0.0', '--volume-res', '24', '--seed', '5', '--vis', 'mesh_grid']
    rt.main(base + ['--out', str(tmp_path / 'raw.npy')])
    rt.main(base + ['--out', str(tmp_path / 'clean.npy'), '--keep-components', '1', '--component-by', 'area'])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2 and lines[0]['components'] is None and lines[1]['components'] == dict(keep=1, by='area', min_triangles=0)
    assert all(0 < c <= r for c, r in zip(lines[1]['triangles'], lines[0]['triangles']) if r) and lines[1]['shape'] == lines[0]['shape']

"""Shape extraction, the parts that need no GPU: the marching-cubes case table (tools/gen_mc_table.py -> csrc/mc_table.inc), the reference
crop, the .obj / .ply / .mrc writers and the command line of tools/extract_geometry.py."""
import importlib.util
import os
import struct

import numpy as np
import pytest

import mc_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def gen():
    return _tool('gen_mc_table')


def _face_segments_of_triangles(gen, tris, face):
    """Directed triangle sides lying on `face` = (axis, side)."""
    out = []
    for t in tris:
        for e0, e1 in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            if face in gen.edge_faces(e0) and face in gen.edge_faces(e1):
                out.append((e0, e1))
    return sorted(out)


def test_table_is_consistent_on_shared_faces(gen):
    """For every case and face the segments the triangles leave on the face depend only on the face's four corner signs, and the cell on the
    other side of the face -- whatever its case -- leaves the same segments there, run through in the opposite direction."""
    tab = gen.table()
    assert len(tab) == 256 and tab[0] == [] and tab[255] == [] and max(len(t) for t in tab) <= gen.MAX_TRIS
    by_signs = {}
    for case, tris in enumerate(tab):
        for face in gen.FACES:
            signs = tuple(sorted((k, (case >> k) & 1) for k in gen.face_corners(*face)))
            segs = _face_segments_of_triangles(gen, tris, face)
            assert by_signs.setdefault((face, signs), segs) == segs, (case, face)
            assert len(segs) in (0, 1, 2) and (len(segs) == 0) == (len({s for _, s in signs}) == 1), (case, face)
    assert len(by_signs) == 6 * 16

    def across(e, a):                     # the same edge seen from the neighbour cell on the other side of a face of axis a
        axis, off = gen.edge_info(e)
        off = list(off)
        off[a] ^= 1
        return next(k for k in range(12) if gen.edge_info(k) == (axis, tuple(off)))

    for a in range(3):
        for bits in range(16):
            hi = gen.face_corners(a, 1)
            signs_hi = tuple(sorted((k, (bits >> i) & 1) for i, k in enumerate(hi)))
            # the neighbour's face (a, 0) carries the same values on the corners with the same in-face coordinates
            signs_lo = tuple(sorted((k ^ (4 >> a), s) for k, s in signs_hi))
            mine = by_signs[((a, 1), signs_hi)]
            theirs = by_signs[((a, 0), signs_lo)]
            assert sorted((across(e1, a), across(e0, a)) for e0, e1 in mine) == theirs, (a, bits)
    gen.check_table(tab)


def test_table_file_is_the_generators_output(gen):
    assert open(gen.INC_PATH).read() == gen.render_inc()
    tdgp_build = importlib.import_module('3dgp_amd.build')
    assert 'mc_table.inc' in tdgp_build.HEADERS and 'geometry.hip' in tdgp_build.SOURCES


def test_table_marches_closed_surfaces(gen):
    """The numpy marcher the GPU tests compare against, on noise with a border below the threshold: a closed, consistently oriented surface with one
    vertex per sign-changing edge -- every one of the 256 cases occurs, ambiguous faces included."""
    vol = np.random.RandomState(3).rand(24, 23, 22).astype(np.float32)
    vol[[0, -1]] = vol[:, [0, -1]] = vol[:, :, [0, -1]] = -1.0
    tris = R.marcher(vol, 0.5, gen.table(), gen.edge_info)
    s = R.inside(vol, 0.5)
    c = sum(s[(k >> 2) & 1:vol.shape[0] - 1 + ((k >> 2) & 1), (k >> 1) & 1:vol.shape[1] - 1 + ((k >> 1) & 1), (k & 1):vol.shape[2] - 1 + (k & 1)].astype(int) << k
            for k in range(8))
    cases = set(np.unique(c).tolist())
    assert len(cases) == 256
    R.assert_closed_oriented(tris)
    assert np.array_equal(np.unique(tris), R.crossing_edge_ids(vol, 0.5))
    assert len(np.unique(tris)) == R.count_crossing_edges(vol, 0.5)
    ids = R.crossing_edge_ids(vol, 0.5)
    verts = R.edge_vertices(vol, 0.5, ids)
    assert R.signed_volume(verts, np.searchsorted(ids, tris)) > 0          # normals toward lower values: the inside blobs have positive volume


@pytest.mark.parametrize('res', [8, 21, 33, 256])
def test_crop_reference_is_pythons_own_slicing(tdgp, res):
    cube = np.arange(res ** 3, dtype=np.int32).reshape(res, res, res)
    want = cube[res // 8:-res // 8:, res // 2:, :-res // 3]
    sl = tdgp.geometry.crop_reference(res)
    assert len(sl) == 3 and all(isinstance(s, slice) for s in sl)
    got = cube[sl]
    assert got.shape == want.shape and np.array_equal(got, want)


def _parse_obj(path):
    v, f = [], []
    for line in open(path):
        p = line.split()
        if p and p[0] == 'v':
            v.append([np.float32(x) for x in p[1:4]])
        elif p and p[0] == 'f':
            f.append([int(x.split('/')[0]) - 1 for x in p[1:4]])
    return np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)


def parse_ply(path):
    """Binary little-endian PLY with float x y z vertices and `list uchar int` faces, read from the format description."""
    data = open(path, 'rb').read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    lines = data[:end].decode('ascii').splitlines()
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    elems, props = [], {}
    for ln in lines[2:]:
        p = ln.split()
        if p[0] == 'element':
            elems.append((p[1], int(p[2])))
            props[p[1]] = []
        elif p[0] == 'property':
            props[elems[-1][0]].append(tuple(p[1:]))
    assert [e for e, _ in elems] == ['vertex', 'face']
    assert props['vertex'] == [('float', 'x'), ('float', 'y'), ('float', 'z')] and props['face'] == [('list', 'uchar', 'int', 'vertex_indices')]
    nv, nf = elems[0][1], elems[1][1]
    v = np.frombuffer(data, '<f4', nv * 3, end).reshape(nv, 3)
    off = end + nv * 12
    f = np.empty([nf, 3], np.int32)
    for i in range(nf):
        assert data[off] == 3
        f[i] = struct.unpack_from('<3i', data, off + 1)
        off += 13
    assert off == len(data)
    return v.copy(), f


def test_writers_round_trip(tdgp, tmp_path):
    G = tdgp.geometry
    rs = np.random.RandomState(5)
    verts = np.concatenate([rs.randn(7, 3), [[0.0, -0.0, 1e-30], [1.0 / 3.0, 123456.789, -2.5e10]]]).astype(np.float32)
    tris = np.array([[0, 1, 2], [2, 1, 3], [8, 7, 6], [4, 5, 0]], np.int32)
    G.save_obj(tmp_path / 'm.obj', verts, tris)
    v, f = _parse_obj(tmp_path / 'm.obj')
    assert np.array_equal(v.view(np.uint32) & 0x7fffffff, verts.view(np.uint32) & 0x7fffffff) and np.array_equal(v, verts) and np.array_equal(f, tris)
    G.save_ply(tmp_path / 'm.ply', verts, tris)
    v, f = parse_ply(tmp_path / 'm.ply')
    assert np.array_equal(v.view(np.uint32), verts.view(np.uint32)) and np.array_equal(f, tris)
    # torch tensors are accepted as well, and an empty mesh writes a valid file
    import torch
    G.save_ply(tmp_path / 't.ply', torch.from_numpy(verts), torch.from_numpy(tris))
    assert open(tmp_path / 't.ply', 'rb').read() == open(tmp_path / 'm.ply', 'rb').read()
    G.save_ply(tmp_path / 'e.ply', np.zeros([0, 3], np.float32), np.zeros([0, 3], np.int32))
    v, f = parse_ply(tmp_path / 'e.ply')
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_mrc_header_and_data(tdgp, tmp_path):
    D, H, W = 3, 4, 5
    vol = np.random.RandomState(6).randn(D, H, W).astype(np.float32)
    tdgp.geometry.save_mrc(tmp_path / 'v.mrc', vol)
    data = open(tmp_path / 'v.mrc', 'rb').read()
    assert len(data) == 1024 + 4 * D * H * W
    i = lambda word, n=1: struct.unpack_from(f'<{n}i', data, 4 * (word - 1))         # noqa: E731   (1-based header words, as the format counts them)
    f = lambda word, n=1: struct.unpack_from(f'<{n}f', data, 4 * (word - 1))         # noqa: E731
    assert i(1, 3) == (W, H, D) and i(4) == (2,) and i(5, 3) == (0, 0, 0) and i(8, 3) == (W, H, D)
    assert f(11, 3) == (float(W), float(H), float(D)) and f(14, 3) == (90.0, 90.0, 90.0)
    assert i(17, 3) == (1, 2, 3)
    dmin, dmax, dmean = f(20, 3)
    assert dmin == vol.min() and dmax == vol.max() and abs(dmean - vol.mean(dtype=np.float64)) < 1e-6
    assert i(24) == (0,)                                  # nsymbt: no extended header
    assert data[208:212] == b'MAP ' and data[212:214] == b'\x44\x44'
    assert abs(f(55)[0] - vol.astype(np.float64).std()) < 1e-6
    assert i(56) == (0,) and i(28) == (20140,)
    back = np.frombuffer(data, '<f4', D * H * W, 1024).reshape(D, H, W)
    assert np.array_equal(back.view(np.uint32), vol.view(np.uint32))
    with pytest.raises(ValueError):
        tdgp.geometry.save_mrc(tmp_path / 'bad.mrc', vol[0])


# configs/scripts/extract_geometry.yaml of the reference: its keys and defaults (`ckpt` is a group of loader options there, a directory here;
# num_ply_points is unused by the reference script and has no counterpart)
YAML_DEFAULTS = dict(seeds=None, num_seeds=None, classes=None, cube_size=0.3, volume_res=256, voxel_origin=[0.0, 0.0, 0.0], output_dir='shapes',
                     thresh_value=25.0, truncation_psi=0.7, verbose=True, save_mrc=True, save_obj=False, save_ply=False)


def test_cli_options(capsys):
    cli = _tool('extract_geometry')
    d = vars(cli.build_parser().parse_args([]))
    for k, v in YAML_DEFAULTS.items():
        assert d[k] == v, k
    assert set(d) == set(YAML_DEFAULTS) | {'ckpt'} and d['ckpt'] is None
    for argv in ([], ['--seeds', '1,2', '--num-seeds', '3']):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2
    capsys.readouterr()
    a = cli.parse_args(['--seeds', '1,2,5-7', '--classes', '3', '--no-save-mrc', '--save-ply', '--voxel-origin', '0.1', '-0.2', '0.3'])
    assert a.seeds == [1, 2, 5, 6, 7] and a.classes == [3] and a.save_mrc is False and a.save_ply is True and a.voxel_origin == [0.1, -0.2, 0.3]
    assert cli.parse_args(['--num-seeds', '4']).num_seeds == 4
    assert cli.sample_names([1, 12], None) == ['0001', '0012'] and cli.sample_names([1, 12], [3, 40]) == ['c0003-s0001', 'c0003-s0012', 'c0040-s0001', 'c0040-s0012']


def test_geometry_entry_points_and_cpu_refusal(tdgp):
    import torch
    for name in ('tdgp_voxel_coords', 'tdgp_mcubes_workspace_bytes', 'tdgp_mcubes_count', 'tdgp_mcubes_emit'):
        assert name in tdgp._lib.EXPORTS
    lib = tdgp._lib.load()
    assert lib.tdgp_mcubes_workspace_bytes(4, 5, 6) > 6 * 120 and lib.tdgp_mcubes_workspace_bytes(1, 5, 6) == -1
    with pytest.raises(RuntimeError, match='GPU'):
        tdgp.geometry.marching_cubes(torch.zeros(3, 3, 3), 0.5)
    with pytest.raises(RuntimeError, match='GPU'):
        tdgp.geometry.create_voxel_coords(8, device='cpu')
    import inspect
    assert list(inspect.signature(tdgp.geometry.create_voxel_coords).parameters)[:4] == ['resolution', 'voxel_origin', 'cube_size', 'batch_size']

"""3dgp_amd/dataset.py on the CPU: ImageFolderDataset on a fixture the test writes itself (directory and zip), InfiniteSampler against
the indices recorded from the reference's sampler (tests/golden/infinite_sampler.npz, tools/gen_goldens.py:gen_infinite_sampler), and the
threaded batch iterator."""
import itertools
import json
import os
import zipfile

import numpy as np
import pytest

from conftest import load_golden

N, RES = 6, 16
LABELS = [2, 0, 1, 2, 1, 0]
DEPTH_KIND = {0: 16, 1: 16, 2: 8}                      # image index -> bit depth of its depth PNG (the others: 16 too, so that use_depth reads all)


def _names():
    return [f'{i // 3:02d}/img{i:03d}.png' for i in range(N)]


def _images():
    rs = np.random.RandomState(0)
    return rs.randint(0, 256, size=(N, RES, RES, 3)).astype(np.uint8)


def _depths():
    rs = np.random.RandomState(1)
    return [rs.randint(0, 256 if DEPTH_KIND.get(i, 16) == 8 else 65536, size=(RES, RES)).astype(np.uint8 if DEPTH_KIND.get(i, 16) == 8 else np.uint16) for i in range(N)]


def _angles():
    rs = np.random.RandomState(2)
    return rs.uniform(-1, 1, size=(N, 3)).astype(np.float32)


def write_fixture(root, name='toyset', extra_json=False):
    """-> (directory, zip path, embeddings path, descriptor path)"""
    import PIL.Image
    d = os.path.join(str(root), name)
    for fname, img, depth in zip(_names(), _images(), _depths()):
        os.makedirs(os.path.dirname(os.path.join(d, fname)), exist_ok=True)
        PIL.Image.fromarray(img).save(os.path.join(d, fname))
        PIL.Image.fromarray(depth).save(os.path.join(d, fname[:-4] + '_depth.png'))
    angles = _angles()
    meta = dict(labels=[[f, c] for f, c in zip(_names(), LABELS)], camera_angles=[[f, [float(v) for v in a]] for f, a in zip(_names(), angles)])
    with open(os.path.join(d, 'dataset.json'), 'w') as f:
        json.dump(meta, f)
    if extra_json:
        with open(os.path.join(d, '00', 'dataset.json'), 'w') as f:
            json.dump(meta, f)
    z = os.path.join(str(root), name + '.zip')
    with zipfile.ZipFile(z, 'w') as zf:
        for r, _, files in os.walk(d):
            for f in files:
                full = os.path.join(r, f)
                zf.write(full, os.path.relpath(full, d))
    emb = np.random.RandomState(3).randn(N, 4).astype(np.float32)
    order = [3, 0, 5, 1, 4, 2]                          # the memmap's rows are NOT in file order
    emb_path, desc_path = os.path.join(str(root), 'emb.memmap'), os.path.join(str(root), 'emb.json')
    mm = np.memmap(emb_path, dtype='float32', mode='w+', shape=(N, 4))
    for i, row in enumerate(order):
        mm[row] = emb[i]
    mm.flush()
    with open(desc_path, 'w') as f:
        json.dump(dict(shape=[N, 4], filepath_to_idx={n: order[i] for i, n in enumerate(_names())}), f)
    return d, z, emb_path, desc_path


@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    return write_fixture(tmp_path_factory.mktemp('data'))


@pytest.fixture(scope='module')
def DS(tdgp):
    return tdgp.dataset


def test_directory_and_zip_readers_agree(DS, fixture):
    d, z, emb, desc = fixture
    kw = dict(resolution=RES, use_depth=True, c_dim=3, use_embeddings=True, embeddings_path=emb, embeddings_desc_path=desc)
    a, b = DS.ImageFolderDataset(d, **kw), DS.ImageFolderDataset(z, **kw)
    assert len(a) == len(b) == N and a.image_shape == [3, RES, RES] and a.name == b.name == 'toyset' and a.label_dim == 3 and a.has_depth
    want_emb = np.random.RandomState(3).randn(N, 4).astype(np.float32)
    for i in range(N):
        x, y = a[i], b[i]
        assert sorted(x) == ['camera_angles', 'depth', 'embedding', 'image', 'label']
        for k in x:
            assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]), (i, k)
        assert x['image'].dtype == np.uint8 and np.array_equal(x['image'], _images()[i].transpose(2, 0, 1))
        assert x['label'].dtype == np.float32 and np.array_equal(x['label'], np.eye(3, dtype=np.float32)[LABELS[i]])          # one-hot
        assert x['camera_angles'].dtype == np.float32 and np.array_equal(x['camera_angles'], _angles()[i])
        assert x['embedding'].dtype == np.float32 and np.array_equal(x['embedding'], want_emb[i])
        assert x['depth'].dtype == np.int32 and x['depth'].shape == (1, RES, RES)
        scale = 256 if DEPTH_KIND.get(i, 16) == 8 else 1                                                                # 8-bit depth x 256
        assert np.array_equal(x['depth'][0], _depths()[i].astype(np.int32) * scale)
    assert _depths()[0].max() > 255                                                                                    # the 16-bit files really carry 16 bits
    b.close()


def test_depth_files_are_not_images_and_defaults(DS, fixture):
    d = fixture[0]
    ds = DS.ImageFolderDataset(d)
    assert ds.image_names == sorted(_names()) and not any(f.endswith('_depth.png') for f in ds.image_names)
    item = ds[0]
    assert item['label'].shape == (0,) and item['embedding'].shape == (0,) and np.array_equal(item['depth'], np.array([[0]], dtype=np.int32))
    with pytest.raises(IOError):
        DS.ImageFolderDataset(d, resolution=32)


def test_float_label_rows_pass_through(DS, tmp_path):
    import PIL.Image
    d = str(tmp_path / 'floats')
    os.makedirs(d)
    rows = [[0.25, 0.5], [1.0, -2.0]]
    for i in range(2):
        PIL.Image.fromarray(_images()[i]).save(os.path.join(d, f'{i}.png'))
    with open(os.path.join(d, 'dataset.json'), 'w') as f:
        json.dump(dict(labels=[[f'{i}.png', rows[i]] for i in range(2)]), f)
    ds = DS.ImageFolderDataset(d, c_dim=2)
    assert ds.label_shape == [2] and not ds.has_onehot_labels
    assert ds[1]['label'].dtype == np.float32 and np.array_equal(ds[1]['label'], np.array(rows[1], np.float32))
    assert np.array_equal(ds[1]['camera_angles'], np.zeros(3, np.float32))                       # no camera_angles field: zeros


@pytest.mark.parametrize('dist', ['truncnorm', 'custom'])
def test_mirror_doubles_flips_w_and_reflects_yaw_about_the_mean(DS, tdgp, fixture, dist):
    cam = dict(fov=dict(dist='uniform', min=10.0, max=30.0), origin=dict(radius=dict(dist='normal', mean=1.5, std=0.0),
               angles=dict(dist=dist, yaw=dict(min=-1.0, max=1.4, mean=0.0, std=0.4), pitch=dict(min=0.4, max=2.6, mean=1.5, std=0.2))))
    ds = DS.ImageFolderDataset(fixture[0], use_depth=True, mirror=True, c_dim=3, camera_cfg=cam)
    assert len(ds) == 2 * N
    mean = ds.mean_camera_params
    if dist == 'custom':                                                                        # dataset.py:230-238: the dataset's own mean
        assert np.allclose(mean[:3], _angles().mean(axis=0), atol=1e-6)
    else:
        assert np.allclose(mean[:3], [0.2, 1.5, 0.0])
    assert mean.shape == (5,) and np.allclose(mean[3:], [20.0, 1.5])
    for i in range(N):
        a, b = ds[i], ds[N + i]
        assert np.array_equal(b['image'], a['image'][:, :, ::-1]) and np.array_equal(b['depth'], a['depth'][:, :, ::-1])
        assert np.array_equal(a['label'], b['label'])
        want = a['camera_angles'].copy()
        want[0] = -(want[0] - mean[0]) + mean[0]
        assert np.array_equal(b['camera_angles'], want.astype(np.float32)) and np.array_equal(b['camera_angles'][1:], a['camera_angles'][1:])


def test_max_size_subset_is_sorted_and_seed_stable(DS, fixture):
    d = fixture[0]
    a = DS.ImageFolderDataset(d, max_size=4, random_seed=5)
    b = DS.ImageFolderDataset(d, max_size=4, random_seed=5)
    c = DS.ImageFolderDataset(d, max_size=4, random_seed=6)
    idx = np.arange(N)
    np.random.RandomState(5).shuffle(idx)
    assert len(a) == 4 and list(a.source_index) == sorted(idx[:4]) == list(b.source_index) and list(a.source_index) == sorted(a.source_index)
    assert list(c.source_index) != list(a.source_index)
    assert np.array_equal(a[1]['image'], _images()[a.source_index[1]].transpose(2, 0, 1))
    assert len(DS.ImageFolderDataset(d, max_size=4, mirror=True)) == 8 and len(DS.ImageFolderDataset(d, max_size=100)) == N


def test_two_dataset_json_files_raise(DS, tmp_path):
    d, z = write_fixture(tmp_path, name='twice', extra_json=True)[:2]
    for path in (d, z):
        with pytest.raises(ValueError, match='dataset.json'):
            DS.ImageFolderDataset(path)


def _png_filter_row(kind, cur, above, bpp):
    """One row of PNG filtering (the encoder's side), bytes as int arrays [w * bpp]."""
    left = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
    upleft = np.concatenate([np.zeros(bpp, np.int64), above[:-bpp]])
    if kind == 0:
        pred = 0
    elif kind == 1:
        pred = left
    elif kind == 2:
        pred = above
    elif kind == 3:
        pred = (left + above) // 2
    else:
        pa, pb, pc = np.abs(above - upleft), np.abs(left - upleft), np.abs(left + above - 2 * upleft)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, above, upleft))
    return (cur - pred) % 256


def write_png16(path, planes):
    """uint16 [h, w, channels] (1: grey, 2: grey + alpha) as a 16-bit PNG, the five row filters used in turn."""
    import struct
    import zlib
    h, w, ch = planes.shape
    rows = planes.astype('>u2').view(np.uint8).reshape(h, w * ch * 2).astype(np.int64)
    raw, above = bytearray(), np.zeros(w * ch * 2, np.int64)
    for y in range(h):
        raw.append(y % 5)
        raw += bytes(_png_filter_row(y % 5, rows[y], above, ch * 2).astype(np.uint8))
        above = rows[y]
    chunk = lambda tag, body: struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body))      # noqa: E731
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 16, 4 if ch == 2 else 0, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(bytes(raw))) + chunk(b'IEND', b''))


def test_sixteen_bit_two_channel_depth_keeps_sixteen_bits(DS, tmp_path):
    """The LeReS depth format: 16-bit grey + alpha.  PIL reduces it to 8 bit, the dataset decodes it itself -- every PNG row filter is in the
    file -- and a one-channel 16-bit file written the same way agrees with PIL's own decoding."""
    import PIL.Image
    rs = np.random.RandomState(4)
    d = str(tmp_path / 'la16')
    os.makedirs(d)
    depth = rs.randint(0, 65536, size=(2, RES, RES, 2)).astype(np.uint16)
    depth[0, :, :, 0] = (np.arange(RES * RES).reshape(RES, RES) * 251) % 65536           # smooth rows too: the filters see small residuals
    for i in range(2):
        PIL.Image.fromarray(_images()[i]).save(os.path.join(d, f'{i}.png'))
    write_png16(os.path.join(d, '0_depth.png'), depth[0])
    write_png16(os.path.join(d, '1_depth.png'), depth[1, :, :, :1])
    assert np.asarray(PIL.Image.open(os.path.join(d, '0_depth.png'))).dtype == np.uint8   # what PIL makes of it: 8 bits per channel
    assert np.array_equal(np.asarray(PIL.Image.open(os.path.join(d, '1_depth.png'))), depth[1, :, :, 0])   # the writer above is a valid encoder
    ds = DS.ImageFolderDataset(d, use_depth=True, mirror=True)
    for i in range(2):
        got = ds[i]['depth']
        assert got.dtype == np.int32 and got.shape == (1, RES, RES) and np.array_equal(got[0], depth[i, :, :, 0].astype(np.int32))
        assert np.array_equal(ds[2 + i]['depth'], got[:, :, ::-1])
    assert depth[0, :, :, 0].max() > 255
    with open(os.path.join(d, '0_depth.png'), 'rb') as f:
        assert np.array_equal(DS.decode_png16(f.read()), depth[0])


def test_infinite_sampler_against_the_recorded_indices(DS):
    g = load_golden('infinite_sampler')
    assert len(g['cases']) == 8
    seen = set()
    for k, (n, seed, rank, world, window) in enumerate(g['cases']):
        s = DS.InfiniteSampler(list(range(int(n))), rank=int(rank), num_replicas=int(world), shuffle=True, seed=int(seed), window_size=float(window))
        got = np.array(list(itertools.islice(iter(s), 64)), dtype=np.int64)
        assert np.array_equal(got, g[f'indices_{k}']), (k, got[:12], g[f'indices_{k}'][:12])
        seen.add((int(n), int(seed), int(rank), int(world), float(window)))
    assert seen == {(10, seed, rank, 2, window) for seed in (0, 3) for rank in (0, 1) for window in (0.5, 0.0)}
    plain = DS.InfiniteSampler(list(range(4)), shuffle=False)
    assert list(itertools.islice(iter(plain), 9)) == [0, 1, 2, 3, 0, 1, 2, 3, 0]


def test_batch_iterator_keeps_the_sampler_order_without_child_processes(DS, fixture):
    import multiprocessing
    import torch
    d, z = fixture[0], fixture[1]
    for path in (d, z):                                                                           # the zip handle is shared by the threads
        ds = DS.ImageFolderDataset(path, use_depth=True, c_dim=3)
        it = DS.batch_iterator(ds, DS.InfiniteSampler(ds, seed=1), batch_size=4, workers=3, pin_memory=False)
        order = list(itertools.islice(iter(DS.InfiniteSampler(ds, seed=1)), 12))
        for b in range(3):
            batch = next(it)
            assert batch['image'].dtype == torch.uint8 and batch['image'].shape == (4, 3, RES, RES)
            assert batch['depth'].dtype == torch.int32 and batch['depth'].shape == (4, 1, RES, RES) and batch['label'].shape == (4, 3)
            for j in range(4):
                assert np.array_equal(batch['image'][j].numpy(), ds[order[4 * b + j]]['image'])
        it.close()
        assert multiprocessing.active_children() == []

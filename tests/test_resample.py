"""Pillow-exact resampling on the host: the plain-loop restatement of the contract (tests/pillow_resample_reference.py) against
tests/golden/resample.npz and against live Pillow, `images.resize` (vectorised host path) against the restatement, the crop window, the shape
rules, `detector_input` against the torch CPU chain on the Pillow-resized image, and the three data tools on a temporary folder.  No GPU here;
the kernels are tests/test_resample_gpu.py."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import pillow_resample_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'tool_{name}', os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def M(tdgp):
    return tdgp.images


@pytest.fixture(scope='module')
def G(golden):
    return golden('resample')


@pytest.fixture(scope='module')
def pil_resize():
    pytest.importorskip('PIL')
    return _tool('gen_resample_goldens').pil_resize


def assert_golden(G, key, y):
    """`y` against the golden's Pillow bytes of case `key` (or their SHA-256 for the large outputs)."""
    if key in G:
        assert G[key].dtype == y.dtype and G[key].shape == y.shape and np.array_equal(G[key], y), f'{key}: {int((G[key] != y).sum())} values differ from Pillow'
    else:
        want = G['sha256:' + key].tobytes()
        assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).digest() == want, f'{key}: differs from Pillow (digest)'


# ----------------------------------------------------------------------------------------------------------------------
# the contract: restatement == golden == live Pillow == images.resize (host)
# ----------------------------------------------------------------------------------------------------------------------
def test_golden_holds_every_case(G):
    assert str(G['pillow_version'])
    keys = [R.case_key(8, *c) for c in R.CASES_U8] + [R.case_key(16, f, hw, out, 1, kind) for f, hw, out, kind in R.CASES_U16]
    assert len(keys) == 162 + 45
    for k in keys:
        assert (k in G) != ('sha256:' + k in G), k
    assert R.case_key(8, 'bicubic', (256, 256), (224, 224), 3, 'noise') in G             # the detector shape is kept in full


@pytest.mark.parametrize('hw,out', R.SIZES_U8, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('filter', R.FILTERS)
def test_u8_restatement_golden_and_host_path(M, G, filter, hw, out):
    for c in (1, 3):
        for kind in R.KINDS:
            x = R.make_input(8, hw, c, kind, key=filter)
            want = R.expected(8, filter, hw, out, c, kind)
            assert want.dtype == np.uint8 and want.shape == out + (c,)
            assert_golden(G, R.case_key(8, filter, hw, out, c, kind), want)
            got = M.resize(x, out, filter)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
            if out == hw:
                assert np.array_equal(want, x)                                             # neither size changes: a copy


@pytest.mark.parametrize('filter', R.FILTERS)
def test_u8_stripes_reach_both_clips(M, filter):
    """0 / 255 stripes through `images.resize`: over the sizes, the outputs hold both 0 and 255, and for the filters with negative lobes both
    were CLIPPED to (the restatement's pre-clip value lay outside [0, 255]); bilinear weights are non-negative and sum to one, so it cannot
    overshoot."""
    low = high = clipped_low = clipped_high = False
    for hw, out in R.SIZES_U8:
        x = R.make_input(8, hw, 3, 'stripes', key=filter)
        y = M.resize(x, out, filter)
        ref, pres = R.resize_u8(x, out, filter, with_preclip=True)
        assert np.array_equal(y, ref)
        low, high = low or bool((y == 0).any()), high or bool((y == 255).any())
        if pres:
            clipped_low, clipped_high = clipped_low or bool((pres[-1] < 0).any()), clipped_high or bool((pres[-1] > 255).any())
    assert low and high
    assert (clipped_low and clipped_high) == (filter != 'bilinear')


@pytest.mark.parametrize('hw,out', R.SIZES_U16, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('filter', R.FILTERS)
def test_u16_restatement_golden_and_host_path(M, G, filter, hw, out):
    for kind in R.KINDS:
        x = R.make_input(16, hw, 1, kind, key=filter)
        want = R.expected(16, filter, hw, out, 1, kind)
        assert want.dtype == np.uint16 and want.shape == out
        assert_golden(G, R.case_key(16, filter, hw, out, 1, kind), want)
        got = M.resize(x, out, filter)
        assert got.dtype == np.uint16 and np.array_equal(got, want)
        wide = M.resize(torch.from_numpy(x.astype(np.int32)), out, filter)                # int32 on the 16-bit scale, a CPU tensor
        assert isinstance(wide, torch.Tensor) and wide.dtype == torch.int32 and np.array_equal(wide.numpy(), want.astype(np.int32))


@pytest.mark.parametrize('filter', R.FILTERS)
def test_host_path_is_live_pillow(M, pil_resize, filter):
    """The one comparison that needs Pillow installed: `images.resize` (and with it the restatement, pinned to it above) against
    `PIL.Image.resize` on every shared case."""
    for hw, out in R.SIZES_U8:
        for c in (1, 3):
            for kind in R.KINDS:
                x = R.make_input(8, hw, c, kind, key=filter)
                live, got = pil_resize(x, out, filter), M.resize(x, out, filter)
                assert np.array_equal(live, got), f'{hw}->{out} c{c} {kind}: {int((live != got).sum())} bytes differ from live Pillow'
    for hw, out in R.SIZES_U16:
        for kind in R.KINDS:
            x = R.make_input(16, hw, 1, kind, key=filter)
            live, got = pil_resize(x, out, filter), M.resize(x, out, filter)
            assert np.array_equal(live, got), f'{hw}->{out} {kind}: {int((live != got).sum())} pixels differ from live Pillow'
    for bits, f, hw, c, box, out in _tool('gen_resample_goldens').BOX_CASES:      # .crop(box).resize(...)
        if f == filter:
            x = R.make_input(bits, hw, c, 'noise', key='box')
            assert np.array_equal(pil_resize(x, out, f, box=box), M.resize(x, out, f, box=box))


def test_u16_ramp_tells_the_lanczos_forms_apart(M, G, monkeypatch):
    """The window written as sin(a / 3) / (a / 3) with a = x pi is the same function as Pillow's sinc(x) sinc(x / 3), but not the same
    doubles: on the (311 i + 173 j) mod 65536 ramp at 64^2 -> 24^2 values sit on exact ties and a few pixels move by one unit.  The product
    uses Pillow's form: it matches the golden where the other form does not."""
    import math
    x = R.make_input(16, (64, 64), 1, 'ramp', key='lanczos')
    assert int(x[3, 5]) == (311 * 3 + 173 * 5) % 65536
    golden = G[R.case_key(16, 'lanczos', (64, 64), (24, 24), 1, 'ramp')]
    assert np.array_equal(M.resize(x, 24, 'lanczos'), golden)

    def other_form(filter, t):
        if not -3.0 <= t < 3.0:
            return 0.0
        if t == 0.0:
            return 1.0
        a = t * math.pi
        return (math.sin(a) / a) * (math.sin(a / 3) / (a / 3))

    monkeypatch.setattr(R, '_weight', other_form)
    R.rows.cache_clear()
    try:
        other = R.resize_u16(x, (24, 24), 'lanczos')
    finally:
        R.rows.cache_clear()                                  # later tests rebuild their rows with Pillow's form
    moved = other.astype(np.int64) - golden.astype(np.int64)
    print(f'{int((moved != 0).sum())} pixels move, by at most {int(np.abs(moved).max())}')
    assert 1 <= int((moved != 0).sum()) <= 24 and int(np.abs(moved).max()) == 1


@pytest.mark.parametrize('filter', ('lanczos', 'bicubic'))
def test_u16_overflow_bytes_and_saturate(M, filter):
    """Stripes overshoot both ends.  Pillow's store of a value above 65535 is 0xFF00 | (v & 255): high byte 255, low byte below 255 somewhere.
    'saturate' differs from 'pillow' exactly on the pixels whose pre-clip value exceeds 65535, and is 65535 there."""
    odd = under = 0
    for hw, out in R.SIZES_U16:
        x = R.make_input(16, hw, 1, 'stripes', key=filter)
        pil, pre = R.resize_u16(x, out, filter, with_preclip=True)
        assert np.array_equal(pil, R.expected(16, filter, hw, out, 1, 'stripes'))
        over = pre > 65535
        odd += int((((pil >> 8) == 255) & ((pil & 255) < 255) & over).sum())
        under += int((pre < 0).sum())
        assert (pil[pre < 0] == 0).all()
        for sat in (R.resize_u16(x, out, filter, overflow='saturate'), M.resize(x, out, filter, overflow='saturate')):
            assert (sat[over] == 65535).all() and np.array_equal(sat[~over], pil[~over])
            assert np.array_equal(sat != pil, over & (pil != 65535))
        assert np.array_equal(M.resize(x, out, filter, overflow='pillow'), pil)
    print(f'{filter}: {odd} stripe pixels with high byte 255 and low byte < 255')
    assert odd >= 1 and under >= 1


def test_crop_window_is_crop_then_resize(M, G):
    box_cases = _tool('gen_resample_goldens').BOX_CASES
    for bits, filter, hw, c, box, out in box_cases:
        assert box[0] % 2 == 1 and box[1] % 2 == 1                                          # odd offsets
        x = R.make_input(bits, hw, c, 'noise', key='box')
        want = (R.resize_u8 if bits == 8 else R.resize_u16)(x, out, filter, box=box)
        assert np.array_equal(G[f'box/u{bits}'], want)
        assert np.array_equal(M.resize(x, out, filter, box=box), want)
        x0, y0, w, h = box
        assert np.array_equal(M.resize(np.ascontiguousarray(x[y0:y0 + h, x0:x0 + w]), out, filter), want)
    with pytest.raises(ValueError, match='box'):
        M.resize(R.make_input(8, (20, 20), 3, 'noise'), 8, box=(15, 0, 8, 8))


def test_tables(M):
    bounds, coeffs = M.resample_tables(512, 24, 'lanczos')
    assert bounds.dtype == np.int32 and bounds.shape == (24, 2) and coeffs.dtype == np.int32 and coeffs.shape == (24, 129)
    assert (bounds[:, 0] >= 0).all() and (bounds.sum(axis=1) <= 512).all() and (bounds[:, 1] <= 129).all()
    b16, c16 = M.resample_tables(64, 24, 'bicubic', bits=16)
    assert c16.dtype == np.float64 and c16.shape == (24, R.rows(64, 24, 'bicubic')[1]) and np.allclose(c16.sum(axis=1), 1.0, atol=1e-12)
    table, _ = R.rows(64, 24, 'bicubic')
    for i, (xmin, w) in enumerate(table):
        assert (int(b16[i, 0]), int(b16[i, 1])) == (xmin, len(w)) and c16[i, :len(w)].tolist() == list(w) and not c16[i, len(w):].any()
    assert M.resample_tables(512, 24, 'lanczos')[1] is coeffs                                # cached
    with pytest.raises(ValueError):
        M.resample_tables(10, 5, 'nearest')
    with pytest.raises(ValueError, match='32768'):
        M.resample_tables(32769, 5, 'lanczos')


def test_shape_rules(M):
    # (h - ch) odd: half the margin ends in .5 and Python rounds half to even
    assert M.center_crop_box(7, 10, 4, 4) == (2, 3)            # 1.5 -> 2, 3.0 -> 3
    assert M.center_crop_box(9, 9, 4, 4) == (2, 2)             # 2.5 -> 2
    assert M.center_crop_box(256, 341, 224, 224) == (16, 58)   # 58.5 -> 58
    assert M.center_crop_box(11, 8, 4, 8) == (4, 0)            # 3.5 -> 4
    assert M.center_crop_box(5, 5, 5, 5) == (0, 0)
    with pytest.raises(ValueError):
        M.center_crop_box(4, 4, 5, 4)
    assert M.resized_shape(375, 500, 256) == (256, 341)        # int(256 * 500 / 375) = int(341.33)
    assert M.resized_shape(500, 375, 256) == (341, 256)
    assert M.resized_shape(256, 256, 256) == (256, 256)
    assert M.resized_shape(40, 56, 32) == (32, 44)             # int(44.8)
    assert M.resized_shape(333, 500, 256) == (256, 384)        # int(384.38)


def test_center_resize_crop(M, pil_resize):
    x = R.make_input(8, (37, 53), 3, 'noise', key='crc')
    got = M.center_resize_crop(x, 16)
    assert np.array_equal(got, pil_resize(x, (16, 16), 'lanczos', box=(8, 0, 37, 37)))      # left = round(16 / 2) = 8
    same = R.make_input(8, (16, 16), 3, 'noise')
    assert M.center_resize_crop(same, 16) is same
    d = R.make_input(16, (30, 21), 1, 'noise', key='crc')
    assert np.array_equal(M.center_resize_crop(d[None], 10)[0], pil_resize(d, (10, 10), 'lanczos', box=(0, 4, 21, 21)))   # top = round(4.5) = 4


@pytest.mark.parametrize('hw,resize,crop', [((40, 56), 32, 24), ((256, 256), 256, 224)])
def test_detector_input_is_the_torch_chain_on_the_pillow_image(M, pil_resize, hw, resize, crop):
    x = np.stack([R.make_input(8, hw, 3, 'noise', key=f'det{i}') for i in range(2)])
    kw = dict(resize=resize, crop=crop) if resize != 256 else {}
    got = M.detector_input(x, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (2, 3, crop, crop)
    oh, ow = M.resized_shape(hw[0], hw[1], resize)
    top, left = M.center_crop_box(oh, ow, crop, crop)
    mean, std = torch.tensor(M.DETECTOR_MEAN).view(3, 1, 1), torch.tensor(M.DETECTOR_STD).view(3, 1, 1)
    for i in range(2):
        r = pil_resize(x[i], (oh, ow), 'bicubic')[top:top + crop, left:left + crop]
        want = torch.from_numpy(np.ascontiguousarray(r.transpose(2, 0, 1))).float().div(255).sub(mean).div(std).numpy()
        assert got[i].tobytes() == want.tobytes()
        assert R.detector_input(x[i], resize, crop, 'bicubic', M.DETECTOR_MEAN, M.DETECTOR_STD).tobytes() == want.tobytes()
    as_tensor = M.detector_input(torch.from_numpy(x), **kw)
    assert isinstance(as_tensor, torch.Tensor) and as_tensor.numpy().tobytes() == got.tobytes()


def test_resize_refuses_what_it_does_not_take(M):
    x = R.make_input(8, (9, 9), 3, 'noise')
    with pytest.raises(TypeError):
        M.resize(x.astype(np.float32), 4)
    with pytest.raises(ValueError, match='channels'):
        M.resize(np.zeros((9, 9, 2), np.uint8), 4)
    with pytest.raises(ValueError, match='overflow'):
        M.resize(x, 4, overflow='wrap')
    with pytest.raises(ValueError, match='32768'):
        M.resize(x, 32769)
    with pytest.raises(ValueError, match='16-bit scale'):
        M.resize(np.full((9, 9), 70000, np.int32), 4)
    assert M.resize(x, (4, 6)).shape == (4, 6, 3) and M.resize(x[None], 5, 'bilinear').shape == (1, 5, 5, 3)


# ----------------------------------------------------------------------------------------------------------------------
# the tools on a temporary folder
# ----------------------------------------------------------------------------------------------------------------------
def _write_folder(root):
    """RGB JPEG and PNG, one L, one RGBA, one 16-bit depth PNG, one text file, a sub-directory."""
    import PIL.Image
    os.makedirs(os.path.join(root, 'sub'))
    img = lambda hw, c, key: R.make_input(8, hw, c, 'noise', key=key)      # noqa: E731
    PIL.Image.fromarray(img((40, 56), 3, 'a')).save(os.path.join(root, 'a.jpg'), quality=95)
    PIL.Image.fromarray(img((37, 53), 3, 'b')).save(os.path.join(root, 'b.png'))
    PIL.Image.fromarray(img((40, 56), 3, 'c')).save(os.path.join(root, 'sub', 'c.jpg'), quality=95)
    PIL.Image.fromarray(img((40, 56), 3, 'c2')).save(os.path.join(root, 'sub', 'c2.png'))
    PIL.Image.fromarray(img((30, 44), 1, 'd')[:, :, 0]).save(os.path.join(root, 'sub', 'd.png'))
    rgba = np.concatenate([img((33, 45), 3, 'e'), img((33, 45), 1, 'ea')], axis=2)
    PIL.Image.fromarray(rgba, 'RGBA').save(os.path.join(root, 'e.png'))
    PIL.Image.fromarray(R.make_input(16, (36, 50), 1, 'noise', key='f')).save(os.path.join(root, 'f.png'))
    with open(os.path.join(root, 'notes.txt'), 'w') as f:
        f.write('not an image\n')
    return ['a.jpg', 'b.png', 'e.png', 'f.png', 'sub/c.jpg', 'sub/c2.png', 'sub/d.png']


def test_write_image_flattens_four_bands_for_jpeg(tdgp, tmp_path):
    import PIL.Image
    T = tdgp.data_tools
    rgba = np.zeros((8, 8, 4), np.uint8)
    rgba[:, :4] = (200, 30, 30, 255)                           # opaque red on the left, fully transparent black on the right
    T.write_image(PIL.Image.fromarray(rgba, 'RGBA'), str(tmp_path / 'a.png'))
    assert PIL.Image.open(str(tmp_path / 'a.png')).mode == 'RGBA'
    T.write_image(PIL.Image.fromarray(rgba, 'RGBA'), str(tmp_path / 'a.jpg'))
    a = PIL.Image.open(str(tmp_path / 'a.jpg'))
    px = np.asarray(a).astype(int)
    assert a.mode == 'RGB' and px[4, 7].min() >= 250 and abs(px[4, 0] - (200, 30, 30)).max() <= 12      # white where it was transparent
    cmyk = PIL.Image.new('CMYK', (8, 8), (0, 255, 255, 0))
    T.write_image(cmyk, str(tmp_path / 'c.png'))
    assert PIL.Image.open(str(tmp_path / 'c.png')).mode == 'RGB'
    # quality 95 goes to .jpg alone
    noise = PIL.Image.fromarray(R.make_input(8, (32, 32), 3, 'noise', key='q'))
    T.write_image(noise, str(tmp_path / 'q.jpg'))
    noise.save(str(tmp_path / 'q95.jpg'), quality=95)
    T.write_image(noise, str(tmp_path / 'q.jpeg'))
    noise.save(str(tmp_path / 'qdef.jpeg'))
    assert open(str(tmp_path / 'q.jpg'), 'rb').read() == open(str(tmp_path / 'q95.jpg'), 'rb').read()
    assert open(str(tmp_path / 'q.jpeg'), 'rb').read() == open(str(tmp_path / 'qdef.jpeg'), 'rb').read()


def _pillow_route(src, trg, size, T):
    """The reference's route with Pillow alone, saved the same way."""
    import PIL.Image
    img = PIL.Image.open(src)
    img.load()
    T.write_image(T._pillow_center_resize_crop(img, size), trg)


def test_resize_dataset_on_the_host(tdgp, tmp_path, capsys):
    import PIL.Image
    T = tdgp.data_tools
    src = str(tmp_path / 'raw')
    names = _write_folder(src)
    res = T.resize_dataset(src, size=16, device=None)
    out = src + '_16'
    assert res['target_dir'] == out and res['num_images'] == 7 and res['resized'] == 6 and res['host_fallback'] == 1 and res['copied'] == 1
    assert res['skipped'] == 0 and res['device'] == 'cpu' and set(res['seconds']) == {'decode', 'resample', 'encode', 'copy', 'total'}
    assert open(os.path.join(out, 'notes.txt')).read() == 'not an image\n'
    modes = {}
    for n in names:
        want_path = str(tmp_path / ('want' + os.path.splitext(n)[1]))
        _pillow_route(os.path.join(src, n), want_path, 16, T)
        got, want = PIL.Image.open(os.path.join(out, n)), PIL.Image.open(want_path)
        assert got.mode == want.mode and got.size == want.size == (16, 16), n
        assert np.array_equal(np.asarray(got), np.asarray(want)), n
        modes[n] = got.mode
    assert modes['f.png'] == 'I;16' and modes['sub/d.png'] == 'L' and modes['e.png'] == 'RGBA'
    # the options: another format (the RGBA image is pasted onto white), images only, numbering, existing files kept
    out2 = str(tmp_path / 'as_jpg')
    res2 = T.resize_dataset(src, target_dir=out2, size=12, format='.jpg', images_only=True, ignore_regex='f\\.png', fname_prefix='p_', device=None)
    assert res2['num_images'] == 6 and res2['copied'] == 0 and not os.path.exists(os.path.join(out2, 'notes.txt'))
    e = PIL.Image.open(os.path.join(out2, 'p_e.jpg'))
    assert e.mode == 'RGB' and e.size == (12, 12) and os.path.exists(os.path.join(out2, 'p_sub', 'd.jpg'))      # the prefix goes in front of the relative name
    want_path = str(tmp_path / 'want_e.jpg')
    _pillow_route(os.path.join(src, 'e.png'), want_path, 12, T)
    assert np.array_equal(np.asarray(e), np.asarray(PIL.Image.open(want_path)))
    res3 = T.resize_dataset(src, target_dir=out2, size=12, format='.jpg', images_only=True, ignore_regex='f\\.png', fname_prefix='p_', ignore_existing=True,
                            ignore_grayscale=True, device=None)
    assert res3['skipped'] == 6 and res3['resized'] == 0
    # the command line prints the same dict as one JSON line
    _tool('resize_dataset').main(['-d', src, '-t', str(tmp_path / 'cli'), '-s', '8', '--rename_enum', '--device', 'cpu'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['resized'] == 6 and line['host_fallback'] == 1 and sorted(os.listdir(str(tmp_path / 'cli')))[0] == '00000000.jpg'
    with pytest.raises(ValueError, match='GPU'):
        T.resize_dataset(src, size=16, device='cpu')


def test_merge_depth_data_writes_the_dataset_layout(tdgp, tmp_path, capsys):
    import PIL.Image
    T = tdgp.data_tools
    imgs, depths, out = str(tmp_path / 'imgs'), str(tmp_path / 'depths'), str(tmp_path / 'merged')
    os.makedirs(os.path.join(imgs, 'n01'))
    os.makedirs(os.path.join(depths, 'n01'))
    d = {}
    for name in ('x', 'n01/y', 'z'):
        PIL.Image.fromarray(R.make_input(8, (16, 16), 3, 'noise', key=name)).save(os.path.join(imgs, name + '.jpg'), quality=95)
    for name in ('x', 'n01/y', 'w'):
        d[name] = R.make_input(16, (16, 16), 1, 'noise', key='d' + name)
        PIL.Image.fromarray(d[name]).save(os.path.join(depths, name + '.png'))
    merged = T.merge_depth_data(imgs, depths, out)
    assert merged == [os.path.join('n01', 'y.jpg'), 'x.jpg']
    assert sorted(os.listdir(out)) == ['n01', 'x.jpg', 'x_depth.png'] and sorted(os.listdir(os.path.join(out, 'n01'))) == ['y.jpg', 'y_depth.png']
    ds = tdgp.dataset.ImageFolderDataset(out, resolution=16, use_depth=True)
    assert len(ds) == 2 and ds.image_names == ['n01/y.jpg', 'x.jpg']
    assert np.array_equal(ds[0]['depth'][0], d['n01/y'].astype(np.int32)) and np.array_equal(ds[1]['depth'][0], d['x'].astype(np.int32))
    assert np.array_equal(ds[1]['image'], np.asarray(PIL.Image.open(os.path.join(imgs, 'x.jpg'))).transpose(2, 0, 1))
    ds.close()
    _tool('merge_depth_data').main(['-i', imgs, '-d', depths, '-t', str(tmp_path / 'cli')])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])['num_merged'] == 2


class IntegerProjection(torch.nn.Module):
    """A stand-in detector whose rows are exact: x * 64 rounded to integers, 8 fixed positions summed per feature (integer sums below 2^24 are
    exact in fp32 in any order, on any device)."""

    def __init__(self, crop, features=6, seed=5):
        super().__init__()
        self.register_buffer('index', torch.from_numpy(np.random.RandomState(seed).randint(0, 3 * crop * crop, size=features * 8)))

    def forward(self, x):
        q = torch.round(x * 64.0).flatten(1)
        return q[:, self.index].reshape(x.shape[0], -1, 8).sum(dim=2)


def write_feature_folder(root):
    """Square RGB images of two sizes (so that a window splits into two batches), one depth map that must be left out."""
    import PIL.Image
    os.makedirs(os.path.join(root, 'sub'))
    names = []
    for i, (name, side) in enumerate([('a.png', 40), ('b.jpg', 48), ('c.png', 40), ('sub/d.png', 40), ('sub/e.jpg', 48), ('sub/f.png', 40), ('g.png', 40)]):
        PIL.Image.fromarray(R.make_input(8, (side, side), 3, 'noise', key=name)).save(os.path.join(root, name), **({'quality': 95} if name.endswith('.jpg') else {}))
        names.append(name)
    PIL.Image.fromarray(R.make_input(16, (40, 40), 1, 'noise', key='depth')).save(os.path.join(root, 'a_depth.png'))
    return sorted(names)


def test_extract_features_feeds_the_dataset_and_instance_selection(tdgp, tmp_path, capsys):
    import PIL.Image
    T, M = tdgp.data_tools, tdgp.images
    root = str(tmp_path / 'data')
    names = write_feature_folder(root)
    det = IntegerProjection(24).eval()
    out, npy = str(tmp_path / 'feats' / 'f.memmap'), str(tmp_path / 'f.npy')
    res = T.extract_features(root, det, out, batch_size=4, device=None, npy_path=npy, resize=32, crop=24)
    assert res['num_images'] == 7 and res['num_features'] == 6 and res['desc_path'] == out.replace('.memmap', '_desc.json')
    assert T.feature_image_paths(root) == names
    desc = json.load(open(res['desc_path']))
    assert desc['shape'] == [7, 6] and desc['filepath_to_idx'] == {n: i for i, n in enumerate(names)}
    rows = np.load(npy)
    assert rows.dtype == np.float32 and rows.shape == (7, 6)
    want = np.stack([det(M.detector_input(torch.from_numpy(np.array(PIL.Image.open(os.path.join(root, n)).convert('RGB'))[None]), resize=32, crop=24))[0].numpy()
                     for n in names])
    assert np.array_equal(rows, want) and np.abs(rows).max() > 0 and np.array_equal(rows, np.round(rows))
    assert np.array_equal(np.memmap(out, dtype='float32', mode='r', shape=(7, 6)), rows)
    ds = tdgp.dataset.ImageFolderDataset(root, use_embeddings=True, embeddings_path=out, embeddings_desc_path=res['desc_path'])
    assert ds.image_names == names
    for i in range(len(ds)):
        assert np.array_equal(ds.get_embedding(i), want[i])
    ds.close()
    # the .npy rows are in the order run_instance_selection discovers the images of a folder without depth maps
    S = tdgp.instance_selection
    plain = str(tmp_path / 'plain')
    import shutil
    shutil.copytree(root, plain, ignore=shutil.ignore_patterns('*_depth.png'))
    assert S.find_images_in_dir(plain) == names
    kept = S.run_instance_selection(plain, str(tmp_path / 'kept'), num_imgs_to_keep=3, reg_covar=1e-3, embeddings=rows, verbose=False, device=None)
    scores = S.compute_gaussian_ll_scores(want, reg_covar=1e-3, device=None)
    assert kept == [names[i] for i in S.select_instances(scores, 3)]
    # the command line: a TorchScript detector file
    pt = str(tmp_path / 'det.pt')
    torch.jit.script(det).save(pt)
    _tool('extract_features').main(['--dataset', root, '--detector', pt, '--out', str(tmp_path / 'cli.memmap'), '--resize', '32', '--crop', '24', '--device', 'cpu',
                                    '--batch_size', '3'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['num_images'] == 7 and np.array_equal(np.memmap(str(tmp_path / 'cli.memmap'), dtype='float32', mode='r', shape=(7, 6)), rows)
    with pytest.raises(ValueError, match='memmap'):
        T.extract_features(root, det, str(tmp_path / 'f.bin'), device=None)

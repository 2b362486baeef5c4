"""Pillow-exact resampling on the GPU: tdgp_resample_u8 / _u16 / _u8_to_f32 (csrc/resample.hip) against the plain-loop restatement of the
contract (tests/pillow_resample_reference.py) and against Pillow's own bytes in tests/golden/resample.npz, byte for byte.  No comparison
here needs Pillow; the last test runs the data tools, which decode and encode with it wherever they run.

Tile edges (csrc/resample.hip): a block is RS_BLOCK = 256 consecutive samples of one row, the horizontal pass gives a lane RS_ROWS = 4 rows.
  (130, 257) -> (64, 86): both passes; 86 * 3 = 258 samples per row = one block + 2; 130 rows = 32 groups of 4 + 2;
  (31, 1025) -> (31, 300): horizontal pass only; 900 samples per row = 3 blocks + 132; 31 rows = 7 groups of 4 + 3;
  (31, 1025) -> (31, 257): with C = 1, 257 samples = one block + 1.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

import pillow_resample_reference as R

pytestmark = pytest.mark.gpu

EDGE_SIZES = (((130, 257), (64, 86)), ((31, 1025), (31, 300)), ((31, 1025), (31, 257)))


@pytest.fixture(scope='module')
def M(tdgp):
    return tdgp.images


@pytest.fixture(scope='module')
def G(golden):
    return golden('resample')


def dev16(a):
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)


def host16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def assert_golden(G, key, y):
    if key in G:
        assert np.array_equal(G[key], y), f'{key}: {int((G[key] != y).sum())} values differ from Pillow'
    else:
        assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).digest() == G['sha256:' + key].tobytes(), f'{key}: differs from Pillow (digest)'


@pytest.mark.parametrize('hw,out', R.SIZES_U8 + EDGE_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('filter', R.FILTERS)
def test_u8_device_is_the_restatement_and_pillow(M, G, filter, hw, out):
    for c in (1, 3):
        xs = [R.make_input(8, hw, c, kind, key=filter) for kind in R.KINDS]
        wants = [R.expected(8, filter, hw, out, c, kind) for kind in R.KINDS]
        batch = M.resize(torch.from_numpy(np.stack(xs)).cuda(), out, filter)                 # B = 3
        assert batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (3,) + out + (c,)
        batch = batch.cpu().numpy()
        for kind, x, want, got3 in zip(R.KINDS, xs, wants, batch):
            got1 = M.resize(torch.from_numpy(x).cuda(), out, filter).cpu().numpy()           # B = 1, given without the batch axis
            assert got1.shape == want.shape
            assert np.array_equal(got1, want), f'{kind} c{c}: {int((got1 != want).sum())} bytes differ'
            assert np.array_equal(got3, want), f'{kind} c{c} in a batch: {int((got3 != want).sum())} bytes differ'
            if (hw, out) in R.SIZES_U8:
                assert_golden(G, R.case_key(8, filter, hw, out, c, kind), got1)


@pytest.mark.parametrize('hw,out', R.SIZES_U16 + EDGE_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('filter', R.FILTERS)
def test_u16_device_is_the_restatement_and_pillow(M, G, filter, hw, out):
    xs = [R.make_input(16, hw, 1, kind, key=filter) for kind in R.KINDS]
    wants = [R.expected(16, filter, hw, out, 1, kind) for kind in R.KINDS]
    batch = M.resize(dev16(np.stack(xs)), out, filter)
    assert batch.dtype == torch.uint16 and tuple(batch.shape) == (3,) + out
    batch = host16(batch)
    for kind, x, want, got3 in zip(R.KINDS, xs, wants, batch):
        got1 = host16(M.resize(dev16(x), out, filter))
        assert np.array_equal(got1, want), f'{kind}: {int((got1 != want).sum())} pixels differ'
        assert np.array_equal(got3, want), f'{kind} in a batch: {int((got3 != want).sum())} pixels differ'
        if (hw, out) in R.SIZES_U16:
            assert_golden(G, R.case_key(16, filter, hw, out, 1, kind), got1)
        wide = M.resize(torch.from_numpy(x.astype(np.int32)).cuda(), out, filter)            # int32 on the 16-bit scale
        assert wide.dtype == torch.int32 and np.array_equal(wide.cpu().numpy(), want.astype(np.int32))
    sat = host16(M.resize(dev16(xs[2]), out, filter, overflow='saturate'))
    assert np.array_equal(sat, R.resize_u16(xs[2], out, filter, overflow='saturate'))


def test_long_tap_loop(M):
    """(512, 512) -> (24, 24): Lanczos ksize 129 -- the tap loop has no built-in maximum."""
    assert M.resample_tables(512, 24, 'lanczos')[1].shape[1] == 129
    x = R.make_input(8, (512, 512), 3, 'noise', key='long')
    assert np.array_equal(M.resize(torch.from_numpy(x).cuda(), 24).cpu().numpy(), R.resize_u8(x, (24, 24), 'lanczos'))
    d = R.make_input(16, (512, 512), 1, 'stripes', key='long')
    assert np.array_equal(host16(M.resize(dev16(d), 24)), R.resize_u16(d, (24, 24), 'lanczos'))


def test_crop_window_and_offsets_past_32_bits(M, G):
    for bits, filter, hw, c, box, out in (((8, 'lanczos', (41, 57), 3, (5, 3, 31, 29), (16, 20))), (16, 'bicubic', (41, 57), 1, (7, 9, 33, 21), (12, 40))):
        x = R.make_input(bits, hw, c, 'noise', key='box')
        got = M.resize(torch.from_numpy(x).cuda() if bits == 8 else dev16(x), out, filter, box=box)
        got = got.cpu().numpy() if bits == 8 else host16(got)
        assert np.array_equal(got, G[f'box/u{bits}'])
    # a window at the far corner of a batch of six 16384^2 RGB images: the last item's window starts 4.8e9 bytes into the buffer.  Only the
    # windows are written and read, so the 4.8 GB cost no time; the restatement sees the windows alone.
    B, S, win = 6, 16384, 40
    big = torch.empty([B, S, S, 3], dtype=torch.uint8, device='cuda')
    wins = np.stack([R.make_input(8, (win, win), 3, 'noise', key=f'far{b}') for b in range(B)])
    big[:, S - win:, S - win:, :] = torch.from_numpy(wins).cuda()
    got = M.resize(big, 16, 'lanczos', box=(S - win, S - win, win, win)).cpu().numpy()
    del big
    for b in (0, 2, 5):
        assert np.array_equal(got[b], R.resize_u8(wins[b], (16, 16), 'lanczos')), b


@pytest.mark.parametrize('hw,resize,crop', [((40, 56), 32, 24), ((256, 256), 256, 224)])
def test_detector_input_is_the_host_chain(M, hw, resize, crop):
    x = np.stack([R.make_input(8, hw, 3, 'noise', key=f'det{i}') for i in range(2)])
    kw = dict(resize=resize, crop=crop) if resize != 256 else {}
    want = M.detector_input(x, **kw)
    got = M.detector_input(torch.from_numpy(x).cuda(), **kw)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2, 3, crop, crop)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert R.detector_input(x[1], resize, crop, 'bicubic', M.DETECTOR_MEAN, M.DETECTOR_STD).tobytes() == want[1].tobytes()
    # the shorter side is already `resize` (no pass runs: crop and normalise alone), with one and three channels; one channel through both passes
    for shape, rs in (((2, 44, 32, 1), 32), ((1, 32, 32, 3), 32), ((2, 50, 40, 1), 32)):
        g = np.random.RandomState(shape[1]).randint(0, 256, size=shape).astype(np.uint8)
        k = dict(resize=rs, crop=24, mean=M.DETECTOR_MEAN[:shape[3]], std=M.DETECTOR_STD[:shape[3]])
        assert M.detector_input(torch.from_numpy(g).cuda(), **k).cpu().numpy().tobytes() == M.detector_input(g, **k).tobytes()


def test_out_guards_repeatability_and_empty_batch(M):
    x = torch.from_numpy(np.stack([R.make_input(8, (37, 53), 3, kind, key='g') for kind in R.KINDS])).cuda()
    want = M.resize(x, 16)
    n = want.numel()
    buf = torch.full([n + 24], 7, dtype=torch.uint8, device='cuda')
    M.resize(x, 16, out=buf[11:11 + n].view(want.shape))                                     # an odd offset inside a larger buffer
    assert torch.equal(buf[11:11 + n].view(want.shape), want) and bool((buf[:11] == 7).all()) and bool((buf[11 + n:] == 7).all())
    assert torch.equal(M.resize(x, 16), want)                                                # the same bytes on every run
    side = torch.cuda.Stream()                                                               # the cached tables were uploaded on the default stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = M.resize(x, 16)
    side.synchronize()
    assert torch.equal(other, want)
    d = dev16(np.stack([R.make_input(16, (37, 53), 1, kind, key='g') for kind in R.KINDS]))
    assert torch.equal(M.resize(d, 16).view(torch.int16), M.resize(d, 16).view(torch.int16))
    empty = M.resize(x[:0], 16)
    assert tuple(empty.shape) == (0, 16, 16, 3)
    assert tuple(M.detector_input(x[:0], resize=32, crop=24).shape) == (0, 3, 24, 24)


def test_native_route_refuses_cpu_tensors_and_names_its_limits(tdgp, M):
    x = torch.zeros([1, 8, 8, 3], dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='GPU'):
        M._resize_device(x, 8, (0, 0, 8, 8), 4, 4, 'lanczos', False, torch.zeros([1, 4, 4, 3], dtype=torch.uint8))
    L = tdgp._lib
    g = x.cuda()
    out = torch.zeros([1, 8, 8, 3], dtype=torch.uint8, device='cuda')
    with pytest.raises(L.Unsupported, match='at most 65535'):
        L.call('tdgp_resample_u8', g.data_ptr(), 65536, 8, 8, 3, 0, 0, 8, 8, None, None, 0, None, None, 0, out.data_ptr(), 8, 8, None, 0, L.stream_of(g))
    with pytest.raises(L.Unsupported, match='at most 32768'):
        L.call('tdgp_resample_u8', g.data_ptr(), 1, 8, 32769, 3, 0, 0, 8, 8, None, None, 0, None, None, 0, out.data_ptr(), 8, 8, None, 0, L.stream_of(g))
    with pytest.raises(RuntimeError, match='crop window'):
        L.call('tdgp_resample_u8', g.data_ptr(), 1, 8, 8, 3, 4, 0, 8, 8, None, None, 0, None, None, 0, out.data_ptr(), 8, 8, None, 0, L.stream_of(g))
    with pytest.raises(RuntimeError, match='tables are given exactly when'):
        L.call('tdgp_resample_u8', g.data_ptr(), 1, 8, 8, 3, 0, 0, 8, 8, None, None, 0, None, None, 0, out.data_ptr(), 4, 8, None, 0, L.stream_of(g))


class IntegerProjection(torch.nn.Module):
    """Exact on any device: x * 64 rounded to integers, 8 fixed positions summed per feature (integer sums below 2^24 are exact in fp32)."""

    def __init__(self, crop, features=6, seed=5):
        super().__init__()
        self.register_buffer('index', torch.from_numpy(np.random.RandomState(seed).randint(0, 3 * crop * crop, size=features * 8)))

    def forward(self, x):
        q = torch.round(x * 64.0).flatten(1)
        return q[:, self.index].reshape(x.shape[0], -1, 8).sum(dim=2)


def test_tools_on_the_device_match_the_host(tdgp, tmp_path):
    T = tdgp.data_tools
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'sub'))
    from PIL import Image                                     # the tools decode and encode with Pillow wherever they run
    for name, hw, c, bits in (('a.png', (40, 40), 3, 8), ('b.png', (48, 48), 3, 8), ('c.png', (40, 40), 3, 8), ('sub/d.png', (40, 56), 3, 8), ('sub/e.png', (30, 44), 1, 8),
                              ('f.png', (36, 50), 1, 16)):
        a = R.make_input(bits, hw, c, 'noise', key=name)
        Image.fromarray(a[:, :, 0] if bits == 8 and c == 1 else a).save(os.path.join(root, name))
    host, dev = str(tmp_path / 'host'), str(tmp_path / 'dev')
    rh, rd = T.resize_dataset(root, target_dir=host, size=16, device=None), T.resize_dataset(root, target_dir=dev, size=16, device='cuda')
    assert rh['resized'] == rd['resized'] == 6 and rd['device'].startswith('cuda')
    for d, _, files in os.walk(host):
        for f in files:
            assert open(os.path.join(d, f), 'rb').read() == open(os.path.join(dev, os.path.relpath(os.path.join(d, f), host)), 'rb').read(), f
    feats = str(tmp_path / 'feats')
    os.makedirs(feats)
    for name in ('a', 'b', 'c'):
        os.replace(os.path.join(root, name + '.png'), os.path.join(feats, name + '.png'))
    det = IntegerProjection(24).eval()
    T.extract_features(feats, det, str(tmp_path / 'h.memmap'), device=None, npy_path=str(tmp_path / 'h.npy'), resize=32, crop=24)
    T.extract_features(feats, det.cuda(), str(tmp_path / 'd.memmap'), device='cuda', npy_path=str(tmp_path / 'd.npy'), resize=32, crop=24)
    h, d = np.load(str(tmp_path / 'h.npy')), np.load(str(tmp_path / 'd.npy'))
    assert h.shape == (3, 6) and np.abs(h).max() > 0 and np.array_equal(h, d)

"""Training data on the host: image folder / zip dataset, the windowed infinite sampler and a threaded batch iterator.

Written from the behaviour of the reference's dataset (`src/training/dataset.py:29-361`): which files count as images, what one item holds,
how `max_size` and `mirror` select and double the items, how a mirrored yaw is reflected.  numpy + PIL only; the one PNG form PIL cannot
decode at full depth (16-bit grey + alpha, the two-channel depth maps) is decoded here from the file's own chunks.  `InfiniteSampler` yields
the indices of `src/torch_utils/misc.py:112-143`.  The batch iterator stands where `torch.utils.data.DataLoader(num_workers=3)` stands in the
reference: it prefetches with a small THREAD pool and starts no child process -- a forked child of a process that has the GPU open is unsafe,
and shared machines cap the processes per GPU -- and yields pinned uint8 / int32 batches ready for an asynchronous copy.
"""
import io
import json
import os
import struct
import threading
import zipfile
import zlib
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

DEPTH_SUFFIX = '_depth.png'
META_FILE = 'dataset.json'


def _lookup(node, dotted):
    for part in dotted.split('.'):
        node = node[part] if isinstance(node, dict) else getattr(node, part)
    return node


def prior_mean(node):
    """Mean of a scalar camera prior (`fov`, `origin.radius`): `mean` of a (truncated) normal, mid-point of a uniform range."""
    kind = _lookup(node, 'dist')
    if kind in ('normal', 'truncnorm'):
        return float(_lookup(node, 'mean'))
    if kind == 'uniform':
        return 0.5 * (float(_lookup(node, 'min')) + float(_lookup(node, 'max')))
    raise NotImplementedError(f'camera prior {kind!r} has no mean defined here')


def prior_mean_angles(node):
    """[yaw, pitch, roll] the angle prior is centred on; None for 'custom' (the dataset's own angles decide)."""
    kind = _lookup(node, 'dist')
    if kind == 'custom':
        return None
    if kind == 'normal':
        return [float(_lookup(node, 'yaw.mean')), float(_lookup(node, 'pitch.mean')), 0.0]
    if kind in ('uniform', 'truncnorm', 'spherical_uniform'):
        mid = lambda axis: 0.5 * (float(_lookup(node, axis + '.min')) + float(_lookup(node, axis + '.max')))      # noqa: E731
        return [mid('yaw'), mid('pitch'), 0.0]
    raise NotImplementedError(f'angle prior {kind!r} has no mean defined here')


def _base_camera():
    """configs/camera/base.yaml, the part a dataset needs (metrics.camera_base holds the whole node; this module stays free of torch)."""
    return dict(fov=dict(dist='uniform', min=10.0, max=45.0),
                origin=dict(radius=dict(dist='normal', mean=1.0, std=0.0),
                            angles=dict(dist='truncnorm', yaw=dict(min=-1.57079633, max=1.57079633, mean=0.0, std=0.4),
                                        pitch=dict(min=0.392699082, max=2.74889357, mean=1.57, std=0.2))))


# ----------------------------------------------------------------------------------------------------------------------
# 16-bit PNGs with an alpha channel: PIL reduces them to 8 bit, so the samples are taken from the file itself
# ----------------------------------------------------------------------------------------------------------------------
def _png_header(data):
    """(width, height, bit depth, colour type, interlace) or None when `data` is not a PNG."""
    if data[:8] != b'\x89PNG\r\n\x1a\n' or data[12:16] != b'IHDR':
        return None
    w, h, bits, colour, _, _, interlace = struct.unpack('>IIBBBBB', data[16:29])
    return w, h, bits, colour, interlace


def decode_png16(data):
    """A non-interlaced 16-bit greyscale PNG with or without alpha -> uint16 [h, w, channels] (1 or 2): inflate the IDAT stream and undo the
    five row filters of the PNG specification.  'Sub' and 'Up' are whole-row operations; 'Average' and 'Paeth' depend on the pixel to the
    left and walk the row pixel by pixel (all bytes of a pixel at once)."""
    hdr = _png_header(data)
    if hdr is None or hdr[2] != 16 or hdr[3] not in (0, 4) or hdr[4] != 0:
        raise ValueError('decode_png16 takes non-interlaced 16-bit greyscale PNGs (with or without alpha)')
    w, h, _, colour, _ = hdr
    channels = 2 if colour == 4 else 1
    bpp = 2 * channels
    pos, stream = 8, []
    while pos + 8 <= len(data):
        size, tag = struct.unpack('>I4s', data[pos:pos + 8])
        if tag == b'IDAT':
            stream.append(data[pos + 8:pos + 8 + size])
        if tag == b'IEND':
            break
        pos += 12 + size
    raw = np.frombuffer(zlib.decompress(b''.join(stream)), dtype=np.uint8)
    if raw.size != h * (1 + w * bpp):
        raise ValueError('PNG data stream has the wrong length')
    raw = raw.reshape(h, 1 + w * bpp)
    out = np.zeros((h, w, bpp), dtype=np.uint8)
    above = np.zeros((w, bpp), dtype=np.int32)
    for y in range(h):
        kind, line = int(raw[y, 0]), raw[y, 1:].reshape(w, bpp).astype(np.int32)
        if kind == 0:
            cur = line
        elif kind == 1:
            cur = np.cumsum(line, axis=0) & 255
        elif kind == 2:
            cur = (line + above) & 255
        elif kind in (3, 4):
            cur = np.empty_like(line)
            left, upleft = np.zeros(bpp, np.int32), np.zeros(bpp, np.int32)
            for x in range(w):
                up = above[x]
                if kind == 3:
                    pred = (left + up) >> 1
                else:
                    pa, pb, pc = np.abs(up - upleft), np.abs(left - upleft), np.abs(left + up - 2 * upleft)
                    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
                left = cur[x] = (line[x] + pred) & 255
                upleft = up
        else:
            raise ValueError(f'PNG row filter {kind} does not exist')
        out[y] = cur
        above = cur
    return np.ascontiguousarray(out).view('>u2').astype(np.uint16).reshape(h, w, channels)


# ----------------------------------------------------------------------------------------------------------------------
# where the files are
# ----------------------------------------------------------------------------------------------------------------------
class _Files:
    """The members of a directory tree or of a zip archive under their relative names; `read` is safe to call from several threads."""

    def __init__(self, path):
        self.path, self._zip, self._lock = path, None, threading.Lock()
        if os.path.isdir(path):
            self.names = sorted(os.path.relpath(os.path.join(d, f), path).replace(os.sep, '/') for d, _, fs in os.walk(path) for f in fs)
        elif os.path.splitext(path)[1].lower() == '.zip':
            self._zip = zipfile.ZipFile(path)
            self.names = sorted(n for n in self._zip.namelist() if not n.endswith('/'))
        else:
            raise IOError(f'{path}: a dataset is a directory or a .zip archive')

    def read(self, name):
        if self._zip is None:
            with open(os.path.join(self.path, name), 'rb') as f:
                return f.read()
        with self._lock:                                   # one archive handle, one reader at a time
            return self._zip.read(name)

    def close(self):
        if self._zip is not None:
            self._zip.close()
            self._zip = None


class ImageFolderDataset:
    """Images in a directory or a .zip, `NAME_depth.png` next to `NAME.<ext>`, one `dataset.json` with `labels` and `camera_angles` (lists of
    [relative file name, value]), optionally an embeddings memmap with its descriptor json.

    `ds[i]` -> dict(image uint8 [C, H, W], label float32 [c_dim], camera_angles float32 [3], depth int32 [1, H, W] (or [[0]] without
    depth), embedding float32 [E] (or [0])).  Integer labels are handed out one-hot, float label rows as they are.  `max_size` keeps a
    seeded random subset (in file order), `mirror` appends a second copy of every item flipped along W, with the yaw reflected about the
    mean yaw.  Everything but pixels is read at construction."""

    def __init__(self, path, resolution=None, use_depth=False, max_size=None, mirror=False, c_dim=0, use_embeddings=False, embeddings_path=None,
                 embeddings_desc_path=None, camera_cfg=None, random_seed=0):
        import PIL.Image
        PIL.Image.init()
        self._files = _Files(path)
        self.name = os.path.splitext(os.path.basename(os.path.normpath(path)))[0]
        known = PIL.Image.EXTENSION
        self.image_names = [n for n in self._files.names if os.path.splitext(n)[1].lower() in known and not n.endswith(DEPTH_SUFFIX)]
        if not self.image_names:
            raise IOError(f'{path}: no image files')
        self.image_shape = list(self._pixels(0).shape)
        if self.image_shape[1] != self.image_shape[2]:
            raise IOError(f'{path}: images must be square, the first one is {self.image_shape[2]} x {self.image_shape[1]}')
        if resolution is not None and self.image_shape[1] != resolution:
            raise IOError(f'{path}: images are {self.image_shape[1]}^2, not the requested {resolution}^2')
        self.camera_cfg = _base_camera() if camera_cfg is None else camera_cfg
        self.use_depth = bool(use_depth)
        count = len(self.image_names)

        meta = self._meta()
        self._labels = self._label_table(meta, count) if c_dim > 0 else np.zeros((count, 0), np.float32)
        self._angles = self._per_image(meta, 'camera_angles')
        self._angles = np.zeros((count, 3), np.float32) if self._angles is None else self._angles.astype(np.float32)
        if self._angles.shape != (count, 3):
            raise ValueError(f'camera_angles must be [yaw, pitch, roll] per image, got an array of shape {self._angles.shape}')
        self._embeddings, self._embedding_row = np.zeros((count, 0), np.float32), np.arange(count)
        if use_embeddings:
            with open(embeddings_desc_path) as f:
                desc = json.load(f)
            self._embeddings = np.memmap(embeddings_path, dtype='float32', mode='r', shape=tuple(desc['shape']))
            self._embedding_row = np.array([desc['filepath_to_idx'][self._meta_key(n)] for n in self.image_names], dtype=np.int64)

        # which image every item shows, and whether mirrored
        chosen = np.arange(count)
        if max_size is not None and max_size < count:
            np.random.RandomState(random_seed).shuffle(chosen)
            chosen = np.sort(chosen[:max_size])
        self.source_index = np.concatenate([chosen, chosen]) if mirror else chosen
        self.mirrored = np.concatenate([np.zeros(len(chosen), bool), np.ones(len(chosen), bool)]) if mirror else np.zeros(len(chosen), bool)

        centre = prior_mean_angles(_lookup(self.camera_cfg, 'origin.angles'))
        if centre is None:                                  # 'custom': the mean of the angles the dataset itself carries
            centre = self._angles.mean(axis=0)
        self.mean_camera_params = np.concatenate([np.asarray(centre, dtype=np.float64),
                                                  [prior_mean(_lookup(self.camera_cfg, 'fov')), prior_mean(_lookup(self.camera_cfg, 'origin.radius'))]])

    # ------------------------------------------------------------------------------------------------------------ metadata
    def _meta_key(self, name):
        """The key of `name` in dataset.json and in the embeddings descriptor: forward slashes, without the dataset's own name in front."""
        key = name.replace('\\', '/').lstrip('/')
        return key[len(self.name) + 1:] if key.startswith(self.name + '/') else key

    def _meta(self):
        found = [n for n in self._files.names if n.endswith(META_FILE)]
        if len(found) > 1:
            raise ValueError(f'a dataset holds one {META_FILE}, this one holds {len(found)}: {found}')
        return json.loads(self._files.read(found[0])) if found else {}

    def _per_image(self, meta, field):
        rows = meta.get(field)
        if rows is None:
            return None
        by_name = dict(rows)
        return np.array([by_name[self._meta_key(n)] for n in self.image_names])

    def _label_table(self, meta, count):
        table = self._per_image(meta, 'labels')
        if table is None:
            raise ValueError(f'c_dim > 0 needs a `labels` entry in {META_FILE}')
        if table.ndim == 1:                                 # class indices
            table = table.astype(np.int64)
            if table.min() < 0:
                raise ValueError('class labels must not be negative')
        elif table.ndim == 2:                               # label vectors
            table = table.astype(np.float32)
        else:
            raise ValueError(f'labels must be class indices or vectors, got an array of shape {table.shape}')
        assert len(table) == count
        return table

    # ------------------------------------------------------------------------------------------------------------ pixels
    def _pixels(self, src):
        import PIL.Image
        px = np.array(PIL.Image.open(io.BytesIO(self._files.read(self.image_names[src]))))
        return (px[:, :, None] if px.ndim == 2 else px).transpose(2, 0, 1)              # [C, H, W]

    def _depth_pixels(self, src):
        """int32 [1, H, W] on the 16-bit scale: an 8-bit file is multiplied by 256; of two channels the first is the depth."""
        import PIL.Image
        name = os.path.splitext(self.image_names[src])[0] + DEPTH_SUFFIX
        data = self._files.read(name)
        hdr = _png_header(data)
        if hdr is not None and hdr[2] == 16 and hdr[3] == 4:
            plane = decode_png16(data)[:, :, 0]                                         # grey + alpha: PIL would hand out 8 bits
        else:
            px = np.asarray(PIL.Image.open(io.BytesIO(data)))
            plane = px if px.ndim == 2 else px[:, :, 0]
            if hdr is not None and hdr[2] == 16 and plane.dtype == np.uint8:
                raise NotImplementedError(f'{name}: a 16-bit PNG of colour type {hdr[3]} is not a depth map this reader knows')
        if plane.dtype == np.uint8:
            plane = plane.astype(np.int32) * 256
        elif plane.dtype.kind not in 'ui' or plane.max() > 65535:
            raise ValueError(f'{name}: depth maps are 8- or 16-bit integer images, this one is {plane.dtype}')
        if list(plane.shape) != self.image_shape[1:]:
            raise ValueError(f'{name}: depth map of {plane.shape[1]} x {plane.shape[0]} next to an image of {self.image_shape[2]} x {self.image_shape[1]}')
        return plane.astype(np.int32)[None]

    # ------------------------------------------------------------------------------------------------------------ items
    def __len__(self):
        return len(self.source_index)

    def __getitem__(self, i):
        image = self._pixels(self.source_index[i])
        if list(image.shape) != self.image_shape or image.dtype != np.uint8:
            raise ValueError(f'{self.image_names[self.source_index[i]]}: {image.dtype} {list(image.shape)}, the dataset holds uint8 {self.image_shape}')
        if self.mirrored[i]:
            image = image[..., ::-1]
        return dict(image=np.ascontiguousarray(image), label=self.get_label(i), camera_angles=self.get_camera_angles(i),
                    depth=self.get_depth(i) if self.use_depth else np.zeros((1, 1), np.int32), embedding=self.get_embedding(i))

    def get_label(self, i):
        entry = self._labels[self.source_index[i]]
        if self._labels.dtype == np.int64:
            return np.eye(self.label_dim, dtype=np.float32)[entry]
        return np.array(entry, dtype=np.float32)

    def get_embedding(self, i):
        return np.array(self._embeddings[self._embedding_row[self.source_index[i]]], dtype=np.float32)

    def get_camera_angles(self, i):
        angles = self._angles[self.source_index[i]].copy()
        if self.mirrored[i]:
            mean_yaw = self.mean_camera_params[0]
            angles[0] = mean_yaw - (angles[0] - mean_yaw)                               # the yaw seen in a mirror standing at the mean yaw
        return angles

    def get_depth(self, i):
        if not self.use_depth:
            raise RuntimeError('the dataset was opened without use_depth')
        depth = self._depth_pixels(self.source_index[i])
        return np.ascontiguousarray(depth[..., ::-1] if self.mirrored[i] else depth)

    # ------------------------------------------------------------------------------------------------------------ shape
    num_channels = property(lambda self: self.image_shape[0])
    resolution = property(lambda self: self.image_shape[1])
    has_onehot_labels = property(lambda self: self._labels.dtype == np.int64)
    label_shape = property(lambda self: [int(self._labels.max()) + 1] if self.has_onehot_labels else list(self._labels.shape[1:]))
    label_dim = property(lambda self: self.label_shape[0])
    has_labels = property(lambda self: self.label_dim > 0)
    has_depth = property(lambda self: self.use_depth)

    def close(self):
        self._files.close()

    def __del__(self):
        files = self.__dict__.get('_files')
        if files is not None:
            files.close()


class InfiniteSampler:
    """misc.py:112-143: loops over the dataset for ever; after every index handed out (to whichever rank) the entry just passed is swapped
    with one up to `window_size * len` places behind it, so the order keeps drifting.  Rank r takes every `num_replicas`-th index."""

    def __init__(self, dataset, rank=0, num_replicas=1, shuffle=True, seed=0, window_size=0.5):
        assert len(dataset) > 0 and num_replicas > 0 and 0 <= rank < num_replicas and 0 <= window_size <= 1
        self.dataset, self.rank, self.num_replicas, self.shuffle, self.seed, self.window_size = dataset, rank, num_replicas, shuffle, seed, window_size

    def __iter__(self):
        import itertools
        n = len(self.dataset)
        order = np.arange(n)
        rnd, window = None, 0
        if self.shuffle:
            rnd = np.random.RandomState(self.seed)
            rnd.shuffle(order)
            window = int(np.rint(n * self.window_size))
        for step in itertools.count():                       # one step per index handed out to ANY rank: all ranks walk the same sequence
            here = step % n
            if step % self.num_replicas == self.rank:
                yield order[here]
            if window >= 2:                                  # one draw per step, taken whether or not this rank took the index
                there = (here - rnd.randint(window)) % n
                order[[here, there]] = order[[there, here]]


def _collate(items, pin):
    import torch
    out = {}
    for k in items[0]:
        t = torch.from_numpy(np.stack([it[k] for it in items]))
        out[k] = t.pin_memory() if pin else t
    return out


def batch_iterator(dataset, sampler, batch_size, workers=3, prefetch=2, pin_memory=None):
    """Endless batches dict(image uint8 [B, C, H, W], label, camera_angles, depth int32, embedding) in the sampler's order.  Items are read by
    `workers` threads (PNG decoding releases the GIL), `prefetch` batches ahead; no child process is started.  Batches are pinned when a GPU
    is there (`pin_memory=None`) so that `.to(device, non_blocking=True)` overlaps with compute."""
    import torch
    pin = torch.cuda.is_available() if pin_memory is None else bool(pin_memory)
    it = iter(sampler)
    with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
        pending = deque()
        try:
            while True:
                while len(pending) <= prefetch:
                    pending.append([pool.submit(dataset.__getitem__, int(next(it))) for _ in range(batch_size)])
                yield _collate([f.result() for f in pending.popleft()], pin)
        finally:
            for batch in pending:
                for f in batch:
                    f.cancel()

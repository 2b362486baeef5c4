"""The offline data scripts of the reference's ImageNet recipe (`scripts/data_scripts/`): `resize_dataset`, `merge_depth_data`,
`extract_features`.  Written from their behaviour; what they write is what `dataset.ImageFolderDataset` and
`instance_selection.run_instance_selection` read.

The resampling runs through `images` (Pillow's arithmetic, bit for bit): on the GPU for `device='cuda'`, on the host for `device=None`.
Decoding and encoding stay on the host in a thread pool of at most 16 threads (PIL releases the GIL while it decodes and encodes); no child
process is started next to a process that holds the GPU.  The detector of `extract_features` is the caller's, as everywhere in this package.
"""
import json
import os
import re
import shutil
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import images
from .instance_selection import find_images_in_dir

MAX_THREADS = 16
DEVICE_MODES = ('L', 'RGB', 'I;16')          # what the kernels take; every other mode stays with Pillow on the host
CHUNK_FILES = 128                            # images decoded ahead of one round of device calls


def _suffix(path):
    """Lower-case extension of a path, with its dot."""
    return os.path.splitext(str(path))[1].lower()


def _threads(threads):
    return max(1, min(MAX_THREADS, int(threads)))


def _device_of(device):
    if device is None:
        return None
    device = torch.device(device)
    if device.type != 'cuda':
        raise ValueError(f'device={str(device)!r}: the device route needs a GPU (its kernels have no CPU path); device=None is the host route')
    return device


class _Clock:
    """Seconds per stage, summed over the threads that spent them."""

    def __init__(self):
        self.seconds = {}
        self._lock = threading.Lock()

    def add(self, stage, t0):
        spent = time.perf_counter() - t0
        with self._lock:
            self.seconds[stage] = self.seconds.get(stage, 0.0) + spent


# ----------------------------------------------------------------------------------------------------------------------
# resize_dataset
# ----------------------------------------------------------------------------------------------------------------------
JPEG_QUALITY = 95                                            # for files named `.jpg`; `.jpeg` keeps Pillow's default, as in the reference
FOUR_BAND_MODES = ('RGBA', 'RGBa', 'RGBX', 'CMYK')           # a JPEG cannot hold them as they are


def write_image(img, path):
    """Save a PIL image the way the reference's resize script does: a four-band image bound for a JPEG file is laid over a white RGB canvas
    with its last band as the mask; otherwise CMYK becomes RGB and everything else is saved in its own mode."""
    import PIL.Image
    suffix = _suffix(path)
    options = dict(quality=JPEG_QUALITY) if suffix == '.jpg' else {}
    if img.mode in FOUR_BAND_MODES and suffix in ('.jpg', '.jpeg'):
        canvas = PIL.Image.new('RGB', img.size, 'white')
        canvas.paste(img, mask=img.getchannel(3))
        img = canvas
    elif img.mode == 'CMYK':
        img = img.convert('RGB')
    img.save(path, **options)


def _pillow_center_resize_crop(img, size):
    """The reference's route for the modes the kernels do not take: torchvision's centre crop and Lanczos resize on the PIL image."""
    import PIL.Image
    w, h = img.size
    side = min(w, h)
    top, left = images.center_crop_box(h, w, side, side)
    img = img.crop((left, top, left + side, top + side))
    return img if side == size else img.resize((size, size), PIL.Image.LANCZOS)


def _to_array(img):
    a = np.asarray(img)
    return a[:, :, None] if img.mode == 'L' else a


def _from_array(a):
    import PIL.Image
    return PIL.Image.fromarray(a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a)


def _files_below(root):
    """Every file under `root` by its path relative to `root`, sorted."""
    found = []
    for folder, _, files in os.walk(root):
        inside = os.path.relpath(folder, root)
        found += [os.path.normpath(os.path.join(inside, f)) for f in files]
    return sorted(found)


def _plan_resize(source_dir, target_dir, format, ignore_ext, ignore_regex, images_only, fname_prefix, rename_enum):
    """-> (image pairs, copy pairs) of (source path, target path).  A file is left out when its relative path ends in `ignore_ext` or matches
    `ignore_regex` as a whole.  An image keeps its relative name without the extension, with `fname_prefix` in front of it, or takes its
    eight-digit position in the sorted listing with `rename_enum`; its extension is `format` when one is given."""
    import PIL.Image
    PIL.Image.init()
    known = PIL.Image.EXTENSION
    unwanted = re.compile(ignore_regex) if ignore_regex is not None else None
    to_resize, to_copy = [], []
    position = -1
    for rel in _files_below(source_dir):
        if ignore_ext is not None and rel.endswith(ignore_ext):
            continue
        if unwanted is not None and unwanted.fullmatch(rel):
            continue
        position += 1
        here = os.path.join(source_dir, rel)
        suffix = _suffix(rel)
        if suffix in known:
            stem = '%08d' % position if rename_enum else fname_prefix + os.path.splitext(rel)[0]
            there = os.path.join(target_dir, stem + (format or suffix))
            if _suffix(there) not in known:
                raise ValueError(f'{there}: Pillow has no image format for the extension {_suffix(there)!r}')
            to_resize.append((here, there))
        elif not images_only:
            if os.path.islink(here):
                raise ValueError(f'{here}: links are not copied')
            to_copy.append((here, os.path.join(target_dir, rel)))
    return to_resize, to_copy


def resize_dataset(source_dir, target_dir=None, size=None, format=None, ignore_ext='.DS_Store', ignore_regex=None, images_only=False, fname_prefix='',
                   rename_enum=False, ignore_grayscale=False, ignore_broken=False, ignore_existing=False, device='cuda', threads=MAX_THREADS):
    """`scripts/data_scripts/resize_dataset.py`: every image under `source_dir` centre-cropped to a square and resized to `size`^2 (Lanczos),
    written to the same relative path under `target_dir` (default `{source_dir}_{size}`; `format` replaces the extension, `fname_prefix` is put
    in front of the relative name, `rename_enum` numbers the files in sorted order); every other file is copied unless `images_only`.

    `L`, `RGB` and `I;16` images go through `images.center_resize_crop` on `device` (images of one size and mode are batched); every other
    mode (`P`, `1`, `LA` / `RGBA`, `CMYK`, ...) goes through Pillow on the host exactly as the reference does and is counted as `host_fallback`.
    Returns the dict the command line prints: counts and the seconds spent decoding, resampling, encoding and copying."""
    import PIL.Image
    if size is None:
        raise ValueError('resize_dataset: size must be given')
    size = int(size)
    device = _device_of(device)
    source_dir = os.path.normpath(source_dir)
    if target_dir is None:
        target_dir = source_dir + '_' + str(size)
    jobs, copies = _plan_resize(source_dir, target_dir, format, ignore_ext, ignore_regex, images_only, fname_prefix, rename_enum)
    for folder in {os.path.dirname(trg) for _, trg in jobs + copies}:
        os.makedirs(folder or '.', exist_ok=True)

    clock = _Clock()
    counts = dict(resized=0, host_fallback=0, skipped=0)
    t_start = time.perf_counter()

    def decode(job):
        """-> (job, array or None, fallback done?)"""
        src, trg = job
        if ignore_existing and os.path.isfile(trg):
            return job, None, False
        t0 = time.perf_counter()
        try:
            img = PIL.Image.open(src)
            if img.mode == 'L' and ignore_grayscale:
                return job, None, False
            img.load()
        except Exception:
            if ignore_broken:
                return job, None, False
            raise
        finally:
            clock.add('decode', t0)
        if img.mode in DEVICE_MODES:
            return job, _to_array(img), False
        t0 = time.perf_counter()
        out = _pillow_center_resize_crop(img, size)
        clock.add('resample', t0)
        t0 = time.perf_counter()
        write_image(out, trg)
        clock.add('encode', t0)
        return job, None, True

    def encode(item):
        trg, a = item
        t0 = time.perf_counter()
        write_image(_from_array(a), trg)
        clock.add('encode', t0)

    def copy(item):
        t0 = time.perf_counter()
        shutil.copyfile(item[0], item[1])
        clock.add('copy', t0)

    with ThreadPoolExecutor(max_workers=_threads(threads)) as pool:
        copied = list(pool.map(copy, copies))
        pending = None
        chunks = [jobs[a:a + CHUNK_FILES] for a in range(0, len(jobs), CHUNK_FILES)]
        ahead = pool.map(decode, chunks[0]) if chunks else None
        for ci in range(len(chunks)):
            decoded = list(ahead)
            ahead = pool.map(decode, chunks[ci + 1]) if ci + 1 < len(chunks) else None      # the next chunk decodes while this one is resampled
            groups = {}
            for (src, trg), arr, fell_back in decoded:
                if arr is None:
                    counts['host_fallback' if fell_back else 'skipped'] += 1
                else:
                    groups.setdefault((arr.shape, arr.dtype.str), []).append((trg, arr))
            done = []
            t0 = time.perf_counter()
            for members in groups.values():
                batch = np.stack([arr for _, arr in members])
                if device is None:
                    res = images.center_resize_crop(batch, size)
                else:
                    x = torch.from_numpy(batch.view(np.int16) if batch.dtype == np.uint16 else batch).to(device)
                    x = x.view(torch.uint16) if batch.dtype == np.uint16 else x
                    res = images.center_resize_crop(x, size)
                    res = (res.view(torch.int16).cpu().numpy().view(np.uint16) if batch.dtype == np.uint16 else res.cpu().numpy())
                done += [(trg, res[i]) for i, (trg, _) in enumerate(members)]
            clock.add('resample', t0)
            counts['resized'] += len(done)
            if pending is not None:
                list(pending)                                  # the previous chunk's files are written while this one was decoded and resampled
            pending = pool.map(encode, done)
        if pending is not None:
            list(pending)
    sec = {k: round(clock.seconds.get(k, 0.0), 4) for k in ('decode', 'resample', 'encode', 'copy')}
    sec['total'] = round(time.perf_counter() - t_start, 4)
    return dict(source_dir=source_dir, target_dir=target_dir, size=size, num_images=len(jobs), copied=len(copied), device=str(device) if device else 'cpu',
                seconds=sec, **counts)


# ----------------------------------------------------------------------------------------------------------------------
# merge_depth_data
# ----------------------------------------------------------------------------------------------------------------------
def merge_depth_data(images_dir, depths_dir, target_dir):
    """`scripts/data_scripts/merge_depth_data.py`: for every `NAME.jpg` under `images_dir` that has a `NAME.png` at the same relative path
    under `depths_dir`, copy the image and the depth map side by side as `NAME.jpg` and `NAME_depth.png` under `target_dir` -- the layout
    `ImageFolderDataset(use_depth=True)` reads.  Returns the merged relative paths, sorted."""
    depth_of = {os.path.splitext(p)[0]: p for p in find_images_in_dir(depths_dir) if _suffix(p) == '.png'}
    merged = []
    for name in find_images_in_dir(images_dir):                       # sorted
        stem = os.path.splitext(name)[0]
        if _suffix(name) != '.jpg' or stem not in depth_of:
            continue
        image_to = os.path.join(target_dir, name)
        os.makedirs(os.path.dirname(image_to) or '.', exist_ok=True)
        shutil.copy(os.path.join(images_dir, name), image_to)
        shutil.copy(os.path.join(depths_dir, depth_of[stem]), os.path.join(target_dir, stem + '_depth.png'))
        merged.append(name)
    return merged


# ----------------------------------------------------------------------------------------------------------------------
# extract_features
# ----------------------------------------------------------------------------------------------------------------------
def feature_image_paths(dataset_path):
    """The images `extract_features` embeds, in row order: `find_images_in_dir` without the depth maps (`extract_features.py:123`)."""
    return [p for p in find_images_in_dir(dataset_path) if not re.fullmatch('.*_depth.png', p)]


def extract_features(dataset_path, detector, output_path, batch_size=256, device='cuda', npy_path=None, threads=MAX_THREADS, **detector_input_kwargs):
    """`scripts/data_scripts/extract_features.py`: `detector` (a callable on fp32 [B, 3, crop, crop] batches returning [B, F]; the command line
    loads a TorchScript module) on every image of `dataset_path`, each converted to RGB and passed through `images.detector_input` (keyword
    arguments beyond these go there).  Images of equal size inside a window of `batch_size` files share a call.

    Writes `output_path` (`*.memmap`, float32 [N, F]) and `*_desc.json` (`{"shape": [N, F], "filepath_to_idx": {relative path: row}}`, forward
    slashes) as the reference does -- what `ImageFolderDataset(use_embeddings=True)` opens -- and, with `npy_path`, the same [N, F] array as
    `.npy` in discovery order, which `run_instance_selection(embeddings=...)` takes.  Returns a summary dict."""
    import PIL.Image
    if not str(output_path).endswith('.memmap'):
        raise ValueError(f'extract_features: output_path must be a *.memmap file name, got {output_path}')
    device = _device_of(device)
    paths = feature_image_paths(dataset_path)
    if not paths:
        raise ValueError(f'extract_features: no image files under {dataset_path}')
    batch_size = max(1, int(batch_size))
    clock = _Clock()
    t_start = time.perf_counter()

    def decode(p):
        t0 = time.perf_counter()
        a = np.asarray(PIL.Image.open(os.path.join(dataset_path, p)).convert('RGB'), dtype=np.uint8)
        clock.add('decode', t0)
        return a

    os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
    desc_path = str(output_path).replace('.memmap', '_desc.json')
    feats = None                                       # the memmap itself, opened when the first batch tells the feature width: rows never pile up in RAM
    with ThreadPoolExecutor(max_workers=_threads(threads)) as pool, torch.no_grad():
        nxt = pool.map(decode, paths[:batch_size])
        for a in range(0, len(paths), batch_size):
            decoded = list(nxt)
            nxt = pool.map(decode, paths[a + batch_size:a + 2 * batch_size])        # the next window decodes while this one is embedded
            groups = {}
            for i, arr in enumerate(decoded):
                groups.setdefault(arr.shape, []).append(a + i)
            for rows in groups.values():
                t0 = time.perf_counter()
                x = torch.from_numpy(np.stack([decoded[i - a] for i in rows]))
                x = images.detector_input(x if device is None else x.to(device), **detector_input_kwargs)
                clock.add('transform', t0)
                t0 = time.perf_counter()
                out = detector(x)
                out = out.detach().float().cpu().numpy() if isinstance(out, torch.Tensor) else np.asarray(out, dtype=np.float32)
                clock.add('detector', t0)
                if out.ndim != 2 or out.shape[0] != len(rows) or (feats is not None and out.shape[1] != feats.shape[1]):
                    raise ValueError(f'the detector returned shape {out.shape} for {len(rows)} images; expected [{len(rows)}, {"F" if feats is None else feats.shape[1]}]')
                t0 = time.perf_counter()
                if feats is None:
                    feats = np.memmap(output_path, dtype='float32', mode='w+', shape=(len(paths), out.shape[1]))
                feats[rows] = out
                clock.add('write', t0)
    t0 = time.perf_counter()
    feats.flush()
    num_features = int(feats.shape[1])
    with open(desc_path, 'w') as f:
        json.dump({'shape': [len(paths), num_features], 'filepath_to_idx': {p.replace(os.sep, '/'): i for i, p in enumerate(paths)}}, f)
    if npy_path is not None:
        np.save(npy_path, feats)                       # straight from the mapped file
    del feats
    clock.add('write', t0)
    sec = {k: round(clock.seconds.get(k, 0.0), 4) for k in ('decode', 'transform', 'detector', 'write')}
    sec['total'] = round(time.perf_counter() - t_start, 4)
    return dict(dataset_path=str(dataset_path), output_path=str(output_path), desc_path=desc_path, npy_path=None if npy_path is None else str(npy_path),
                num_images=len(paths), num_features=num_features, device=str(device) if device else 'cpu', seconds=sec)

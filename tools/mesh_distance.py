#!/usr/bin/env python3
"""How far mesh A is from mesh B: the sampled two-sided surface distance (maximum = Hausdorff, area-weighted mean and RMS) on the GPU.

    python tools/mesh_distance.py decimated.obj full.ply --json distance.json --ply decimated_error.ply

A and B are .obj / .ply files as `geometry.save_obj` / `geometry.save_ply` write them (the readers below take exactly those layouts).
`--spacing` is the sampling resolution in the units of the files (default: each mesh's own default, twice the root of its mean triangle
area); the result is a lower bound of the true Hausdorff distance at that resolution.  `--one-sided` measures A -> B only.  `--ply PATH`
writes A with its per-vertex distance to B as colours (dark blue: 0, red: the largest vertex distance).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLY_TYPES = {'float': '<f4', 'uchar': 'u1', 'int': '<i4'}


def read_obj(path):
    """`v x y z` and `f a b c` / `a//na` / `a/ta` / `a/ta/na` lines (1-based) -> (vertices fp32 [V,3], triangles int32 [T,3]); other lines are skipped."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            part = line.split()
            if not part:
                continue
            if part[0] == 'v':
                v.append([np.float32(x) for x in part[1:4]])
            elif part[0] == 'f':
                if len(part) != 4:
                    raise ValueError(f'{path}: only triangles are read, got {line.strip()!r}')
                f.append([int(x.split('/')[0]) - 1 for x in part[1:4]])
    return np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)


def read_ply(path):
    """Binary little-endian .ply with float x y z first among the vertex properties (normals and colours may follow) and faces as a uchar
    count of 3 and three int32 indices -> (vertices fp32 [V,3], triangles int32 [T,3])."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError(f'{path}: not a .ply file')
    lines = data[:end].decode('ascii').split('\n')
    if 'format binary_little_endian 1.0' not in lines:
        raise ValueError(f'{path}: only binary little-endian .ply files are read')
    counts, props, element = {}, [], None
    for line in lines:
        part = line.split()
        if part[:1] == ['element']:
            element, counts[part[1]] = part[1], int(part[2])
        elif part[:1] == ['property'] and element == 'vertex':
            if part[1] not in PLY_TYPES:
                raise ValueError(f'{path}: vertex property of type {part[1]!r}')
            props.append((part[2], PLY_TYPES[part[1]]))
        elif part[:1] == ['property'] and element == 'face' and part[1:] != ['list', 'uchar', 'int', 'vertex_indices']:
            raise ValueError(f'{path}: faces must be `property list uchar int vertex_indices`')
    if [n for n, _ in props[:3]] != ['x', 'y', 'z'] or any(t != '<f4' for _, t in props[:3]):
        raise ValueError(f'{path}: the vertex must start with float x y z')
    at = end + len(b'end_header\n')
    V, T = counts.get('vertex', 0), counts.get('face', 0)
    vert = np.frombuffer(data, dtype=np.dtype(props), count=V, offset=at)
    faces = np.frombuffer(data, dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]), count=T, offset=at + V * vert.dtype.itemsize)
    if T and (faces['n'] != 3).any():
        raise ValueError(f'{path}: only triangles are read')
    return np.stack([vert['x'], vert['y'], vert['z']], 1).astype(np.float32).reshape(-1, 3), np.ascontiguousarray(faces['i'], np.int32).reshape(-1, 3)


def read_mesh(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == '.obj':
        return read_obj(path)
    if ext == '.ply':
        return read_ply(path)
    raise ValueError(f'{path}: .obj or .ply expected')


def _positive(s):
    x = float(s)
    if not 0 < x < float('inf'):
        raise argparse.ArgumentTypeError(f'a positive finite number is expected, got {s!r}')
    return x


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('a', metavar='A', help='the mesh that is measured (.obj / .ply)')
    p.add_argument('b', metavar='B', help='the mesh it is measured against (.obj / .ply)')
    p.add_argument('--spacing', type=_positive, default=None, help="sampling resolution (default: each mesh's own)")
    p.add_argument('--one-sided', action='store_true', help='A -> B only')
    p.add_argument('--json', default=None, metavar='PATH', help='write the statistics as JSON')
    p.add_argument('--ply', default=None, metavar='PATH', help='write A with its per-vertex distance to B as colours')
    return p.parse_args(argv)


def _side(s):
    return None if s is None else dict(max=s.max, mean=s.mean, rms=s.rms, area=s.area, argmax_sample=s.argmax_sample, samples=s.samples)


def report(d):
    """MeshDistance -> the dict that is printed and written."""
    return dict(hausdorff=d.hausdorff, mean=d.mean, rms=d.rms, a_to_b=_side(d.a_to_b), b_to_a=_side(d.b_to_a))


def main(argv=None):
    args = parse_args(argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    tdgp = importlib.import_module('3dgp_amd')
    M = tdgp.mesh_distance
    (va, ta), (vb, tb) = ((torch.from_numpy(x).to('cuda') for x in read_mesh(path)) for path in (args.a, args.b))
    d = M.mesh_distance(va, ta, vb, tb, spacing=args.spacing, symmetric=not args.one_sided)
    out = report(d)
    out.update(a=dict(path=args.a, vertices=int(va.shape[0]), triangles=int(ta.shape[0])), b=dict(path=args.b, vertices=int(vb.shape[0]), triangles=int(tb.shape[0])),
               spacing=args.spacing)
    if args.ply is not None:
        dist = M.vertex_distances(va, M.build_grid(vb, tb)).distance
        finite = dist[torch.isfinite(dist)]
        top = float(finite.max()) if finite.numel() else 0.0
        tdgp.geometry.save_ply(args.ply, va, ta, colours=M.error_colours(dist, top))
        out['vertex_max'] = top
    print(json.dumps(out))
    if args.json is not None:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == '__main__':
    main()

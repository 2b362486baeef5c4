#!/usr/bin/env python3
"""Train or fine-tune a generator: the command line of 3dgp_amd/training_loop.py.

    python tools/train.py --config run.yaml [--outdir runs/exp1] [key=value ...]

`run.yaml` holds `TrainingOptions` fields (3dgp_amd/training_loop.py); `key=value` / `key.sub=value` arguments override them, values parsed
as yaml (`total_kimg=100`, `augment.mode=ada`, `patch.resolution=64`).  An unknown key is an error.  Fine-tuning an exported checkpoint:
`resume=DIR` (the directory `weights.load_exported` reads) without `generator`.  Under torchrun (RANK / WORLD_SIZE set) every rank runs
this script; gradients are exchanged over RCCL.  Prints one JSON line at the end: the final stats and the run directory.
"""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--config', required=True, help='yaml file of TrainingOptions fields')
    ap.add_argument('--outdir', default=None, help='run directory (default: runs/<config name>)')
    ap.add_argument('overrides', nargs='*', help='key=value overrides')
    args = ap.parse_args(argv)
    import yaml
    tdgp = importlib.import_module('3dgp_amd')
    TL = tdgp.training_loop
    with open(args.config) as f:
        d = yaml.safe_load(f) or {}
    opts = TL.TrainingOptions.from_dict(TL.apply_overrides(d, args.overrides))
    run_dir = args.outdir or os.path.join('runs', os.path.splitext(os.path.basename(args.config))[0])
    rank, world, _ = tdgp.distributed.init_from_env()
    if rank == 0:
        os.makedirs(run_dir, exist_ok=True)
        with open(os.path.join(run_dir, 'options.yaml'), 'w') as f:
            f.write(opts.to_yaml())
    stats = TL.training_loop(opts, run_dir, rank=rank, world=world)
    if rank == 0:
        print(json.dumps(dict(run_dir=run_dir, world=world, **{k: (None if isinstance(v, float) and v == float('inf') else v) for k, v in stats.items()})))
    return stats


if __name__ == '__main__':
    main()

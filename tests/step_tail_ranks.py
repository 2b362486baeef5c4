"""One rank of tests/test_step_tail_gpu.py::test_two_ranks_share_one_gpu: a process of its own with its own HIP context on GPU 0, a gloo
process group (RCCL cannot put two ranks on one device), gradients that depend on the rank, one `FusedStepTail.step(world=2)`; the
parameters go to `<argv[1]>.rank<r>.pt`.  `make` and `grads` are imported by the test for the single-process restatement."""
import importlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 50.0
COUNTS = (3, 5, 4097, 8197)


def make(dev):
    g = torch.Generator().manual_seed(7)
    mod = torch.nn.Module()
    mod.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g).to(dev)) for n in COUNTS])
    return mod, torch.optim.Adam(mod.parameters(), lr=2e-3, betas=(0.0, 0.99), eps=1e-8)


def grads(mod, rank):
    """CPU tensors; rank 0 carries an inf and a NaN (the sum of the two ranks is sanitised, not each addend)."""
    g = torch.Generator().manual_seed(50 + rank)
    out = [torch.randn(p.shape, generator=g) for p in mod.ps]
    if rank == 0:
        out[1][4] = float('inf')
        out[3][4096] = float('nan')
    return out


def main():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch.distributed as dist
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    tdgp = importlib.import_module('3dgp_amd')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mod, opt = make('cuda:0')
    for p, g in zip(mod.ps, grads(mod, rank)):
        p.grad = g.to('cuda:0')
    rec = tdgp.step_tail.FusedStepTail(mod, opt).step(world=world, grad_clip=CLIP)
    assert rec['launches'] == 4
    torch.cuda.synchronize()
    torch.save([p.detach().cpu() for p in mod.ps], f'{sys.argv[1]}.rank{rank}.pt')
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

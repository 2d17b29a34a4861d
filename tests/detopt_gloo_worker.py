"""One rank of tests/test_detector_optim_host.py's gloo run: allreduce_gradients(FlatSGD) leaves the mean of the ranks' gradients in the flat
buffer, a gradient that was detached from the buffer on one rank included."""
import os
import pathlib
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
SHAPES = [(3, 5), (7,), (2, 2, 3), (1,)]               # 15, 7, 12, 1 elements: every start but the first needs padding


def gradients(rank):
    return [torch.arange(1, 1 + torch.Size(s).numel(), dtype=torch.float32).reshape(s) * (rank + 1) * (i + 1) for i, s in enumerate(SHAPES)]


def worker(rank, world, port, q):
    try:
        sys.path.insert(0, str(REPO))
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import torch.distributed as dist
        from cosypose_amd.detector_optim import FlatSGD
        from cosypose_amd.train_engine import allreduce_gradients
        dist.init_process_group('gloo', rank=rank, world_size=world)
        params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
        opt = FlatSGD(params, lr=0.1)
        with torch.no_grad():
            for p, g in zip(params, gradients(rank)):
                p.grad.copy_(g)
        if rank == 1:                                   # Detector.zero_grad() then a backward: a fresh tensor, not the view
            params[1].grad = None
            params[1].grad = gradients(rank)[1].clone()
            params[3].grad = None                       # no gradient at all on this rank: zeros
        out = allreduce_gradients(opt)
        ok = out is opt.grad
        for i, (p, o) in enumerate(zip(params, opt.offsets)):
            per_rank = [gradients(r)[i] for r in range(world)]
            if i == 3:
                per_rank[1] = torch.zeros_like(per_rank[1])
            want = sum(per_rank) / world
            ok &= torch.equal(opt.grad[o:o + p.numel()].view(p.shape), want) and p.grad.data_ptr() == opt.grad.data_ptr() + 4 * o
        used = torch.zeros(opt.grad.numel(), dtype=torch.bool)
        for p, o in zip(params, opt.offsets):
            used[o:o + p.numel()] = True
        ok &= bool((opt.grad[~used] == 0).all())         # the padding stays zero through the collective
        q.put((rank, bool(ok)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        traceback.print_exc()
        q.put((rank, False))
        raise

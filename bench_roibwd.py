#!/usr/bin/env python3
"""Timing of the backward of the multi-scale RoIAlign into the feature maps (cosy_msroi_align_backward, csrc/kernels_detpre.hip, DESIGN.md
section 24) on one GPU.  Features as in bench_rpn.py: 8 frames seen at 800x1067, the first four FPN levels (200x272 ... 25x34), C = 256.
Rows as detector_losses makes them (bench_dettrain.py): 8 x 512 padded rows at 7 x 7 for the box head, 8 x 128 at 14 x 14 for the mask head,
sampling_ratio 2.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_roibwd.py --out profiles/roibwd_bench.json

Each stage is the median WALL time of `--runs` backward calls (torch.autograd.grad through the retained graph of one forward, synchronised
before and after) after `--warmup` calls.  It is timed in the same process against the same contract as differentiable torch ops on the device
(bench_rpn.py's gather-based bilinear over chunks of 256 boxes, whose backward is autograd's index_put with accumulation): what a user has
without this kernel.  No ratio is fixed in advance: a stage that comes out slower than the torch route says so (`slower_than_torch_ops`).
`store_GBps`: the bytes of the gradients of the four levels, each written once, over the kernel route's time; `copy_GBps`: a device-to-device
copy of as many bytes in the same process (read + write counted once, as the stores are).  `equal`: the two routes' gradients agree to 1e-4
of the largest gradient (both are float32 sums, in different orders; the tests hold the kernel to float64 within a derived bound)."""
import argparse
import json
import math
import statistics
import subprocess
import time

GRID = [(200, 272), (100, 136), (50, 68), (25, 34)]
NET = (800, 1067)


def torch_roi_align(feats, scales, boxes, im_ids, P, g, chunk=256):
    """bench_rpn.py's torch route, kept differentiable with respect to the features"""
    import torch
    C = feats[0].shape[1]
    s = torch.sqrt((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))
    k_min, k_max = round(-math.log2(scales[0])), round(-math.log2(scales[-1]))
    lvl = torch.floor(4 + torch.log2(s / 224 + 1e-6)).clamp(k_min, k_max).long() - k_min
    grid = (torch.arange(P, device=boxes.device, dtype=torch.float32)[:, None]
            + (torch.arange(g, device=boxes.device, dtype=torch.float32)[None, :] + 0.5) / g).reshape(-1)

    def axis(lo, hi, scale, size):
        start = lo * scale
        bin_ = (hi * scale - start).clamp(min=1) / P
        v = start[:, None] + grid[None, :] * bin_[:, None]
        ok = (v >= -1) & (v <= size)
        v = v.clamp(min=0)
        low = v.floor().long().clamp(max=size - 1)
        high = (low + 1).clamp(max=size - 1)
        l = torch.where(low >= size - 1, torch.zeros_like(v), v - low)
        return ok, low, high, l, 1 - l
    parts, order = [], []
    for l, f in enumerate(feats):
        rows = torch.nonzero(lvl == l).reshape(-1)
        H, W = f.shape[2:]
        fi = f.permute(0, 2, 3, 1)
        for at in range(0, len(rows), chunk):
            r = rows[at:at + chunk]
            bx, im = boxes[r], im_ids[r]
            oy, y0, y1, ly, hy = axis(bx[:, 1], bx[:, 3], scales[l], H)
            ox, x0, x1, lx, hx = axis(bx[:, 0], bx[:, 2], scales[l], W)
            tap = lambda yy, xx: fi[im[:, None, None], yy[:, :, None], xx[:, None, :]]
            wgt = lambda a, b: (a[:, :, None] * b[:, None, :])[..., None]
            v = wgt(hy, hx) * tap(y0, x0) + wgt(hy, lx) * tap(y0, x1) + wgt(ly, hx) * tap(y1, x0) + wgt(ly, lx) * tap(y1, x1)
            v = v * (oy[:, :, None] & ox[:, None, :])[..., None]
            parts.append(v.reshape(len(r), P, g, P, g, C).sum((2, 4)).permute(0, 3, 1, 2) / (g * g))
            order.append(r)
    return torch.cat(parts)[torch.argsort(torch.cat(order))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--commit', default=None, help='the commit the measured tree stands on (default: asked of git, where there is a repository)')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build
    from cosypose_amd.detector_rpn import infer_scales, multiscale_roi_align
    assert torch.cuda.is_available(), 'bench_roibwd.py needs a ROCm device'
    B, C, g = args.frames, args.channels, 2
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    rng = np.random.RandomState(args.seed)
    nets = [NET] * B
    scales = infer_scales(GRID, nets)
    grad_bytes = sum(B * C * H * W * 4 for H, W in GRID)

    def wall(call, runs, warmup):
        for _ in range(warmup):
            call()
        out = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(out), 3), [round(v, 3) for v in out]

    src, dst = torch.empty(grad_bytes // 4, device='cuda'), torch.empty(grad_bytes // 4, device='cuda')
    copy_ms, _ = wall(lambda: dst.copy_(src), args.runs, args.warmup)
    del src, dst
    stages = {}
    for name, rows, P in (('box_head_7', 512, 7), ('mask_head_14', 128, 14)):
        side = np.exp(rng.uniform(np.log(24), np.log(700), B * rows))          # sides from 24 to 700 px: every level gets rows
        w, h = side * rng.uniform(0.6, 1.6, B * rows), side / rng.uniform(0.6, 1.6, B * rows)
        x1, y1 = rng.uniform(-20, NET[1] - 20, B * rows), rng.uniform(-20, NET[0] - 20, B * rows)
        boxes = torch.from_numpy(np.stack([x1, y1, np.minimum(x1 + w, NET[1]), np.minimum(y1 + h, NET[0])], 1).astype(np.float32)).cuda()
        counts = torch.full((B,), rows, dtype=torch.int32, device='cuda')
        im_ids = torch.arange(B, device='cuda').repeat_interleave(rows)
        feats = [torch.randn((B, C, H, W), generator=gen, device='cuda').requires_grad_(True) for H, W in GRID]
        grad_out = torch.randn((B * rows, C, P, P), generator=gen, device='cuda')
        out, levels = multiscale_roi_align(feats, boxes, nets, P, g, counts=counts, return_levels=True)
        ours = lambda: torch.autograd.grad(out, feats, grad_out, retain_graph=True)
        ref_out = torch_roi_align(feats, scales, boxes, im_ids, P, g)
        theirs = lambda: torch.autograd.grad(ref_out, feats, grad_out, retain_graph=True)
        a, b = ours(), theirs()
        scale = max(float(t.abs().max()) for t in b)
        max_diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
        del a, b
        ms, runs = wall(ours, args.runs, args.warmup)
        t_ms, t_runs = wall(theirs, args.runs, args.warmup)
        stages[name] = dict(ms=ms, runs_ms=runs, torch_ms=t_ms, torch_runs_ms=t_runs, speedup_vs_torch_ops=round(t_ms / ms, 2),
                            slower_than_torch_ops=ms > t_ms, equal=max_diff <= 1e-4 * scale, max_abs_diff=max_diff, largest_gradient=scale,
                            rows=B * rows, rows_per_level=torch.bincount(levels.long(), minlength=len(GRID)).tolist(),
                            grad_out_bytes=grad_out.numel() * 4, store_GBps=round(grad_bytes / ms / 1e6, 1))
        del out, ref_out, feats, grad_out
    commit = args.commit
    if commit is None:
        r = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else None
    stamp = build.read_stamp() or {}
    total = round(sum(s['ms'] for s in stages.values()), 3)
    result = {
        'metric': 'RoIAlign backward into the feature maps: 8 x 512 rows at 7 x 7 plus 8 x 128 rows at 14 x 14, sum of the median wall times',
        'value': total, 'unit': 'ms', 'higher_is_better': False, 'torch_ms': round(sum(s['torch_ms'] for s in stages.values()), 3),
        'stages': stages, 'equal': all(s['equal'] for s in stages.values()),
        'gradient_bytes_per_call': grad_bytes, 'copy_ms': copy_ms, 'copy_GBps': round(grad_bytes / copy_ms / 1e6, 1),
        'config': {'seed': args.seed, 'frames': B, 'net': list(NET), 'levels': [list(s) for s in GRID], 'channels': C, 'sampling_ratio': g,
                   'runs': args.runs, 'warmup': args.warmup},
        'device': torch.cuda.get_device_name(0), 'commit': commit, 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Timing of the detector's proposal side (cosypose_amd.detector_rpn, csrc/kernels_detpre.hip) on one GPU: 8 frames the network saw at
800x1067, padded to 800x1088, five FPN levels (200x272 ... 13x17), A = 3 anchors per cell, C = 256 channels.  Prints one JSON line.
bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_rpn.py --out profiles/rpn_bench.json

Three stages, each the median WALL time of `--runs` calls (device work and the host's share, synchronised before and after):
rpn_proposals (pre / post_nms_top_n = 1000), then multiscale_roi_align at 7 and at 14 on its 8 x 1000 padded proposals over the first
four levels.  Each is timed in the same process against the same contract written with torch ops on the device (`torch_ms`): topk per
level, gathers from an anchor table made beforehand, decode / clip as tensor ops and the package's own batched_nms per image; for
RoIAlign a per-level gather-based bilinear over chunks of 256 boxes.  No ratio is fixed in advance: a stage that comes out slower than
the torch-ops chain says so (`slower_than_torch_ops`).  `equal`: the same number of proposals per image and the same boxes to 1e-3 px;
no RoI whose features differ by more than 2e-3: the torch route forms a sample position as start + (p + (i + 0.5) / g) bin, a few ulps
of a coordinate up to 272 (3e-5) away from the contract's, and unit-variance features change by several units per pixel."""
import argparse
import json
import math
import statistics
import time

GRID = [(200, 272), (100, 136), (50, 68), (25, 34), (13, 17)]
NET, PAD = (800, 1067), (800, 1088)


def torch_proposals(obj, dl, anchors, B, pre, post, batched_nms):
    import torch
    boxes, scores, levels = [], [], []
    for l, (o, d) in enumerate(zip(obj, dl)):
        A, H, W = o.shape[1:]
        logit = o.permute(0, 2, 3, 1).reshape(B, -1)
        rel = d.view(B, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(B, -1, 4)
        top, idx = logit.topk(min(pre, logit.shape[1]), dim=1)
        rel = rel.gather(1, idx[:, :, None].expand(-1, -1, 4))
        anc = anchors[l][idx]
        w, h = anc[..., 2] - anc[..., 0], anc[..., 3] - anc[..., 1]
        cx, cy = anc[..., 0] + 0.5 * w, anc[..., 1] + 0.5 * h
        dw, dh = rel[..., 2].clamp(max=math.log(1000 / 16)), rel[..., 3].clamp(max=math.log(1000 / 16))
        pcx, pcy, pw, ph = rel[..., 0] * w + cx, rel[..., 1] * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
        boxes.append(torch.stack([(pcx - 0.5 * pw).clamp(0, NET[1]), (pcy - 0.5 * ph).clamp(0, NET[0]),
                                  (pcx + 0.5 * pw).clamp(0, NET[1]), (pcy + 0.5 * ph).clamp(0, NET[0])], -1))
        scores.append(top); levels.append(torch.full_like(idx, l))
    boxes, scores, levels = torch.cat(boxes, 1), torch.cat(scores, 1), torch.cat(levels, 1)
    out = []
    for b in range(B):
        big = torch.nonzero(((boxes[b, :, 2] - boxes[b, :, 0]) >= 1e-3) & ((boxes[b, :, 3] - boxes[b, :, 1]) >= 1e-3)).reshape(-1)
        bx, sc, lv = boxes[b, big], scores[b, big], levels[b, big]
        out.append(bx[batched_nms(bx, sc, lv, 0.7)[:post]])
    return out


def torch_roi_align(feats, scales, boxes, im_ids, P, g, chunk=256):
    import torch
    C = feats[0].shape[1]
    s = torch.sqrt((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))
    k_min, k_max = round(-math.log2(scales[0])), round(-math.log2(scales[-1]))
    lvl = torch.floor(4 + torch.log2(s / 224 + 1e-6)).clamp(k_min, k_max).long() - k_min
    out = torch.zeros((len(boxes), C, P, P), dtype=torch.float32, device=boxes.device)
    grid = (torch.arange(P, device=boxes.device, dtype=torch.float32)[:, None]
            + (torch.arange(g, device=boxes.device, dtype=torch.float32)[None, :] + 0.5) / g).reshape(-1)          # p + (i + 0.5) / g

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
    for l, f in enumerate(feats):
        rows = torch.nonzero(lvl == l).reshape(-1)
        H, W = f.shape[2:]
        for at in range(0, len(rows), chunk):
            r = rows[at:at + chunk]
            bx, im = boxes[r], im_ids[r]
            oy, y0, y1, ly, hy = axis(bx[:, 1], bx[:, 3], scales[l], H)
            ox, x0, x1, lx, hx = axis(bx[:, 0], bx[:, 2], scales[l], W)
            fi = f.permute(0, 2, 3, 1)                                        # (B,H,W,C): one gather fetches a tap's channels
            tap = lambda yy, xx: fi[im[:, None, None], yy[:, :, None], xx[:, None, :]]                                  # (n, Pg, Pg, C)
            wgt = lambda a, b: (a[:, :, None] * b[:, None, :])[..., None]
            v = wgt(hy, hx) * tap(y0, x0) + wgt(hy, lx) * tap(y0, x1) + wgt(ly, hx) * tap(y1, x0) + wgt(ly, lx) * tap(y1, x1)
            v = v * (oy[:, :, None] & ox[:, None, :])[..., None]
            out[r] = v.reshape(len(r), P, g, P, g, C).sum((2, 4)).permute(0, 3, 1, 2) / (g * g)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build
    from cosypose_amd.detector import batched_nms
    from cosypose_amd.detector_rpn import infer_scales, multiscale_roi_align, rpn_anchors, rpn_proposals
    assert torch.cuda.is_available(), 'bench_rpn.py needs a ROCm device'
    B, C, A, pre, post = args.frames, args.channels, 3, 1000, 1000
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    obj = [torch.randn((B, A, H, W), generator=gen, device='cuda') for H, W in GRID]
    dl = [torch.randn((B, 4 * A, H, W), generator=gen, device='cuda') * 0.2 for H, W in GRID]
    feats = [torch.randn((B, C, H, W), generator=gen, device='cuda') for H, W in GRID[:4]]
    nets = [NET] * B
    table = rpn_anchors(GRID, PAD).cuda()
    first = np.cumsum([0] + [A * H * W for H, W in GRID])
    anchors = [table[first[l]:first[l + 1]] for l in range(len(GRID))]
    scales = infer_scales(GRID[:4], nets)

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

    props, counts, _ = rpn_proposals(obj, dl, nets, PAD, pre_nms_top_n=pre, post_nms_top_n=post)
    ref_props = torch_proposals(obj, dl, anchors, B, pre, post, batched_nms)
    kept = counts.cpu().tolist()
    same_counts = kept == [len(p) for p in ref_props]
    same_boxes = same_counts and all(bool(torch.allclose(props[b * post:b * post + n], ref_props[b], atol=1e-3, rtol=0)) for b, n in enumerate(kept))
    im_ids = torch.arange(B, device='cuda').repeat_interleave(post)
    stages = {}
    ms, runs = wall(lambda: rpn_proposals(obj, dl, nets, PAD, pre_nms_top_n=pre, post_nms_top_n=post), args.runs, args.warmup)
    t_ms, t_runs = wall(lambda: torch_proposals(obj, dl, anchors, B, pre, post, batched_nms), args.runs, 1)
    stages['rpn_proposals'] = dict(ms=ms, runs_ms=runs, torch_ms=t_ms, torch_runs_ms=t_runs, equal=bool(same_counts and same_boxes),
                                   proposals_per_frame=kept)
    for P in (7, 14):
        got = multiscale_roi_align(feats, props, nets, P, 2, counts=counts)
        want = torch_roi_align(feats, scales, props, im_ids, P, 2)
        valid = (torch.arange(post, device='cuda')[None, :] < counts[:, None]).reshape(-1)
        diff = (got[valid] - want[valid]).abs().reshape(int(valid.sum()), -1).max(1)[0]
        max_diff, rows_off = float(diff.max()), int((diff > 2e-3).sum())
        del got, want
        ms, runs = wall(lambda: multiscale_roi_align(feats, props, nets, P, 2, counts=counts), args.runs, args.warmup)
        t_ms, t_runs = wall(lambda: torch_roi_align(feats, scales, props, im_ids, P, 2), args.runs, 1)
        out_bytes = B * post * C * P * P * 4
        stages[f'multiscale_roi_align_{P}'] = dict(ms=ms, runs_ms=runs, torch_ms=t_ms, torch_runs_ms=t_runs, equal=rows_off == 0, max_abs_diff=max_diff,
                                                   rows_differing_more=rows_off, output_bytes=out_bytes,
                                                   write_GBps=round(out_bytes / ms / 1e6, 1))
    for s in stages.values():
        s['speedup_vs_torch_ops'] = round(s['torch_ms'] / s['ms'], 2)
        s['slower_than_torch_ops'] = s['ms'] > s['torch_ms']
    stamp = build.read_stamp() or {}
    total = round(sum(s['ms'] for s in stages.values()), 3)
    result = {
        'metric': 'detector proposal side: rpn_proposals + multiscale_roi_align(7) + multiscale_roi_align(14), sum of the median wall times',
        'value': total, 'unit': 'ms', 'higher_is_better': False, 'torch_ms': round(sum(s['torch_ms'] for s in stages.values()), 3),
        'stages': stages, 'equal': all(s['equal'] for s in stages.values()),
        'config': {'seed': args.seed, 'frames': B, 'net': list(NET), 'padded': list(PAD), 'levels': [list(g) for g in GRID], 'anchors_per_cell': A,
                   'channels': C, 'pre_nms_top_n': pre, 'post_nms_top_n': post, 'sampling_ratio': 2, 'runs': args.runs, 'warmup': args.warmup},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()

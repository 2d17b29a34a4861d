#!/usr/bin/env python3
"""Timing of the detection side (cosypose_amd.mask_ops, cosypose_amd.detection_meters, csrc/kernels_det.hip) on one GPU: 64 instance
masks of 480x640 with 20 instances each (synthetic.make_instance_masks, seed 0) and a detection scene of 64 views
(synthetic.make_det_scene).  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_det.py --warmup 3 --runs 7 --out profiles/det_bench.json

Reported, each the median over the runs of a window of `--iters` calls between two device events, all in this process:
mask_instance_stats on the batch; instance_masks for every present (image, id > 0) row; box_iou_pairs on the scene's tentative pairs;
and DetectionMeter.add on that scene as WALL time (it is host work around one launch).  In the same process, the route a user has
today with torch ops on the device: torch.unique plus a per-id min / max of nonzero, `mask == ids[:, None, None]`, and the IoU formula
in torch ops on 512-pair chunks of the full matrix with its diagonal, as the reference's DetectionMeter does it (`torch_*`, windows of
one call).  `equal`: every output of the two routes is the same (the IoUs bit for bit).  What binds each kernel is read from a kernel
trace, not from this script.
"""
import argparse
import json
import statistics
import time


def torch_stats(masks, n_ids):
    import torch
    out = torch.full((masks.shape[0], n_ids, 5), -1, dtype=torch.int32, device=masks.device)
    out[:, :, 0] = 0
    for b, mask in enumerate(masks):
        for i in torch.unique(mask).tolist():
            yx = (mask == i).nonzero()
            out[b, i] = torch.stack([torch.as_tensor(len(yx), device=masks.device), yx[:, 1].min(), yx[:, 0].min(), yx[:, 1].max(), yx[:, 0].max()]).int()
    return out


def torch_instance_masks(masks, ids_per_image):
    import torch
    return torch.cat([(mask == ids[:, None, None]).to(torch.uint8) for mask, ids in zip(masks, ids_per_image)])


def torch_iou_pairs(a, b, bsz=512):
    import torch
    out = []
    for n in range(0, len(a), bsz):
        a_, b_ = a[n:n + bsz], b[n:n + bsz]
        area_a = (a_[:, 2] - a_[:, 0]) * (a_[:, 3] - a_[:, 1])
        area_b = (b_[:, 2] - b_[:, 0]) * (b_[:, 3] - b_[:, 1])
        wh = (torch.min(a_[:, None, 2:], b_[:, 2:]) - torch.max(a_[:, None, :2], b_[:, :2])).clamp(min=0)
        inter = wh[:, :, 0] * wh[:, :, 1]
        iou = inter / (area_a[:, None] + area_b - inter)
        out.append(iou[torch.arange(len(a_)), torch.arange(len(a_))])
    return torch.cat(out) if out else a.new_zeros(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--instances', type=int, default=20)
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20, help='calls per timed window of the HIP route')
    ap.add_argument('--torch-runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import pandas as pd
    import torch
    from cosypose_amd import build
    from cosypose_amd import synthetic as syn
    from cosypose_amd.detection_meters import DetectionMeter, box_iou_pairs
    from cosypose_amd.mask_ops import instance_masks, mask_instance_stats
    from cosypose_amd.pose_meters import prepare_candidates
    from cosypose_amd.tensor_collection import PandasTensorCollection
    assert torch.cuda.is_available(), 'bench_det.py needs a ROCm device'
    B, H, W = args.batch, args.height, args.width
    masks = torch.from_numpy(syn.make_instance_masks(args.seed, B, H, W, args.instances)).cuda()
    n_ids = 256

    stats = mask_instance_stats(masks)
    present = (stats[:, 1:, 0] > 0).nonzero()                     # (image, id - 1) of every visible instance
    row_image, row_id = present[:, 0].int().contiguous(), (present[:, 1] + 1).int().contiguous()
    ids_per_image = [row_id[row_image == b].to(torch.uint8) for b in range(B)]

    scene = syn.make_det_scene(args.seed, scene_ids=(0,), n_views=args.views)
    names = np.array([f'obj_{n + 1:06d}' for n in range(int(scene['gt_label'].max()) + 1)])
    gt_infos = pd.DataFrame(dict(scene_id=scene['gt_scene_id'], view_id=scene['gt_view_id'], label=names[scene['gt_label']]))
    pred_infos = pd.DataFrame(dict(scene_id=scene['pred_scene_id'], view_id=scene['pred_view_id'], label=names[scene['pred_label']],
                                   score=scene['pred_score']))
    gt_boxes, pred_boxes = torch.from_numpy(scene['gt_bboxes']).cuda(), torch.from_numpy(scene['pred_bboxes']).cuda()
    prep = prepare_candidates(pred_infos, gt_infos)
    cand = prep['cand_infos']
    idx = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.long, device='cuda')
    pair_a = pred_boxes[idx(prep['keep_ids'])][idx(prep['filtered_ids'])][idx(cand['pred_id'].values)].contiguous()
    pair_b = gt_boxes[idx(cand['gt_id'].values)].contiguous()

    def timed(call, iters, runs, warmup):
        def window():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(iters):
                call()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) / iters
        for _ in range(warmup):
            call()
        windows = [window() for _ in range(runs)]
        return statistics.median(windows), windows

    hip = {
        'mask_instance_stats': lambda: mask_instance_stats(masks),
        'instance_masks': lambda: instance_masks(masks, row_image, row_id),
        'box_iou_pairs': lambda: box_iou_pairs(pair_a, pair_b),
    }
    via_torch = {
        'mask_instance_stats': lambda: torch_stats(masks, n_ids),
        'instance_masks': lambda: torch_instance_masks(masks, ids_per_image),
        'box_iou_pairs': lambda: torch_iou_pairs(pair_a, pair_b),
    }
    ms, runs_ms, torch_ms = {}, {}, {}
    for k, call in hip.items():
        ms[k], runs_ms[k] = timed(call, args.iters, args.runs, args.warmup)
    for k, call in via_torch.items():
        torch_ms[k], _ = timed(call, 1, args.torch_runs, 1)
    equal = {k: bool(torch.equal(hip[k](), via_torch[k]())) for k in hip if k != 'box_iou_pairs'}
    equal['box_iou_pairs'] = bool(torch.equal(hip['box_iou_pairs']().view(torch.int32), via_torch['box_iou_pairs']().view(torch.int32)))

    def meter_add():
        meter = DetectionMeter()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        meter.add(PandasTensorCollection(pred_infos.copy(), bboxes=pred_boxes), PandasTensorCollection(gt_infos.copy(), bboxes=gt_boxes))
        return 1e3 * (time.perf_counter() - t0), meter
    meter_add()
    add_runs = [meter_add()[0] for _ in range(args.runs)]
    summary = meter_add()[1].summary()[0]

    stamp = build.read_stamp() or {}
    total = sum(ms.values())
    result = {
        'metric': 'detection side: mask_instance_stats + instance_masks + box_iou_pairs (device time of one call each)', 'value': round(total, 4),
        'unit': 'ms', 'higher_is_better': False,
        'ms': {k: round(v, 4) for k, v in ms.items()}, 'runs_ms': {k: [round(r, 4) for r in v] for k, v in runs_ms.items()},
        'torch_ms': {k: round(v, 3) for k, v in torch_ms.items()}, 'speedup_vs_torch_ops': {k: round(torch_ms[k] / ms[k], 1) for k in ms},
        'equal': all(equal.values()), 'equal_per_output': equal,
        'detection_meter_add_wall_ms': round(statistics.median(add_runs), 3),
        'bytes': {'masks_read': int(masks.numel()), 'instance_masks_written': int(len(row_id)) * H * W},
        'config': {'seed': args.seed, 'batch': B, 'height': H, 'width': W, 'instances': args.instances, 'rows': int(len(row_id)), 'views': args.views,
                   'pairs': int(len(cand)), 'n_gt': int(len(gt_infos)), 'n_pred': int(len(pred_infos)), 'n_matched': int(summary['n_matched']),
                   'warmup': args.warmup, 'runs': args.runs, 'iters': args.iters, 'torch_runs': args.torch_runs},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()

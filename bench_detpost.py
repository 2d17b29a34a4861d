#!/usr/bin/env python3
"""Timing of the detector's output side (cosypose_amd.detector, csrc/kernels_detpost.hip) on one GPU: 8 frames of 480x640 that the
network saw at 800x1067, 1000 proposals each, C = 22, M = 28, logits drawn (seed 0) so that NMS leaves more than 100 boxes per frame and
the cut to detections_per_img = 100 decides.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not
affected.

    timeout -k 10 600 python bench_detpost.py --out profiles/detpost_bench.json

Reported: the median WALL time of `--runs` detections_from_heads(output_masks=True) calls (device work, the one device-to-host copy and
the host's table included; the mask head is a lookup into logits made beforehand), and in the same process the same contract written
with torch ops on the device (`torch_ms`): softmax / decode / clip as tensor ops, per image the IoU matrix of the shifted candidates,
copied to the host and scanned greedily there (what torchvision's device NMS does), then per detection F.interpolate of the padded
probabilities, a float (n,1,H,W) paste and `>`.  `equal`: the kept (image, proposal, label) sets and labels are the same, the boxes
agree to 4 float32 ulps (the two sides differ in their exp only), the masks agree on every pixel whose torch value is not within 1e-5 of
mask_th.  Rows are matched by (image, candidate): the two softmaxes round differently, so two scores a few ulps apart may swap places
(`rows_in_another_place`, with the largest score gap of such a pair).  `paste`: the paste kernel alone between two device events, and its write rate against the bool output's bytes (D H W).
"""
import argparse
import json
import statistics
import time


def make_case(seed, B, R, C, M, net, dpi):
    import numpy as np
    rng = np.random.RandomState(seed)
    net_h, net_w = net
    n = B * R
    logits = rng.normal(0, 1, (n, C)).astype(np.float32)
    logits[:, 0] += 6
    hot = rng.rand(n) < 0.4
    logits[np.flatnonzero(hot), rng.randint(1, C, int(hot.sum()))] += rng.normal(8, 2, int(hot.sum())).astype(np.float32)
    reg = (rng.normal(0, 1, (n, C, 4)) * np.array([1, 1, 0.5, 0.5])).astype(np.float32).reshape(n, 4 * C)
    w, h = rng.uniform(30, 220, n), rng.uniform(30, 220, n)
    x1, y1 = rng.uniform(0, net_w - w), rng.uniform(0, net_h - h)
    props = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    y, x = np.meshgrid(np.linspace(-1, 1, M), np.linspace(-1, 1, M), indexing='ij')
    centre, radius = rng.uniform(-0.3, 0.3, (B * dpi, C, 2)), rng.uniform(0.45, 0.8, (B * dpi, C))
    mask_logits = 6 * (1 - ((x - centre[..., 0, None, None]) ** 2 + (y - centre[..., 1, None, None]) ** 2) / radius[..., None, None] ** 2) + 0.37
    return logits, reg, props, mask_logits.astype(np.float32)


def torch_boxes(logits, reg, props, counts, net, frame, score_thresh, nms_thresh, dpi):
    """steps 1-6 of DESIGN.md section 21 in torch ops on the device"""
    import math
    import numpy as np
    import torch
    import torch.nn.functional as F
    C = logits.shape[1]
    scores = F.softmax(logits, -1)
    rel = reg.reshape(len(props), C, 4)
    w, h = props[:, 2] - props[:, 0], props[:, 3] - props[:, 1]
    cx, cy = props[:, 0] + 0.5 * w, props[:, 1] + 0.5 * h
    dw, dh = torch.clamp(rel[:, :, 2] / 5, max=math.log(1000 / 16)), torch.clamp(rel[:, :, 3] / 5, max=math.log(1000 / 16))
    pcx, pcy = rel[:, :, 0] / 10 * w[:, None] + cx[:, None], rel[:, :, 1] / 10 * h[:, None] + cy[:, None]
    pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
    boxes = torch.stack([(pcx - 0.5 * pw).clamp(0, net[1]), (pcy - 0.5 * ph).clamp(0, net[0]),
                         (pcx + 0.5 * pw).clamp(0, net[1]), (pcy + 0.5 * ph).clamp(0, net[0])], -1)
    ratio = torch.tensor([np.float32(frame[1]) / np.float32(net[1]), np.float32(frame[0]) / np.float32(net[0])] * 2, device=boxes.device)
    out_boxes, out_labels, out_src, out_im, first = [], [], [], [], 0
    for b, R in enumerate(counts):
        bx, sc = boxes[first:first + R, 1:].reshape(-1, 4), scores[first:first + R, 1:].reshape(-1)
        first += R
        label = torch.arange(1, C, device=bx.device).repeat(R)
        cand = torch.nonzero((sc > score_thresh) & ((bx[:, 2] - bx[:, 0]) >= 1e-2) & ((bx[:, 3] - bx[:, 1]) >= 1e-2)).reshape(-1)
        bx, sc, label = bx[cand], sc[cand], label[cand]
        order = torch.sort(sc, descending=True, stable=True)[1]
        s = (bx + (label.to(bx) * (bx.max() + 1))[:, None])[order]
        area = (s[:, 2] - s[:, 0]) * (s[:, 3] - s[:, 1])
        wh = (torch.min(s[:, None, 2:], s[:, 2:]) - torch.max(s[:, None, :2], s[:, :2])).clamp(min=0)
        inter = wh[:, :, 0] * wh[:, :, 1]
        over = (inter / ((area[:, None] + area) - inter) > nms_thresh).cpu().numpy()
        removed, keep = np.zeros(len(over), bool), []
        for i in range(len(over)):
            if not removed[i]:
                keep.append(i)
                if len(keep) == dpi:
                    break
                removed |= over[i]
        keep = order[torch.as_tensor(keep, dtype=torch.int64, device=bx.device)]
        out_boxes.append(bx[keep] * ratio); out_labels.append(label[keep]); out_src.append(cand[keep])
        out_im.append(torch.full((len(keep),), b, dtype=torch.int64, device=bx.device))
    return dict(boxes=torch.cat(out_boxes), labels=torch.cat(out_labels), src=torch.cat(out_src), im=torch.cat(out_im))


def torch_masks(boxes_f, labels, mask_logits, frame, mask_th):
    """step 8 in torch ops on the device: mask_logits[d] belongs to detection d"""
    import torch
    import torch.nn.functional as F
    M = mask_logits.shape[-1]
    D, (H, W) = len(labels), frame
    prob = F.pad(torch.sigmoid(mask_logits[:D][torch.arange(D, device=labels.device), labels]), (1, 1, 1, 1))
    scale = torch.tensor(M + 2, dtype=torch.float32) / torch.tensor(M, dtype=torch.float32)
    xc, yc = (boxes_f[:, 2] + boxes_f[:, 0]) * 0.5, (boxes_f[:, 3] + boxes_f[:, 1]) * 0.5
    hw_, hh_ = (boxes_f[:, 2] - boxes_f[:, 0]) * 0.5 * scale.item(), (boxes_f[:, 3] - boxes_f[:, 1]) * 0.5 * scale.item()
    ib = torch.stack([xc - hw_, yc - hh_, xc + hw_, yc + hh_], 1).to(torch.int64).cpu().numpy()
    pasted = torch.zeros((D, 1, H, W), dtype=torch.float32, device=labels.device)
    for d in range(D):
        bx1, by1, bx2, by2 = (int(v) for v in ib[d])
        w_, h_ = max(bx2 - bx1 + 1, 1), max(by2 - by1 + 1, 1)
        x0, x1, y0, y1 = max(bx1, 0), min(bx2 + 1, W), max(by1, 0), min(by2 + 1, H)
        if x0 < x1 and y0 < y1:
            up = F.interpolate(prob[d][None, None], size=(h_, w_), mode='bilinear', align_corners=False)[0, 0]
            pasted[d, 0, y0:y1, x0:x1] = up[y0 - by1:y1 - by1, x0 - bx1:x1 - bx1]
    return pasted[:, 0] > mask_th, pasted[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--proposals', type=int, default=1000)
    ap.add_argument('--classes', type=int, default=22)
    ap.add_argument('--mask-side', type=int, default=28)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--paste-iters', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build
    from cosypose_amd.detector import detections_from_heads, paste_masks, postprocess_detections
    assert torch.cuda.is_available(), 'bench_detpost.py needs a ROCm device'
    B, R, C, M, dpi = args.frames, args.proposals, args.classes, args.mask_side, 100
    net, frame, mask_th = (800, 1067), (480, 640), 0.8
    logits, reg, props, mask_logits = (torch.from_numpy(a).cuda() for a in make_case(args.seed, B, R, C, M, net, dpi))
    counts = [R] * B
    names = {c: f'obj_{c:06d}' for c in range(1, C)}
    mask_head = lambda boxes_net, batch_im_id: mask_logits[:len(boxes_net)]

    def ours():
        return detections_from_heads(logits, reg, props, [net] * B, [frame] * B, names, mask_head=mask_head, output_masks=True, counts=counts,
                                     detections_per_img=dpi, mask_th=mask_th)

    def theirs():
        r = torch_boxes(logits, reg, props, counts, net, frame, 0.05, 0.5, dpi)
        return r, torch_masks(r['boxes'], r['labels'], mask_logits, frame, mask_th)

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
        return statistics.median(out), out

    ms, runs_ms = wall(ours, args.runs, args.warmup)
    torch_ms, torch_runs_ms = wall(theirs, args.runs, 1)
    got, ref = ours(), theirs()[0]
    boxes, scores, labels, im_ids, src = postprocess_detections(logits, reg, props, [net] * B, [frame] * B, counts=counts, detections_per_img=dpi,
                                                                return_source=True)
    D = len(labels)
    per_frame = np.bincount(im_ids.cpu().numpy(), minlength=B).tolist()
    # the two routes round their softmaxes differently, so two scores a few ulps apart may swap places: rows are matched by (image,
    # candidate) and the order is reported on its own; the torch route's masks are made from the logits of the rows they are matched with
    key, ref_key = (im_ids << 21 | src).cpu().numpy(), (ref['im'] << 21 | ref['src']).cpu().numpy()
    same_sets = D == len(ref_key) and bool(np.array_equal(np.sort(key), np.sort(ref_key)))
    equal = {'kept': same_sets}
    if same_sets:
        by_key = np.argsort(key)
        match = torch.as_tensor(by_key[np.searchsorted(key[by_key], ref_key)]).cuda()          # the row of ours for every row of theirs
        ref_masks, ref_values = torch_masks(ref['boxes'], ref['labels'], mask_logits[match], frame, mask_th)
        mag = torch.maximum(ref['boxes'][:, [2, 3, 2, 3]].abs(), ref['boxes'][:, [0, 1, 0, 1]].abs()).cpu().numpy()
        box_ulps = float((np.abs(got.bboxes[match].cpu().numpy().astype(np.float64) - ref['boxes'].cpu().numpy())
                          / np.spacing(np.maximum(mag, np.float32(1e-30)))).max())
        differ = got.masks[match] != ref_masks
        near = (ref_values - mask_th).abs() <= 1e-5
        score_gap = (scores[match] - scores).abs().max().item()
        equal.update(labels=bool(torch.equal(labels[match], ref['labels'])), boxes=box_ulps <= 4, masks=int((differ & ~near).sum()) == 0)
        detail = {'boxes_max_ulps': round(box_ulps, 3), 'mask_pixels_differing': int(differ.sum()), 'mask_pixels_within_1e-5_of_th': int(near.sum()),
                  'rows_in_another_place': int((match.cpu().numpy() != np.arange(D)).sum()), 'largest_score_gap_of_a_swapped_row': score_gap}
    else:
        detail = {'rows': [D, len(ref_key)]}

    sel_labels = labels.to(torch.int32)
    out = torch.empty((D,) + frame, dtype=torch.bool, device='cuda')
    for _ in range(3):
        paste_masks(mask_logits[:D], boxes, sel_labels, frame, mask_th, out=out)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    windows = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.paste_iters):
            paste_masks(mask_logits[:D], boxes, sel_labels, frame, mask_th, out=out)
        end.record()
        torch.cuda.synchronize()
        windows.append(start.elapsed_time(end) / args.paste_iters)
    paste_ms = statistics.median(windows)

    stamp = build.read_stamp() or {}
    result = {
        'metric': 'detector output side: detections_from_heads(output_masks=True), wall time of one call', 'value': round(ms, 3), 'unit': 'ms',
        'higher_is_better': False, 'runs_ms': [round(v, 3) for v in runs_ms],
        'torch_ms': round(torch_ms, 3), 'torch_runs_ms': [round(v, 3) for v in torch_runs_ms], 'speedup_vs_torch_ops': round(torch_ms / ms, 1),
        'equal': all(equal.values()), 'equal_per_output': equal, 'equal_detail': detail,
        'paste': {'ms': round(paste_ms, 4), 'bytes_written': D * frame[0] * frame[1], 'write_GBps': round(D * frame[0] * frame[1] / paste_ms / 1e6, 1)},
        'config': {'seed': args.seed, 'frames': B, 'proposals': R, 'classes': C, 'mask_side': M, 'net': list(net), 'frame': list(frame),
                   'detections': D, 'detections_per_frame': per_frame, 'runs': args.runs, 'warmup': args.warmup, 'paste_iters': args.paste_iters},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()

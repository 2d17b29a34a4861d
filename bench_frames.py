#!/usr/bin/env python3
"""Timing of the frames' own resize (cosypose_amd.frames.resize_frames, csrc/kernels_frames.hip) on one GPU: one call on a list of 64
RGB frames with their instance masks -- a seeded half-and-half mix of 540x720 (T-LESS Primesense) and 960x1280 (ITODD) -- brought to
480x640 with boxes=True, as CropResizeToAspectAugmentation(resize=(640, 480)) brings every frame of the reference's datasets to the
training size.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_frames.py --warmup 3 --runs 7 --out profiles/frames_bench.json

Reported: milliseconds per resize_frames call (median over the runs of a window of `--iters` calls between two device events, all in
this process; a call includes building and uploading its descriptor table, and the mask statistics) and per frame; the bytes the call
has to move at least (images and masks read, images and masks written, the masks read once more for the statistics) over that time; and
two baselines on the same frames in the same process:
  torch_device_ms   the reference's chain in torch device ops, the frames of one size stacked into one batch: .float() / 255,
                    F.interpolate(bilinear, align_corners=False), * 255 -> uint8; the mask through .float(), F.interpolate(nearest),
                    -> uint8; mask_instance_stats on the result (the same call as in resize_frames);
  cpu_ms_per_frame_one_core   the reference's chain frame by frame with torch on ONE core (torch.set_num_threads(1)), without the boxes.
`differs_from_torch_device` / `differs_from_cpu_one_core` count the image bytes (of all) where the call's output is not the baseline's,
with the largest difference: DESIGN.md section 18 says why a few must differ.  Which launch binds is read from a kernel trace, not from
this script.
"""
import argparse
import json
import statistics
import time

SIZES = ((540, 720), (960, 1280))            # (h, w)


def make_inputs(seed, n):
    import numpy as np
    rs = np.random.RandomState(seed)
    kinds = rs.permutation(n) % len(SIZES)   # half and half, in a seeded order
    images, masks = [], []
    for b in range(n):                       # gradients, a textured half and noise: neither flat nor white noise
        h, w = SIZES[kinds[b]]
        y, x = np.mgrid[0:h, 0:w]
        base = np.stack([(x * (b + 1)) % 256, (y * 2 + b * 7) % 256, ((x + y) // 2 + 31 * b) % 256]).astype(np.int32)
        base[:, :, w // 2:] += rs.randint(-30, 31, (3, h, w - w // 2))
        images.append(np.clip(base, 0, 255).astype(np.uint8))
        m = np.zeros((h, w), np.uint8)
        for i in range(1, 9):
            hh, ww = rs.randint(h // 8, h // 2), rs.randint(w // 8, w // 2)
            y0, x0 = rs.randint(0, h - hh), rs.randint(0, w - ww)
            m[y0:y0 + hh, x0:x0 + ww] = i
        masks.append(m)
    return images, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20, help='calls per timed window')
    ap.add_argument('--no-cpu', action='store_true', help='skip the one-core baseline')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    from cosypose_amd import build
    from cosypose_amd.frames import resize_frames
    from cosypose_amd.mask_ops import mask_instance_stats
    assert torch.cuda.is_available(), 'bench_frames.py needs a ROCm device'
    B, (H, W) = args.batch, (480, 640)
    images, masks = make_inputs(args.seed, B)
    images_d = [torch.from_numpy(im).cuda() for im in images]
    masks_d = [torch.from_numpy(m).cuda() for m in masks]
    out_d = torch.empty(B, 3, H, W, dtype=torch.uint8, device='cuda')
    out_masks_d = torch.empty(B, H, W, dtype=torch.uint8, device='cuda')
    call = lambda: resize_frames(images_d, (W, H), masks=masks_d, boxes=True, out=out_d, out_masks=out_masks_d)

    groups = {s: [b for b in range(B) if images[b].shape[1:] == s] for s in SIZES}
    stacked = {s: (torch.stack([images_d[b] for b in idx]), torch.stack([masks_d[b] for b in idx])) for s, idx in groups.items() if idx}
    ref_d, ref_masks_d = torch.empty_like(out_d), torch.empty_like(out_masks_d)

    def torch_chain():
        for s, (im, m) in stacked.items():
            idx = groups[s]
            x = F.interpolate(im.float() / 255, size=(H, W), mode='bilinear', align_corners=False)
            ref_d[idx] = (x * 255).to(torch.uint8)
            ref_masks_d[idx] = F.interpolate(m.unsqueeze(1).float(), size=(H, W), mode='nearest')[:, 0].to(torch.uint8)
        return mask_instance_stats(ref_masks_d)

    def window(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / args.iters

    def differs(got, want):
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        return {'bytes': int((d != 0).sum()), 'of': int(d.size), 'largest': int(d.max())}

    timings = {}
    for name, fn in (('call', call), ('torch', torch_chain)):
        for _ in range(args.warmup):
            fn()
        timings[name] = [window(fn) for _ in range(args.runs)]
    ms, torch_ms = statistics.median(timings['call']), statistics.median(timings['torch'])
    res = call()
    got, got_masks = out_d.cpu().numpy(), out_masks_d.cpu().numpy()
    stats_equal = bool(torch.equal(res.stats, torch_chain()))
    vs_torch = differs(got, ref_d.cpu().numpy())
    masks_equal_torch = bool(np.array_equal(got_masks, ref_masks_d.cpu().numpy()))

    min_bytes = sum(4 * h * w + 4 * H * W + H * W for _, h, w in (im.shape for im in images))

    cpu_ms_per_frame = vs_cpu = masks_equal_cpu = None
    if not args.no_cpu:
        threads = torch.get_num_threads()
        torch.set_num_threads(1)

        def cpu_chain(im, m):                 # augmentations.py:152-153, 176-177, 188-189 on an (h,w,3) frame
            x = (torch.as_tensor(im).float() / 255).unsqueeze(0).permute(0, 3, 1, 2)
            mm = torch.as_tensor(m).unsqueeze(0).unsqueeze(0).float()
            x = F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False)
            mm = F.interpolate(mm, size=(H, W), mode='nearest')
            return (x[0].permute(1, 2, 0) * 255).to(torch.uint8), mm[0, 0].to(torch.uint8)
        hwc = [np.ascontiguousarray(im.transpose(1, 2, 0)) for im in images]
        cpu_chain(hwc[0], masks[0])
        t0 = time.perf_counter()
        ref = [cpu_chain(im, m) for im, m in zip(hwc, masks)]
        cpu_ms_per_frame = 1e3 * (time.perf_counter() - t0) / B
        torch.set_num_threads(threads)
        vs_cpu = differs(got, np.stack([r[0].numpy().transpose(2, 0, 1) for r in ref]))
        masks_equal_cpu = bool(all(np.array_equal(r[1].numpy(), g) for r, g in zip(ref, got_masks)))
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'frames to the training size, frames.resize_frames (one call, one list of frames with masks, boxes=True)', 'value': round(ms, 4),
        'unit': 'ms/call', 'higher_is_better': False, 'runs_ms': [round(r, 4) for r in timings['call']], 'ms_per_frame': round(ms / B, 5),
        'frames_per_s': round(B / (ms * 1e-3), 1), 'min_bytes_moved': int(min_bytes), 'min_bytes_per_s': round(min_bytes / (ms * 1e-3), 1),
        'torch_device_ms': round(torch_ms, 4), 'torch_device_runs_ms': [round(r, 4) for r in timings['torch']],
        'speedup_vs_torch_device': round(torch_ms / ms, 2),
        'cpu_ms_per_frame_one_core': None if cpu_ms_per_frame is None else round(cpu_ms_per_frame, 3),
        'speedup_vs_cpu_one_core': None if cpu_ms_per_frame is None else round(cpu_ms_per_frame / (ms / B), 1),
        'differs_from_torch_device': vs_torch, 'differs_from_cpu_one_core': vs_cpu, 'masks_equal_torch_device': masks_equal_torch,
        'masks_equal_cpu_one_core': masks_equal_cpu, 'stats_equal_torch_device': stats_equal,
        'config': {'seed': args.seed, 'batch': B, 'height': H, 'width': W, 'warmup': args.warmup, 'runs': args.runs, 'iters': args.iters,
                   'sizes': {f'{h}x{w}': len(idx) for (h, w), idx in groups.items()}},
        'torch_version': torch.__version__, 'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()

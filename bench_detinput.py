#!/usr/bin/env python3
"""Timing of the detector's input side (cosypose_amd.detector_input, csrc/kernels_detin.hip) on one GPU.  Prints one
JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_detinput.py --out profiles/detinput_bench.json

Two cases, each on 8 HWC uint8 frames of 480 x 640:
  reference_480_640    min_size 480, max_size 640, the reference's configuration: the network sees the frames at their own size (the one-tap
                       path), no targets;
  torchvision_800_1333 torchvision's defaults: 800 x 1066 (torch 1.3's floor of 1066.67) padded to 800 x 1088, with 20 masks and 20 boxes
                       per frame.
Reported per case: the median WALL time of `--calls` detector_input calls after `--warmup` warm-up calls, each from the Python call to the
end of torch.cuda.synchronize() -- so the host share (sizes, tables, the upload of the descriptors) is in it; the same for the same
contract in torch ops on the device in the same process (per frame: permute, float(), / 255, - mean, / std, F.interpolate(size=) bilinear,
a copy into the batch, which is kept between calls and zeroed by each; per frame's masks: float(), F.interpolate(size=) nearest, byte();
boxes times a ratio tensor made once, outside the timed calls); the bytes the call has to move at least (frames and masks read, batch and
masks written) over its time, beside a device copy of the batch's size timed the same way (its bytes: read + written).
`largest_difference_from_torch` compares the two results: the device's own interpolate is within section 25's bound of the contract, not
bit-equal.  No ratio is fixed in advance.
The split of a call, per case: `host_ms`, the median time until detector_input returns to Python with an idle device (sizes, tables, the
upload, the enqueue), and `back_to_back_ms`, the time per call of `--window` calls in a row between two device events (median of
`--calls` windows): where it lies above host_ms the device binds and it is the device's time per call, otherwise the host binds and the
kernel hides behind the next call's Python.  For the case with targets the same window without the masks and without any target, which
brackets the mask planes' share.  Not measured here: kernel times from a trace, other batch sizes, frames that are not contiguous HWC.
"""
import argparse
import json
import statistics
import time

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = (('reference_480_640', 480, 640, 0), ('torchvision_800_1333', 800, 1333, 20))


def make_frames(seed, n, h=480, w=640):
    import numpy as np
    rs = np.random.RandomState(seed)
    frames = []
    for b in range(n):                       # gradients, a textured half and noise: neither flat nor white noise
        y, x = np.mgrid[0:h, 0:w]
        base = np.stack([(x * (b + 1)) % 256, (y * 2 + b * 7) % 256, ((x + y) // 2 + 31 * b) % 256], axis=-1).astype(np.int32)
        base[:, w // 2:] += rs.randint(-30, 31, (h, w - w // 2, 3))
        frames.append(np.clip(base, 0, 255).astype(np.uint8))
    return frames


def make_targets(seed, n, G, h=480, w=640):
    import numpy as np
    rs = np.random.RandomState(seed + 1)
    out = []
    for _ in range(n):
        boxes, masks = np.zeros((G, 4), np.float32), np.zeros((G, h, w), np.uint8)
        for g in range(G):
            hh, ww = rs.randint(h // 8, h // 2), rs.randint(w // 8, w // 2)
            y0, x0 = rs.randint(0, h - hh), rs.randint(0, w - ww)
            masks[g, y0:y0 + hh, x0:x0 + ww] = 1
            boxes[g] = (x0, y0, x0 + ww, y0 + hh)
        out.append((boxes, masks))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--window', type=int, default=20, help='calls in a row between two device events')
    ap.add_argument('--parent', default=None, help='the commit this was measured on top of, recorded in the result')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    from cosypose_amd import build
    from cosypose_amd import detector_input as di
    assert torch.cuda.is_available(), 'bench_detinput.py needs a ROCm device'
    B = args.batch
    frames = [torch.from_numpy(f).cuda() for f in make_frames(args.seed, B)]
    mean_d, std_d = (torch.tensor(v, dtype=torch.float32, device='cuda')[:, None, None] for v in (MEAN, STD))

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(times), [round(t, 4) for t in times]

    def split(fn):
        """-> (host_ms: median time until fn returns with an idle device, back_to_back_ms: per call of a window between device events)"""
        for _ in range(args.warmup):
            fn()
        host_times = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            host_times.append(1e3 * (time.perf_counter() - t0))
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        windows = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            start.record()
            for _ in range(args.window):
                fn()
            end.record()
            torch.cuda.synchronize()
            windows.append(start.elapsed_time(end) / args.window)
        return round(statistics.median(host_times), 4), round(statistics.median(windows), 4)

    cases = {}
    for name, lo, hi, G in CASES:
        targets = None
        if G:
            targets = [dict(boxes=torch.from_numpy(b).cuda(), masks=torch.from_numpy(m).cuda()) for b, m in make_targets(args.seed, B, G)]
        nets = [di.network_size(480, 640, lo, hi)] * B
        Hp, Wp = di.padded_size(nets, 32)
        out = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device='cuda')

        def call():
            return di.detector_input(frames, targets, min_size=lo, max_size=hi, out=out)

        batch = torch.empty_like(out)                        # kept between calls, as `out` is; each call zeroes it
        ratios = [torch.tensor([rw, rh, rw, rh], dtype=torch.float32, device='cuda') for rw, rh in (di.box_ratios(480, 640, *s) for s in nets)]

        def torch_chain():
            batch.zero_()
            new = None if targets is None else []
            for i, f in enumerate(frames):
                nh, nw = nets[i]
                x = (f.permute(2, 0, 1).float() / 255 - mean_d) / std_d
                batch[i, :, :nh, :nw].copy_(F.interpolate(x[None], size=(nh, nw), mode='bilinear', align_corners=False)[0])
                if targets is not None:
                    new.append(dict(boxes=targets[i]['boxes'] * ratios[i], masks=F.interpolate(targets[i]['masks'][None].float(), size=(nh, nw))[0].byte()))
            return batch, new

        ms, runs = wall(call)
        torch_ms, torch_runs = wall(torch_chain)
        src = torch.empty_like(out)
        copy_ms, copy_runs = wall(lambda: src.copy_(out))
        host_ms, back_to_back_ms = split(call)
        without = {}
        if targets is not None:
            boxes_only = [dict(boxes=t['boxes']) for t in targets]
            without['back_to_back_ms_without_masks'] = split(lambda: di.detector_input(frames, boxes_only, min_size=lo, max_size=hi, out=out))[1]
            without['back_to_back_ms_without_targets'] = split(lambda: di.detector_input(frames, None, min_size=lo, max_size=hi, out=out))[1]
        got = call()
        want, want_targets = torch_chain()
        diff = float((got.images - want).abs().max())
        masks_equal = boxes_equal = None
        if targets is not None:
            masks_equal = all(bool(torch.equal(g['masks'], w['masks'])) for g, w in zip(got.targets, want_targets))
            boxes_equal = all(bool(torch.equal(g['boxes'], w['boxes'])) for g, w in zip(got.targets, want_targets))
        nh, nw = nets[0]
        min_bytes = B * (3 * 480 * 640 + 4 * 3 * Hp * Wp + G * (480 * 640 + nh * nw))
        cases[name] = {
            'min_size': lo, 'max_size': hi, 'net_size': [nh, nw], 'padded_size': [Hp, Wp], 'masks_per_frame': G, 'ms_per_call': round(ms, 4),
            'runs_ms': runs, 'ms_per_frame': round(ms / B, 5), 'torch_device_ms': round(torch_ms, 4), 'torch_device_runs_ms': torch_runs,
            'torch_device_over_call': round(torch_ms / ms, 2), 'min_bytes_moved': int(min_bytes), 'min_bytes_per_s': round(min_bytes / (ms * 1e-3), 1),
            'device_copy_ms': round(copy_ms, 4), 'device_copy_runs_ms': copy_runs, 'device_copy_bytes_per_s': round(2 * out.numel() * 4 / (copy_ms * 1e-3), 1),
            'largest_difference_from_torch': diff, 'masks_equal_torch': masks_equal, 'boxes_equal_torch': boxes_equal,
            'host_ms': host_ms, 'back_to_back_ms': back_to_back_ms, **without,
        }
        del out, src, want, got, targets, batch
        torch.cuda.empty_cache()
    stamp = build.read_stamp() or {}
    first = cases[CASES[0][0]]
    result = {
        'metric': 'detector input side, detector_input (one call, 8 HWC frames of 480x640 at 480/640), wall time with the host share',
        'value': first['ms_per_call'], 'unit': 'ms/call', 'higher_is_better': False, 'cases': cases,
        'config': {'seed': args.seed, 'batch': B, 'warmup': args.warmup, 'calls': args.calls, 'window': args.window, 'frames': 'HWC uint8 480x640'},
        'date': time.strftime('%Y-%m-%d'), 'parent_commit': args.parent, 'torch_version': torch.__version__,
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
        'not_measured': 'kernel times from a trace (host_ms and back_to_back_ms bracket the split), other batch sizes, frames that are not contiguous HWC',
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Timing of the image resize (cosypose_amd.resize.resize_images, csrc/kernels_resize.hip) on one GPU: one call on a list of 64 RGB images
of VOC-like sizes -- a seeded mix of 500x375, 500x333, 375x500 and 334x500 (width x height) -- resized to 480x640 with bicubic, as
BackgroundAugmentation resizes its backgrounds.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not
affected.

    timeout -k 10 600 python bench_resize.py --warmup 3 --runs 7 --out profiles/resize_bench.json

Reported: milliseconds per resize_images call (median over the runs of a window of `--iters` calls between two device events, all in this
process; a call includes building and uploading its descriptor table) and per frame; the bytes the two launches have to move at least
(sources read, the row pass written and read, the output written) over that time; and, where PIL can be imported, the same images through
Pillow's own Image.resize on ONE core of this machine (`pillow_ms_per_frame_one_core`, else null), with `pillow_equal`: the device's bytes
are Pillow's on every frame.  Which launch binds is read from a kernel trace, not from this script.
"""
import argparse
import json
import statistics
import time

SIZES = ((375, 500), (333, 500), (500, 375), (500, 334))     # (h, w)


def make_inputs(seed, n):
    import numpy as np
    rs = np.random.RandomState(seed)
    images = []
    for b in range(n):                       # gradients, a textured half and noise: neither flat nor white noise
        h, w = SIZES[rs.randint(len(SIZES))]
        y, x = np.mgrid[0:h, 0:w]
        base = np.stack([(x * (b + 1)) % 256, (y * 2 + b * 7) % 256, ((x + y) // 2 + 31 * b) % 256]).astype(np.int32)
        base[:, :, w // 2:] += rs.randint(-30, 31, (3, h, w - w // 2))
        images.append(np.clip(base, 0, 255).astype(np.uint8))
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--resample', default='bicubic', choices=('bicubic', 'bilinear'))
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20, help='resize_images calls per timed window')
    ap.add_argument('--no-pillow', action='store_true')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build
    from cosypose_amd.resize import resize_images
    assert torch.cuda.is_available(), 'bench_resize.py needs a ROCm device'
    B, H, W = args.batch, args.height, args.width
    images = make_inputs(args.seed, B)
    images_d = [torch.from_numpy(im).cuda() for im in images]
    out_d = torch.empty(B, 3, H, W, dtype=torch.uint8, device='cuda')
    call = lambda: resize_images(images_d, (H, W), args.resample, out=out_d)

    def window():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.iters):
            call()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / args.iters

    for _ in range(args.warmup):
        call()
    runs = [window() for _ in range(args.runs)]
    ms = statistics.median(runs)
    got = out_d.cpu().numpy()

    # sources read; where both axes change, the row pass (h x W) written and read; the output written
    min_bytes = sum(3 * (h * w + (2 * h * W if (h != H and w != W) else 0) + H * W) for _, h, w in (im.shape for im in images))

    pillow_equal = pillow_ms_per_frame = None
    try:
        import PIL
        have_pil = not args.no_pillow
    except ImportError:
        have_pil = False
    if have_pil:
        from PIL import Image
        filt = Image.BICUBIC if args.resample == 'bicubic' else Image.BILINEAR
        torch.set_num_threads(1)
        pils = [Image.fromarray(np.ascontiguousarray(im.transpose(1, 2, 0))) for im in images]
        pils[0].resize((W, H), filt)
        t0 = time.perf_counter()
        ref = [p.resize((W, H), filt) for p in pils]
        dt = time.perf_counter() - t0
        pillow_ms_per_frame = 1e3 * dt / B
        pillow_equal = bool(all(np.array_equal(np.asarray(r).transpose(2, 0, 1), g) for r, g in zip(ref, got)))
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'image resize, resize.resize_images (one call, one list of images)', 'value': round(ms, 4), 'unit': 'ms/call', 'higher_is_better': False,
        'runs_ms': [round(r, 4) for r in runs], 'ms_per_frame': round(ms / B, 5), 'frames_per_s': round(B / (ms * 1e-3), 1),
        'min_bytes_moved': int(min_bytes), 'min_bytes_per_s': round(min_bytes / (ms * 1e-3), 1),
        'pillow_ms_per_frame_one_core': None if pillow_ms_per_frame is None else round(pillow_ms_per_frame, 3),
        'pillow_version': PIL.__version__ if have_pil else None, 'pillow_equal': pillow_equal,
        'speedup_vs_pillow_one_core': None if pillow_ms_per_frame is None else round(pillow_ms_per_frame / (ms / B), 1),
        'config': {'seed': args.seed, 'batch': B, 'height': H, 'width': W, 'resample': args.resample, 'warmup': args.warmup, 'runs': args.runs,
                   'iters': args.iters, 'sizes': {f'{w}x{h}': int(sum(im.shape[1:] == (h, w) for im in images)) for h, w in SIZES}},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()

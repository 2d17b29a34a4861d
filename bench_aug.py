#!/usr/bin/env python3
"""Timing of the training augmentations (cosypose_amd.augmentations.augment_batch, csrc/kernels_aug.hip) on one GPU: one collated batch of
64 frames of 480x640 uint8, parameter records drawn with seed 0 as a dataset with background, rgb and gray augmentation all enabled would
draw them, 8 backgrounds at frame size.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_aug.py --warmup 3 --runs 7 --out profiles/aug_bench.json

Reported: milliseconds per augment_batch call (median over the runs of a window of `--iters` calls between two device events, all in this
process) and frames per second; the bytes the three launches have to move at least (images, masks and pasted backgrounds read, two
intermediate batches written and read, the output written) over that time; and, where PIL can be imported, the same frames and records
through Pillow's own GaussianBlur / ImageEnhance on ONE core of this machine (`pillow_frames_per_s`, else null), with `pillow_equal`: the
device's bytes are Pillow's on every frame.  Which launch binds is read from a kernel trace, not from this script.
"""
import argparse
import json
import random
import statistics
import time


def make_inputs(seed, B, H, W, n_bg):
    import numpy as np
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    images = np.empty((B, 3, H, W), np.uint8)
    for b in range(B):                       # gradients, a textured half and noise: neither flat nor white noise
        base = np.stack([(x * (b + 1)) % 256, (y * 2 + b * 7) % 256, ((x + y) // 2 + 31 * b) % 256]).astype(np.int32)
        base[:, :, W // 2:] += rs.randint(-30, 31, (3, H, W - W // 2))
        images[b] = np.clip(base, 0, 255)
    masks = np.zeros((B, H, W), np.uint8)
    masks[:, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1
    backgrounds = rs.randint(0, 256, (n_bg, 3, H // 8, W // 8)).astype(np.uint8).repeat(8, axis=2).repeat(8, axis=3)[:, :, :H, :W]
    return images, masks, np.ascontiguousarray(backgrounds)


def pillow_chain(image, rec, mask, backgrounds):
    """one frame through Pillow as PoseDataset.get_data sends it (this package's own restatement of the call sequence; nothing is read
    from the reference)"""
    import numpy as np
    from PIL import Image, ImageEnhance, ImageFilter
    im = np.ascontiguousarray(image.transpose(1, 2, 0))
    if rec['bg'] >= 0:
        bg = backgrounds[rec['bg']].transpose(1, 2, 0)
        im = im.copy()
        im[mask == 0] = bg[mask == 0]
    if rec['gate']:
        pil = Image.fromarray(im).filter(ImageFilter.GaussianBlur(rec['k']))
        for name, enhancer in (('sharpness', ImageEnhance.Sharpness), ('contrast', ImageEnhance.Contrast), ('brightness', ImageEnhance.Brightness),
                               ('color', ImageEnhance.Color)):
            if rec[name] is not None:
                pil = enhancer(pil).enhance(rec[name])
        im = np.asarray(pil)
        if rec['gray']:
            f = im.astype(np.float32)
            g = (np.float32(0.2989) * f[..., 0] + np.float32(0.5870) * f[..., 1] + np.float32(0.1140) * f[..., 2]).astype(np.uint8)
            im = np.repeat(g[..., None], 3, axis=2)
    return im.transpose(2, 0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--backgrounds', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20, help='augment_batch calls per timed window')
    ap.add_argument('--no-pillow', action='store_true')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build
    from cosypose_amd.augmentations import augment_batch, draw_sample_params, pack_params
    assert torch.cuda.is_available(), 'bench_aug.py needs a ROCm device'
    B, H, W = args.batch, args.height, args.width
    images, masks, backgrounds = make_inputs(args.seed, B, H, W, args.backgrounds)
    rng = random.Random(args.seed)
    recs = [draw_sample_params(rng, rgb_augmentation=True, gray_augmentation=True, n_backgrounds=args.backgrounds) for _ in range(B)]
    d = lambda a: torch.from_numpy(a).cuda()
    images_d, masks_d, backgrounds_d = d(images), d(masks), d(backgrounds)
    table_d = d(pack_params(recs).view(np.int32).reshape(B, 8))
    out_d = torch.empty_like(images_d)
    call = lambda: augment_batch(images_d, table_d, masks=masks_d, backgrounds=backgrounds_d, out=out_d)

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

    plane = 3 * H * W
    gated = sum(r['gate'] for r in recs)
    pasted = sum(r['bg'] >= 0 for r in recs)
    # gate off: read + write once.  gate on: images read, T1 written and read, T2 written and read, out written.  A paste reads the mask and the background too.
    min_bytes = (B - gated) * 2 * plane + gated * 6 * plane + pasted * (H * W + plane)

    pillow_fps = pillow_equal = pillow_ms_per_frame = None
    try:
        import PIL
        have_pil = not args.no_pillow
    except ImportError:
        have_pil = False
    if have_pil:
        torch.set_num_threads(1)
        pillow_chain(images[0], recs[0], masks[0], backgrounds)
        t0 = time.perf_counter()
        ref = [pillow_chain(images[b], recs[b], masks[b], backgrounds) for b in range(B)]
        dt = time.perf_counter() - t0
        pillow_fps, pillow_ms_per_frame = B / dt, 1e3 * dt / B
        pillow_equal = bool(all(np.array_equal(r, g) for r, g in zip(ref, got)))
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'training augmentations, augmentations.augment_batch (one call, one batch)', 'value': round(ms, 4), 'unit': 'ms/call', 'higher_is_better': False,
        'runs_ms': [round(r, 4) for r in runs], 'frames_per_s': round(B / (ms * 1e-3), 1), 'min_bytes_moved': int(min_bytes),
        'min_bytes_per_s': round(min_bytes / (ms * 1e-3), 1),
        'pillow_frames_per_s': None if pillow_fps is None else round(pillow_fps, 2),
        'pillow_ms_per_frame_one_core': None if pillow_ms_per_frame is None else round(pillow_ms_per_frame, 3),
        'pillow_version': PIL.__version__ if have_pil else None, 'pillow_equal': pillow_equal,
        'speedup_vs_pillow_one_core': None if pillow_fps is None else round(B / (ms * 1e-3) / pillow_fps, 1),
        'config': {'seed': args.seed, 'batch': B, 'height': H, 'width': W, 'backgrounds': args.backgrounds, 'warmup': args.warmup, 'runs': args.runs,
                   'iters': args.iters, 'gated': int(gated), 'pasted': int(pasted),
                   'stages': {n: int(sum(r[n] is not None for r in recs)) for n in ('sharpness', 'contrast', 'brightness', 'color')},
                   'gray': int(sum(r['gray'] for r in recs)), 'k': [int(sum(r['k'] == k for r in recs)) for k in (1, 2, 3)]},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()

"""One training step of the whole detector, and the optimiser's share of it.

Workload: `--frames` uint8 frames of `--height` x `--width` with `--gt` ground truths (boxes, labels, masks) each, a ResNet-50 + FPN Mask R-CNN
with random weights, trunk (from layer2 on) and heads trainable on bfloat16 rows under float32 master weights.  Two detectors are built from
the same state dict and timed in this process:
  (a) `flat`:  FlatSGD.zero_grad -> Detector.losses -> backward -> FlatSGD.step (norm, update, ONE launch that repacks every layer);
  (b) `torch`: the route before FlatSGD: Detector.zero_grad -> losses -> backward -> clip_grad_norm_(inf) -> torch.optim.SGD.step, and the
      per-layer packs of the next forward.
`ms`: the median WALL time of `--runs` calls after `--warmup` (synchronised before and after).  The optimiser's share is timed on its own, on
the gradients the last backward left: FlatSGD.step() against clip_grad_norm_ + torch.optim.SGD.step() + layer.refresh() over all layers (the
packs the next forward would launch).  Launches: FlatSGD.step's are read off its code (two of the norm, the update, the table); the torch
route's are the kernels torch.profiler sees in clip_grad_norm_ + step, plus one pack per layer.
`equal`: one step on both routes from the same state and the same gradients; the parameters agree within twice the first-order bound of the
update's three roundings (torch's kernels may fuse a product into a sum: both are within the bound of the exact update), and with route (a)'s
parameters loaded into route (b)'s detector -- whose layers then pack one by one -- the five maps and the heads' outputs of both are equal bits:
the table's launch writes the per-layer packs' bytes.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import statistics
import time

from bench_dethead import build_modules
from bench_dettrunk import build_backbone

U = 2.0 ** -24


def state_dict(seed, n_classes):
    import torch
    from cosypose_amd.detector_heads import BOX_KEYS, MASK_KEYS, RPN_KEYS
    gen = torch.Generator().manual_seed(seed)
    sd = {f'backbone.{k}': v for k, v in build_backbone(gen).state_dict().items()}
    rpn, box, box_pred, mask, mask_pred = build_modules(256, 3, 1024, n_classes, gen)
    mods = [(RPN_KEYS[0], rpn.conv), (RPN_KEYS[1], rpn.cls_logits), (RPN_KEYS[2], rpn.bbox_pred), (BOX_KEYS[0], box.fc6), (BOX_KEYS[1], box.fc7),
            (BOX_KEYS[2], box_pred.cls_score), (BOX_KEYS[3], box_pred.bbox_pred)] + [(MASK_KEYS[i], getattr(mask, f'mask_fcn{i + 1}')) for i in range(4)] + [
            (MASK_KEYS[4], mask_pred.conv5_mask), (MASK_KEYS[5], mask_pred.mask_fcn_logits)]
    for key, m in mods:
        sd[f'{key}.weight'], sd[f'{key}.bias'] = m.weight.detach(), m.bias.detach()
    return sd


def workload(args, n_classes):
    import torch
    gen = torch.Generator().manual_seed(args.seed + 1)
    B, H, W, G = args.frames, args.height, args.width, args.gt
    frames = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=gen).cuda() for _ in range(B)]
    targets = []
    for _ in range(B):
        w, h = torch.randint(40, 200, (G,), generator=gen), torch.randint(40, 200, (G,), generator=gen)
        x1, y1 = (torch.rand(G, generator=gen) * (W - w)).floor(), (torch.rand(G, generator=gen) * (H - h)).floor()
        boxes = torch.stack([x1, y1, x1 + w, y1 + h], 1).float()
        masks = torch.zeros(G, H, W, dtype=torch.uint8)
        for m, (a, b, c, d) in zip(masks, boxes.long().tolist()):
            m[b:d, a:c] = 1
        targets.append(dict(boxes=boxes.cuda(), labels=torch.randint(1, n_classes, (G,), generator=gen).cuda(), masks=masks.cuda()))
    return frames, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--gt', type=int, default=20)
    ap.add_argument('--classes', type=int, default=22)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import torch
    from cosypose_amd import Detector, build
    assert torch.cuda.is_available(), 'bench_detstep.py needs a ROCm device'
    BF16 = torch.bfloat16
    HYPER = dict(lr=0.02, momentum=0.9, weight_decay=1e-4)
    sd = state_dict(args.seed, args.classes)
    labels = {f'obj_{i:06d}': i for i in range(1, args.classes)}
    make = lambda: Detector.from_state_dict(sd, labels, input_resize=(args.height, args.width), trainable=True, train_dtype=BF16, heads_train_dtype=BF16)
    flat_det, torch_det = make(), make()
    flat_opt = flat_det.optimizer(**HYPER)
    torch_opt = torch.optim.SGD(torch_det.parameters(), **HYPER)
    layers = flat_opt.layers
    torch_layers = [l for l in torch_det.trunk.layers() + torch_det.heads.layers() if hasattr(l, 'refresh')]
    assert len(layers) == len(torch_layers)
    frames, targets = workload(args, args.classes)
    keys_gen = torch.Generator(device='cuda')

    def backward(det):
        keys_gen.manual_seed(args.seed)                                  # the same sampler keys on every call and on both routes
        sum(det.losses(frames, targets, generator=keys_gen).values()).backward()

    def flat_step():
        flat_opt.zero_grad()
        backward(flat_det)
        return flat_opt.step()

    def torch_share():
        norm = torch.nn.utils.clip_grad_norm_(torch_det.parameters(), max_norm=float('inf'), norm_type=2)
        torch_opt.step()
        return norm

    def torch_step():
        torch_det.zero_grad()
        backward(torch_det)
        return torch_share()

    def refresh_all():
        for l in torch_layers:
            l.refresh()

    def forward(det):
        g = torch.Generator(device='cuda').manual_seed(args.seed + 2)
        with torch.no_grad():
            maps = det.trunk(torch.randn(2, 3, 224, 288, generator=g, device='cuda'))
            obj, dlt = det.heads.rpn_head(maps)
            out = list(maps) + list(obj) + list(dlt) + list(det.heads.box_head(torch.randn(64, 256, 7, 7, generator=g, device='cuda')))
            return out + [det.heads.mask_head(torch.randn(16, 256, 14, 14, generator=g, device='cuda'))]

    # ---- equal: one step on both routes from the same state and the same gradients ----
    flat_opt.zero_grad()
    backward(flat_det)
    flat_opt._collect_stray_gradients()
    w0, g0 = flat_opt.flat.double().clone(), flat_opt.grad.double().clone()
    torch_det.zero_grad()
    for p, q in zip(torch_det.parameters(), flat_det.parameters()):
        p.grad = q.grad.detach().clone()
    norm_flat = float(flat_opt.step())
    norm_torch = float(torch_share())
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    lr, wd = f32(HYPER['lr']), f32(HYPER['weight_decay'])
    d = g0 + wd * w0                                                     # the first step: m' = d
    bound = 1.01 * (lr * U * ((wd * w0).abs() + d.abs()) + U * ((lr * d).abs() + (w0 - lr * d).abs()))
    share = 0.0
    for p, q in zip(torch_det.parameters(), flat_det.parameters()):
        o = (q.data_ptr() - flat_opt.flat.data_ptr()) // 4
        err = (p.detach().double() - q.detach().double()).abs().reshape(-1)
        share = max(share, float((err / (2 * bound[o:o + p.numel()]).clamp_min(1e-300)).max()))
    out_flat = forward(flat_det)                                         # packings written by the table's launch
    torch_det.load_state_dict(flat_det.state_dict())                    # route (a)'s parameters, packed layer by layer
    out_torch = forward(torch_det)
    maps_equal = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out_flat, out_torch))
    equal = bool(maps_equal and share <= 1.0 and abs(norm_flat - norm_torch) <= 1e-5 * norm_torch)

    def wall(call, runs=args.runs, before=None):
        for _ in range(args.warmup):
            if before is not None:
                before()
            call()
        out = []
        for _ in range(runs):
            if before is not None:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(out), 3), [round(v, 3) for v in out]

    flat_ms, flat_runs = wall(flat_step)
    torch_ms, torch_runs = wall(torch_step)
    # the parent route's step leaves its packs to the next forward: the whole step with them
    torch_packed_ms, torch_packed_runs = wall(lambda: (torch_step(), refresh_all()))
    # ---- the optimiser's share, on the gradients the last backward left ----
    share_runs = max(args.runs, 11)
    flat_share_ms, flat_share_runs = wall(flat_opt.step, share_runs)
    count0 = torch_det.trunk.pack_count + torch_det.heads.pack_count
    torch_share_ms, torch_share_runs = wall(lambda: (torch_share(), refresh_all()), share_runs)
    packs_per_step = (torch_det.trunk.pack_count + torch_det.heads.pack_count - count0) // (share_runs + args.warmup)
    torch_opt_ms, _ = wall(torch_share, share_runs)
    torch_kernels = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            torch_share()
            torch.cuda.synchronize()
        torch_kernels = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and not e.name.lower().startswith('memcpy'))
    except Exception as e:                                               # the count is a report, the timings do not depend on it
        torch_kernels = None
        print(f'torch.profiler: {type(e).__name__}: {e}', flush=True)

    stamp = build.read_stamp() or {}
    result = {
        'metric': 'detector training step, bfloat16 rows under float32 master weights: ResNet-50 + FPN Mask R-CNN, losses + backward + FlatSGD.step, median wall time',
        'value': flat_ms, 'unit': 'ms', 'higher_is_better': False, 'runs_ms': flat_runs,
        'torch_sgd_ms': torch_ms, 'torch_sgd_runs_ms': torch_runs, 'torch_sgd_with_packs_ms': torch_packed_ms, 'torch_sgd_with_packs_runs_ms': torch_packed_runs,
        'optimizer_share': {'flat_sgd_step_ms': flat_share_ms, 'flat_sgd_step_runs_ms': flat_share_runs,
                            'torch_sgd_clip_and_packs_ms': torch_share_ms, 'torch_sgd_clip_and_packs_runs_ms': torch_share_runs, 'torch_sgd_clip_ms': torch_opt_ms,
                            'speedup': round(torch_share_ms / flat_share_ms, 2), 'flat_sgd_step_slower': bool(flat_share_ms > torch_share_ms)},
        'launches': {'flat_sgd_step': 4, 'torch_sgd_clip_kernels': torch_kernels, 'per_layer_packs': int(packs_per_step),
                     'torch_route': None if torch_kernels is None else int(torch_kernels + packs_per_step)},
        'layers': len(layers), 'parameters': int(sum(p.numel() for p in flat_det.parameters())), 'flat_elements': int(flat_opt.flat.numel()),
        'equal': equal, 'maps_equal_bits': bool(maps_equal), 'largest_share_of_parameter_bound': share, 'grad_norm': [norm_flat, norm_torch],
        'speedup_whole_step': round(torch_packed_ms / flat_ms, 3), 'slower_whole_step': bool(flat_ms > torch_packed_ms),
        'not_measured': ['a kernel trace of the step', 'hardware counters (memory traffic of the update and of the table\'s launch)', 'other batch sizes and frame sizes',
                         'more than one rank (the all-reduce of the flat gradient)'],
        'config': {'seed': args.seed, 'frames': args.frames, 'height': args.height, 'width': args.width, 'gt': args.gt, 'classes': args.classes, 'runs': args.runs,
                   'share_runs': share_runs, 'warmup': args.warmup, 'train_from_stage': 2, 'train_dtype': 'bfloat16', 'heads_train_dtype': 'bfloat16', **HYPER},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()

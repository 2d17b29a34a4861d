#!/usr/bin/env python3
"""Timing of the detector trunk's training step (forward + backward of cosypose_amd.DetectorTrunk with trainable=True, csrc/kernels_dettrunk.hip
and csrc/kernels_detbwd.hip) on one GPU, float32, at bench_dettrunk.py's shape: 8 frames padded to 800x1088 through ResNet-50 + FPN, with
gradients arriving at the four maps.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 900 python bench_dettrunkbwd.py --out profiles/dettrunkbwd_bench.json

`ms`: the median WALL time of `--runs` forward + backward calls after `--warmup` (synchronised before and after), against the same network as
torch.nn modules with autograd and the same requires_grad set (body.layer2.., the FPN) on the device in float32, in the same process
(`torch_ms`: MIOpen).  No time is a pass criterion: DESIGN.md section 28 measured the weight-gradient kernel at about half of torch's speed
(its operands are not staged through LDS) and this backward inherits that load path; `slower_than_torch_ops` says how it came out.
`split_ms`: the device time of the body's data-gradient launches, the body's weight-gradient launches and the FPN's backward, from events
around the three groups of one backward.  `kept_bytes`: the rows one forward holds for its backward.
`equal`: each of layer2.0's four layers alone on a subsample (a (1,256,24,32) input) meets DESIGN.md section 29's bounds against float64
torch.autograd on the CPU: |dW - dW64| <= (T + 3) u |scale| S_W, |dX - dX64| <= (K + 3) u S (`largest_share_of_bound`).
Not measured: the kernels alone without the host's share; memory traffic; LDS staging of the weight gradient (not built); 16-bit training
(not built).

    timeout -k 10 900 python bench_dettrunkbwd.py --train-dtype bfloat16

prints the same line for DESIGN.md section 30's path (bfloat16 rows and packed weights, float32 master weights; csrc/kernels_detbwd16.hip) at the
same shape and writes it to profiles/dettrunkbwd16_bench.json.  `torch_ms`: the same torch.nn modules under torch.autocast('cuda',
torch.bfloat16) with the same requires_grad set, in the same process; `float32_ms`: the float32 step of the same build; `kept_bytes` beside
`float32_kept_bytes`; `equal`: layer2.0's four layers alone on the subsample, fed bf16-exact operands, inside section 30's bounds against
float64: |dW - dW64| <= (T + 3) 2^-23 |scale| S_W, |dX - dX64| <= b + 2^-8 (|dX64| + b) with b = (K + 2) 2^-23 S."""
import argparse
import contextlib
import json
import statistics
import time

from bench_dettrunk import build_backbone

U = 2.0 ** -24
U16 = 2.0 ** -23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1088)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    ap.add_argument('--train-dtype', choices=['bfloat16'], default=None, help='time DESIGN.md section 30\'s bfloat16 path instead (writes profiles/dettrunkbwd16_bench.json)')
    args = ap.parse_args()
    if args.train_dtype:
        return main16(args)

    import torch
    import torch.nn.functional as F
    from cosypose_amd import build
    from cosypose_amd.detector_trunk import DetectorTrunk
    from cosypose_amd.detector_trunk_backward import layer_dgrad, layer_wgrad
    assert torch.cuda.is_available(), 'bench_dettrunkbwd.py needs a ROCm device'
    B, H, W = args.frames, args.height, args.width
    model = build_backbone(torch.Generator().manual_seed(args.seed))
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    images = torch.randn((B, 3, H, W), generator=gen, device='cuda')
    trunk = DetectorTrunk.from_modules(model, device='cuda', trainable=True, train_from_stage=2)
    dev_model = build_backbone(torch.Generator().manual_seed(args.seed))
    dev_model.load_state_dict(model.state_dict())
    dev_model.to('cuda')
    t_params = [p for k, p in dev_model.named_parameters() if k.startswith('fpn.') or (k.startswith('body.layer') and not k.startswith('body.layer1.'))]
    for p in t_params:
        p.requires_grad_(True)
    assert len(t_params) == len(trunk.parameters())
    grads = []

    def step(ours):
        params = trunk.parameters() if ours else t_params
        for p in params:
            p.grad = None
        out = (trunk if ours else dev_model)(images)[:4]
        if not grads:
            grads.extend(torch.randn(o.shape, generator=gen, device='cuda') for o in out)
        torch.autograd.backward(list(out), grads)

    def wall(call):
        for _ in range(args.warmup):
            call()
        out = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(out), 3), [round(v, 3) for v in out]

    def split():
        spans = {'dgrad': [], 'wgrad': [], 'fpn': []}

        @contextlib.contextmanager
        def timer(group):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            yield
            e1.record()
            spans[group].append((e0, e1))
        trunk.timer = timer
        try:
            step(True)
            torch.cuda.synchronize()
        finally:
            trunk.timer = None
        return {'body_dgrad': round(sum(a.elapsed_time(b) for a, b in spans['dgrad']), 3), 'body_wgrad': round(sum(a.elapsed_time(b) for a, b in spans['wgrad']), 3),
                'fpn': round(sum(a.elapsed_time(b) for a, b in spans['fpn']), 3)}

    def layer_check(layer, conv, bn, x, on_output_grid=False):
        """one layer alone on the subsample x (CPU float32) -> the largest share of its two bounds"""
        scale = (bn.weight * bn.running_var.rsqrt()).float()
        w64, x64, s64 = conv.weight.detach().double(), x.double(), scale.double().reshape(1, -1, 1, 1)
        stride, pad = conv.stride, conv.padding
        y = F.conv2d(x64, w64, None, stride, pad)
        g = torch.randn(y.shape, generator=torch.Generator().manual_seed(args.seed + 1), dtype=torch.float64).float()

        def grads64(xx, ww, gg):
            xx, ww = xx.clone().requires_grad_(), ww.clone().requires_grad_()
            F.conv2d(xx, ww, None, stride, pad).backward(gg)
            return xx.grad, ww.grad
        dx64, dw64 = grads64(x64, w64, g.double() * s64)
        Sx, Sw = grads64(x64.abs(), w64.abs(), g.double().abs() * s64.abs())
        T, K = g.shape[0] * g.shape[2] * g.shape[3], w64.shape[0] * w64.shape[2] * w64.shape[3]
        share = lambda got, want, bound: float(((got.cpu().double() - want).abs() / bound.clamp(min=1e-300)).max())
        dw = layer_wgrad(layer, x.cuda().contiguous(), g.cuda())[0]
        if on_output_grid:      # downsample.0: the data gradient runs at stride 1 on the output grid; its rows are the even cells of dX
            dx = layer_dgrad(layer, g.cuda(), g.shape[2], g.shape[3], stride=1)
            dx64, Sx = dx64[..., ::2, ::2], Sx[..., ::2, ::2]
        else:
            dx = layer_dgrad(layer, g.cuda(), x.shape[2], x.shape[3])
        return max(share(dw, dw64, (T + 3) * U * Sw), share(dx, dx64, (K + 3) * U * Sx))

    blk, b = trunk.block(2, 0), model.body.layer2[0]
    cpu = torch.Generator().manual_seed(args.seed + 2)
    x = torch.randn((1, 256, 24, 32), generator=cpu)
    share = max(layer_check(blk.conv1, b.conv1, b.bn1, x), layer_check(blk.conv2, b.conv2, b.bn2, torch.randn((1, 128, 24, 32), generator=cpu)),
                layer_check(blk.conv3, b.conv3, b.bn3, torch.randn((1, 128, 12, 16), generator=cpu)),
                layer_check(blk.downsample, b.downsample[0], b.downsample[1], x, on_output_grid=True))
    ms, runs = wall(lambda: step(True))
    kept = trunk.last_kept_bytes
    parts = split()
    torch.cuda.empty_cache()
    t_ms, t_runs = wall(lambda: step(False))
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'detector trunk, float32: forward + backward of ResNet-50 + FPN trained from layer2 on, median wall time of one call',
        'value': ms, 'unit': 'ms', 'higher_is_better': False, 'runs_ms': runs, 'torch_ms': t_ms, 'torch_runs_ms': t_runs,
        'split_ms': parts, 'kept_bytes': int(kept), 'equal': bool(share <= 1.0), 'largest_share_of_bound': share,
        'speedup_vs_torch_ops': round(t_ms / ms, 2), 'slower_than_torch_ops': ms > t_ms, 'pack_count': trunk.pack_count,
        'not_measured': ['kernel time without the host\'s share', 'memory traffic', 'LDS staging of the weight gradient (not built)', '16-bit training (not built)'],
        'config': {'seed': args.seed, 'frames': B, 'height': H, 'width': W, 'train_from_stage': 2, 'runs': args.runs, 'warmup': args.warmup},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


def main16(args):
    import torch
    import torch.nn.functional as F
    from cosypose_amd import build
    from cosypose_amd.detector_trunk import DetectorTrunk
    from cosypose_amd.detector_trunk_backward import layer_dgrad, layer_wgrad
    assert torch.cuda.is_available(), 'bench_dettrunkbwd.py needs a ROCm device'
    BF16 = torch.bfloat16
    B, H, W = args.frames, args.height, args.width
    model = build_backbone(torch.Generator().manual_seed(args.seed))
    gen = torch.Generator(device='cuda').manual_seed(args.seed)
    images = torch.randn((B, 3, H, W), generator=gen, device='cuda')
    trunk = DetectorTrunk.from_modules(model, device='cuda', trainable=True, train_from_stage=2, train_dtype=BF16)
    trunk32 = DetectorTrunk.from_modules(model, device='cuda', trainable=True, train_from_stage=2)
    dev_model = build_backbone(torch.Generator().manual_seed(args.seed))
    dev_model.load_state_dict(model.state_dict())
    dev_model.to('cuda')
    t_params = [p for k, p in dev_model.named_parameters() if k.startswith('fpn.') or (k.startswith('body.layer') and not k.startswith('body.layer1.'))]
    for p in t_params:
        p.requires_grad_(True)
    assert len(t_params) == len(trunk.parameters()) == len(trunk32.parameters())
    grads = []

    def step(which):
        params = t_params if which == 'torch' else (trunk if which == 'bf16' else trunk32).parameters()
        for p in params:
            p.grad = None
        if which == 'torch':
            with torch.autocast('cuda', BF16):
                out = dev_model(images)[:4]
        else:
            out = (trunk if which == 'bf16' else trunk32)(images)[:4]
        if not grads:
            grads.extend(torch.randn(o.shape, generator=gen, device='cuda') for o in out)
        torch.autograd.backward(list(out), [g.to(o.dtype) for g, o in zip(grads, out)])

    def wall(call):
        for _ in range(args.warmup):
            call()
        out = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(out), 3), [round(v, 3) for v in out]

    def split():
        spans = {'dgrad': [], 'wgrad': [], 'fpn': []}

        @contextlib.contextmanager
        def timer(group):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            yield
            e1.record()
            spans[group].append((e0, e1))
        trunk.timer = timer
        try:
            step('bf16')
            torch.cuda.synchronize()
        finally:
            trunk.timer = None
        return {'body_dgrad': round(sum(a.elapsed_time(b) for a, b in spans['dgrad']), 3), 'body_wgrad': round(sum(a.elapsed_time(b) for a, b in spans['wgrad']), 3),
                'fpn': round(sum(a.elapsed_time(b) for a, b in spans['fpn']), 3)}

    r16 = lambda t: t.to(BF16).to(t.dtype)

    def layer_check(layer, conv, bn, x, on_output_grid=False):
        """one layer alone on the subsample x (CPU float32, rounded to bfloat16 like g) -> the largest share of its two bounds"""
        scale = (bn.weight * bn.running_var.rsqrt()).float()
        x = r16(x)
        ws64 = r16(conv.weight.detach().float() * scale.reshape(-1, 1, 1, 1)).double()          # what cosy_trunk_weight_pack16 packs
        x64, s64 = x.double(), scale.double().reshape(-1, 1, 1, 1)
        stride, pad = conv.stride, conv.padding
        y = F.conv2d(x64, ws64, None, stride, pad)
        g = r16(torch.randn(y.shape, generator=torch.Generator().manual_seed(args.seed + 1), dtype=torch.float64).float())

        def grads64(xx, ww, gg):
            xx, ww = xx.clone().requires_grad_(), ww.clone().requires_grad_()
            F.conv2d(xx, ww, None, stride, pad).backward(gg)
            return xx.grad, ww.grad
        dx64, _ = grads64(x64, ws64, g.double())
        Sx, _ = grads64(x64.abs(), ws64.abs(), g.double().abs())
        _, dw64 = grads64(x64, ws64, g.double())
        _, Sw = grads64(x64.abs(), ws64.abs(), g.double().abs())
        dw64, Sw = dw64 * s64, Sw * s64.abs()                                                 # dW = scale[o] sum g x: the sums do not depend on the weight
        T, K = g.shape[0] * g.shape[2] * g.shape[3], ws64.shape[0] * ws64.shape[2] * ws64.shape[3]
        share = lambda got, want, bound: float(((got.cpu().double() - want).abs() / bound.clamp(min=1e-300)).max())
        dw = layer_wgrad(layer, x.cuda().contiguous(), g.cuda())[0]
        if on_output_grid:      # downsample.0: the data gradient runs at stride 1 on the output grid; its rows are the even cells of dX
            dx = layer_dgrad(layer, g.cuda(), g.shape[2], g.shape[3], stride=1)
            dx64, Sx = dx64[..., ::2, ::2], Sx[..., ::2, ::2]
        else:
            dx = layer_dgrad(layer, g.cuda(), x.shape[2], x.shape[3])
        b = (K + 2) * U16 * Sx
        return max(share(dw, dw64, (T + 3) * U16 * Sw), share(dx, dx64, b + 2.0 ** -8 * (dx64.abs() + b)))

    blk, b = trunk.block(2, 0), model.body.layer2[0]
    cpu = torch.Generator().manual_seed(args.seed + 2)
    x = torch.randn((1, 256, 24, 32), generator=cpu)
    share = max(layer_check(blk.conv1, b.conv1, b.bn1, x), layer_check(blk.conv2, b.conv2, b.bn2, torch.randn((1, 128, 24, 32), generator=cpu)),
                layer_check(blk.conv3, b.conv3, b.bn3, torch.randn((1, 128, 12, 16), generator=cpu)),
                layer_check(blk.downsample, b.downsample[0], b.downsample[1], x, on_output_grid=True))
    ms, runs = wall(lambda: step('bf16'))
    kept = trunk.last_kept_bytes
    parts = split()
    torch.cuda.empty_cache()
    f_ms, f_runs = wall(lambda: step('f32'))
    kept32 = trunk32.last_kept_bytes
    torch.cuda.empty_cache()
    t_ms, t_runs = wall(lambda: step('torch'))
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'detector trunk, bfloat16 rows under float32 master weights: forward + backward of ResNet-50 + FPN trained from layer2 on, median wall time of one call',
        'value': ms, 'unit': 'ms', 'higher_is_better': False, 'runs_ms': runs, 'torch_ms': t_ms, 'torch_runs_ms': t_runs, 'torch': 'torch.autocast(cuda, bfloat16)',
        'float32_ms': f_ms, 'float32_runs_ms': f_runs, 'split_ms': parts, 'kept_bytes': int(kept), 'float32_kept_bytes': int(kept32),
        'equal': bool(share <= 1.0), 'largest_share_of_bound': share,
        'speedup_vs_torch_ops': round(t_ms / ms, 2), 'slower_than_torch_ops': ms > t_ms, 'speedup_vs_float32': round(f_ms / ms, 2), 'slower_than_float32': ms > f_ms,
        'pack_count': trunk.pack_count,
        'not_measured': ['kernel time without the host\'s share', 'memory traffic', 'LDS bank conflicts of the weight gradient (predicted, no counter run)', 'bfloat16 heads (not built)'],
        'config': {'seed': args.seed, 'frames': B, 'height': H, 'width': W, 'train_from_stage': 2, 'runs': args.runs, 'warmup': args.warmup, 'train_dtype': 'bfloat16'},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    out = args.out or 'profiles/dettrunkbwd16_bench.json'
    with open(out, 'w') as f:
        f.write(json.dumps(result, indent=1) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
